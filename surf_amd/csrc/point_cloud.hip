// Fused point clouds (surf_amd/fusion.py fuse_points): the depth maps of many views merged into ONE cloud with one point per
// surface sample - the merge of Gipuma's fusibile, the fusion most MVSNet-family results use, stated with this project's
// consistency rule (depth_filter.hip).  A pixel that enough other views agree with is emitted once, and the pixels of those
// views that saw the same surface sample are marked so that they are not emitted again when their own view's turn comes.
//
// State: per view v a map used[v] (H_v, W_v) uint8, all zero at the start.  Views are visited in index order r = 0 .. n-1; each
// pixel (x, y) of r is independent of the others:
//   1. candidate:   d = depth_r[y, x] * dscale_r is measured (d > 0 and d <= FLT_MAX) and used[r][y, x] == 0
//        (points_candidates_kernel: cand = used ? 0 : depth_r, so that everything below sees a used pixel as no measurement)
//   2. every source s of sources[r], in the order given: the round-trip rule of depth_filter.hip's header comment, verbatim
//        (surf_consistency_rule in consistency_rule.h, the one copy: u, sx, sy, the four measured taps, ds, w, e2 < px2 and
//        rel < rel_thresh, px2 formed on the host); the source maps are read as they are - a used pixel still supports others.
//        On agreement   count += 1;  zsum += w.z   (surf_depth_consistency on cand, more than 16 sources as further launches)
//        and the source's matched pixel is (mx, my) = (rintf(sx), rintf(sy)), round half to even: in range because
//        0 <= sx <= Ws-1 and 0 <= sy <= Hs-1, and one of the four measured taps.
//   3. accept iff count >= min_consistent            (surf_depth_consistency_finish's keep; min_consistent = 0: every candidate)
//   4. on acceptance
//        used[s][my, mx] = 1 for every agreeing source s          (points_mark_kernel: re-runs the rule at the accepted pixels)
//        z  = average ? (zsum + d) / (float)(count + 1) : d
//        qx = (float)x * z;  qy = (float)y * z
//        X_k = ((Minv[k][0] * qx + Minv[k][1] * qy) + Minv[k][2] * z) + c[k]      k = 0, 1, 2   (points_lift_kernel)
//        with Minv = M_r^-1 and c = -M_r^-1 t_r for P_r = [M_r | t_r], formed in float64 on the host and rounded to fp32 once:
//        there is no fp32 subtraction of the large t_r.
//        colour (when the views carry images) = image_r[y, x] per channel:  q = c * 256;  q = fmin(fmax(q, 0), 255);  (uint8)q
//        (fuse_vertex_colors_kernel's quantisation);   origin = (r, y * W + x)
//   5. output order: by view index, then row-major pixel index (the lift runs over the ordered list of accepted pixels).
// Launches for consecutive r run in order on one stream.  A launch for r reads used[r] and writes only used[s], s != r, and the
// writes are idempotent byte stores of 1: the result is deterministic.
// All three are gather / bandwidth kernels: 256-thread blocks, no LDS, one thread per pixel (mark: the accepted pixels are
// usually most of the measured ones, so a list would not be shorter than the map).
#include "consistency_rule.h"

namespace {

struct MarkMaps { uint8_t* used[SURF_FUSE_MAX_VIEWS]; };
struct Lift { float Minv[9], c[3]; };

__global__ __launch_bounds__(256) void points_candidates_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ used,
                                                                int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = used[i] ? 0.0f : depth[i];
}

__global__ __launch_bounds__(256) void points_mark_kernel(const float* __restrict__ cand_r, int H, int W, float dscale_r,
                                                          const uint8_t* __restrict__ keep, FilterSources sources, MarkMaps maps,
                                                          int n_sources, float px2, float rel_thresh) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)H * (uint32_t)W) return;
  if (!keep[i]) return;
  const float d = cand_r[i] * dscale_r;
  if (!surf_measured(d)) return;                                // keep implies it; the rule below divides by d
  const int y = (int)(i / (uint32_t)W), x = (int)(i - (uint32_t)y * (uint32_t)W);
  const float xf = (float)x, yf = (float)y;
  const float qx = xf * d, qy = yf * d, qz = d;
  for (int s = 0; s < n_sources; ++s) {
    float wz, sx, sy;
    if (!surf_consistency_rule(sources.s[s], xf, yf, d, qx, qy, qz, px2, rel_thresh, &wz, &sx, &sy)) continue;
    const int mx = (int)rintf(sx), my = (int)rintf(sy);         // 0 <= sx <= Ws-1, 0 <= sy <= Hs-1: so are their roundings
    maps.used[s][(int64_t)my * sources.s[s].W + mx] = 1;
  }
}

template <bool COLOR>
__global__ __launch_bounds__(256) void points_lift_kernel(const float* __restrict__ cand_r, int W, int64_t n_pixels, float dscale_r,
                                                          const int32_t* __restrict__ count, const float* __restrict__ zsum,
                                                          int average, const int64_t* __restrict__ kept, int64_t n_kept, Lift L,
                                                          const float* __restrict__ image, int view, float* __restrict__ points,
                                                          uint8_t* __restrict__ colors, int32_t* __restrict__ origin) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_kept) return;
  const int64_t i = kept[k];
  if (i < 0 || i >= n_pixels) return;                           // not a pixel of this map: nothing is read or written for it
  const int y = (int)((uint32_t)i / (uint32_t)W), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)W);
  const float d = cand_r[i] * dscale_r;
  const float z = average ? (zsum[i] + d) / (float)(count[i] + 1) : d;
  const float qx = (float)x * z, qy = (float)y * z;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    points[k * 3 + a] = ((L.Minv[3 * a + 0] * qx + L.Minv[3 * a + 1] * qy) + L.Minv[3 * a + 2] * z) + L.c[a];
  if (COLOR) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float q = image[i * 3 + c] * 256.0f;
      q = fminf(fmaxf(q, 0.0f), 255.0f);
      colors[k * 3 + c] = (uint8_t)q;
    }
  }
  origin[k * 2 + 0] = view;
  origin[k * 2 + 1] = (int32_t)i;
}

inline bool map_limits(int H, int W) {
  const int side_max = 1 << 24;                                 // (float)(side - 1) is exact
  return (int64_t)H * W < ((int64_t)1 << 31) && H <= side_max && W <= side_max;
}

}  // namespace

extern "C" int surf_points_candidates(const float* depth, const uint8_t* used, int64_t n, float* out, void* stream) {
  if (n == 0) return 0;
  if (!depth || !used || !out || n < 0) return SURF_E_ARG;
  if (n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(points_candidates_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, depth, used, n,
                     out);
  return surf_check_launch();
}

extern "C" int surf_points_mark(const float* cand_r, int H, int W, float dscale_r, const uint8_t* keep, const float* h_T,
                                const float* const* h_depths, uint8_t* const* h_used, const int* h_hw, const float* h_dscale,
                                int n_sources, float px2, float rel_thresh, void* stream) {
  if (H == 0 || W == 0 || n_sources == 0) return 0;
  if (!cand_r || !keep || !h_T || !h_depths || !h_used || !h_hw || !h_dscale) return SURF_E_ARG;
  if (H < 0 || W < 0 || n_sources < 0) return SURF_E_ARG;
  if (n_sources > SURF_FUSE_MAX_VIEWS) return SURF_E_LIMIT;
  if (!map_limits(H, W)) return SURF_E_LIMIT;
  FilterSources sources;
  const int bad = surf_fill_filter_sources(sources, h_T, h_depths, h_hw, h_dscale, n_sources);
  if (bad) return bad;
  MarkMaps maps;
  for (int s = 0; s < SURF_FUSE_MAX_VIEWS; ++s) maps.used[s] = s < n_sources ? h_used[s] : nullptr;
  for (int s = 0; s < n_sources; ++s)
    if (!maps.used[s]) return SURF_E_ARG;
  const unsigned blocks = (unsigned)(((int64_t)H * W + 255) / 256);
  hipLaunchKernelGGL(points_mark_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cand_r, H, W, dscale_r, keep, sources, maps,
                     n_sources, px2, rel_thresh);
  return surf_check_launch();
}

extern "C" int surf_points_lift(const float* cand_r, int H, int W, float dscale_r, const int32_t* count, const float* zsum,
                                int average, const int64_t* kept, int64_t n_kept, const float* h_lift, const float* image, int view,
                                float* points, uint8_t* colors, int32_t* origin, void* stream) {
  if (n_kept == 0 || H == 0 || W == 0) return 0;
  if (!cand_r || !count || !zsum || !kept || !h_lift || !points || !origin) return SURF_E_ARG;
  if (H < 0 || W < 0 || n_kept < 0 || view < 0 || (image && !colors)) return SURF_E_ARG;
  if (!map_limits(H, W) || n_kept > (int64_t)H * W) return SURF_E_LIMIT;
  Lift L;
  for (int e = 0; e < 9; ++e) L.Minv[e] = h_lift[e];
  for (int e = 0; e < 3; ++e) L.c[e] = h_lift[9 + e];
  const unsigned blocks = (unsigned)((n_kept + 255) / 256);
  const int64_t n_pixels = (int64_t)H * W;
  if (image)
    hipLaunchKernelGGL(points_lift_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cand_r, W, n_pixels, dscale_r, count,
                       zsum, average, kept, n_kept, L, image, view, points, colors, origin);
  else
    hipLaunchKernelGGL(points_lift_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cand_r, W, n_pixels, dscale_r, count,
                       zsum, average, kept, n_kept, L, image, view, points, colors, origin);
  return surf_check_launch();
}
