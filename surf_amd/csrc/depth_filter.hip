// Multi-view geometric consistency of depth maps (surf_amd/fusion.py filter_views): the cross-view check that decides which
// pixels of the rendered depth maps go into the fused lattice (fuse.hip).  The standard filter of this family of methods
// (MVSNet-style fusion): reproject a pixel into another view, read that view's depth there, reproject back, and keep the pixel
// only if enough views agree.  The test itself - round-trip error under 1 pixel, relative depth error under 1 % - is the one of
// the reference's models/losses/consistency_loss.py:43-52.
//
//  * depth_consistency_kernel: one thread per pixel of the reference map.  The sources of a launch (<= SURF_FUSE_MAX_VIEWS) are
//    looped INSIDE the kernel with the pixel's d, count and zsum in registers: the reference-side streams (depth read; count and
//    zsum read at measured pixels, written where a source agreed) are paid once per launch, the source maps are gathered through
//    the caches, four taps per (pixel, source).  The source table travels as a kernel argument (16 x 120 B).
//    Thread-to-pixel mapping (template parameter TW, the results do not depend on it): TW = 64: a wavefront covers 64
//    consecutive pixels of the flat index (best-coalesced reference streams, a long thin footprint in each source map);
//    TW = 16 / 8: a wavefront covers a 16 x 4 / 8 x 8 tile of a 32 x 8 block tile (a compact footprint in each source map).
//    The library is compiled with -ffp-contract=off; every line below is one fp32 operation per operator, in exactly this order
//    (surf_amd/fusion.py consistency_host mirrors it in numpy fp32 and the tests demand equality; the code is
//    surf_consistency_rule in consistency_rule.h, which point_cloud.hip includes too).  With P = [M | t] per view,
//    A_rs = M_s M_r^-1, b_rs = t_s - A_rs t_r (and A_sr, b_sr likewise), formed on the host in float64 and rounded once:
//        d  = depth_r[y, x] * dscale_r;     the pixel is "measured" iff d > 0 and d <= FLT_MAX   (else nothing is done)
//        q  = ((float)x * d, (float)y * d, d);      for each source s, in the order given:
//        u  = ((A0*qx + A1*qy) + A2*qz) + b0        (three rows of A_rs / b_rs);     skip s unless u.z > 0
//        sx = u.x / u.z;  sy = u.y / u.z            (IEEE division)
//        skip unless 0 <= sx <= Ws-1 and 0 <= sy <= Hs-1                            (float compares: a NaN fails)
//        x0 = floorf(sx); y0 = floorf(sy); fx = sx - x0; fy = sy - y0; x1 = min(x0+1, Ws-1); y1 = min(y0+1, Hs-1)
//        d00, d01, d10, d11 = depth_s[y0|y1, x0|x1] * dscale_s  (dYX);   skip unless all four are measured (no depth across holes)
//        top = d00 + (d01 - d00) * fx;  bot = d10 + (d11 - d10) * fx;  ds = top + (bot - top) * fy
//        v  = (sx * ds, sy * ds, ds);  w = A_sr v + b_sr  (grouped like u);          skip unless w.z > 0
//        ex = w.x / w.z - (float)x;  ey = w.y / w.z - (float)y;  e2 = ex*ex + ey*ey;  rel = fabsf(w.z - d) / d
//        consistent iff e2 < px2 and rel < rel_thresh       (px2 = px_thresh^2 formed on the host in fp32: no sqrt here)
//        count += 1;  zsum += w.z                           (fp32 sum, in source order)
//  * depth_consistency_finish_kernel, per pixel:
//        keep = measured and count >= min_consistent
//        out  = 0 where not kept; depth_r[y, x] unchanged where kept, or with `average`
//               ((zsum + d) / (float)(count + 1)) / dscale_r       (the mean over the reference and its agreeing sources)
// Both are bandwidth / gather kernels: 256-thread blocks, no LDS.
#include "consistency_rule.h"        // the rule itself (surf_consistency_rule), shared with point_cloud.hip

namespace {

template <int TW>
__global__ __launch_bounds__(256) void depth_consistency_kernel(const float* __restrict__ depth_r, int H, int W, float dscale_r,
                                                                FilterSources sources, int n_sources, float px2, float rel_thresh,
                                                                int32_t* __restrict__ count, float* __restrict__ zsum) {
  int x, y;
  if (TW == 64) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)H * (uint32_t)W) return;
    y = (int)(i / (uint32_t)W);
    x = (int)(i - (uint32_t)y * (uint32_t)W);
  } else {
    // a 32 x 8 block tile: TW = 16: four 16 x 4 wavefront tiles, 2 x 2; TW = 8: four 8 x 8 wavefront tiles side by side
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wx = TW == 16 ? (wave & 1) * 16 : wave * 8, wy = TW == 16 ? (wave >> 1) * 4 : 0;
    x = (int)blockIdx.x * 32 + wx + (lane & (TW - 1));
    y = (int)blockIdx.y * 8 + wy + lane / TW;
    if (x >= W || y >= H) return;
  }
  const int64_t i = (int64_t)y * W + x;
  const float d = depth_r[i] * dscale_r;
  if (!surf_measured(d)) return;
  const float xf = (float)x, yf = (float)y;
  const float qx = xf * d, qy = yf * d, qz = d;
  int cnt = count[i];
  float zs = zsum[i];
  const int cnt0 = cnt;
  for (int s = 0; s < n_sources; ++s) {
    float wz, sx, sy;
    if (!surf_consistency_rule(sources.s[s], xf, yf, d, qx, qy, qz, px2, rel_thresh, &wz, &sx, &sy)) continue;
    cnt += 1;
    zs = zs + wz;
  }
  if (cnt == cnt0) return;                                      // no source agreed: the pixel's state is unchanged, nothing to write
  count[i] = cnt;
  zsum[i] = zs;
}

__global__ __launch_bounds__(256) void depth_consistency_finish_kernel(const float* __restrict__ depth_r, float dscale_r,
                                                                       const int32_t* __restrict__ count,
                                                                       const float* __restrict__ zsum, int64_t n, int min_consistent,
                                                                       int average, float* __restrict__ out_depth,
                                                                       uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float raw = depth_r[i];
  const float d = raw * dscale_r;
  const int cnt = count[i];
  const bool k = surf_measured(d) && cnt >= min_consistent;
  float out = 0.0f;
  if (k) out = average ? ((zsum[i] + d) / (float)(cnt + 1)) / dscale_r : raw;
  out_depth[i] = out;
  keep[i] = k ? 1 : 0;
}

template <int TW>
void launch_consistency(const float* depth_r, int H, int W, float dscale_r, const FilterSources& sources, int n_sources, float px2,
                        float rel_thresh, int32_t* count, float* zsum, hipStream_t stream) {
  const dim3 grid = TW == 64 ? dim3((unsigned)(((int64_t)H * W + 255) / 256)) : dim3((unsigned)((W + 31) / 32), (unsigned)((H + 7) / 8));
  hipLaunchKernelGGL(depth_consistency_kernel<TW>, grid, dim3(256), 0, stream, depth_r, H, W, dscale_r, sources, n_sources, px2,
                     rel_thresh, count, zsum);
}

}  // namespace

extern "C" int surf_depth_consistency(const float* depth_r, int H, int W, float dscale_r, const float* h_T,
                                      const float* const* h_depths, const int* h_hw, const float* h_dscale, int n_sources, float px2,
                                      float rel_thresh, int32_t* count, float* zsum, int tile_w, void* stream) {
  const int side_max = 1 << 24;                                 // (float)(side - 1) is exact: the bounds test keeps every tap inside
  if (!depth_r || !h_T || !h_depths || !h_hw || !h_dscale || !count || !zsum) return SURF_E_ARG;
  if (H < 1 || W < 1 || n_sources < 1) return SURF_E_ARG;
  if (tile_w != 64 && tile_w != 16 && tile_w != 8) return SURF_E_ARG;
  if (n_sources > SURF_FUSE_MAX_VIEWS) return SURF_E_LIMIT;
  if ((int64_t)H * W >= ((int64_t)1 << 31) || H > side_max || W > side_max || (H + 7) / 8 > 65535) return SURF_E_LIMIT;
  FilterSources sources;
  const int bad = surf_fill_filter_sources(sources, h_T, h_depths, h_hw, h_dscale, n_sources);
  if (bad) return bad;
  if (tile_w == 64)
    launch_consistency<64>(depth_r, H, W, dscale_r, sources, n_sources, px2, rel_thresh, count, zsum, (hipStream_t)stream);
  else if (tile_w == 16)
    launch_consistency<16>(depth_r, H, W, dscale_r, sources, n_sources, px2, rel_thresh, count, zsum, (hipStream_t)stream);
  else
    launch_consistency<8>(depth_r, H, W, dscale_r, sources, n_sources, px2, rel_thresh, count, zsum, (hipStream_t)stream);
  return surf_check_launch();
}

extern "C" int surf_depth_consistency_finish(const float* depth_r, float dscale_r, const int32_t* count, const float* zsum, int64_t n,
                                             int min_consistent, int average, float* out_depth, uint8_t* keep, void* stream) {
  if (!depth_r || !count || !zsum || !out_depth || !keep || n < 1 || min_consistent < 0) return SURF_E_ARG;
  if (n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(depth_consistency_finish_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, depth_r, dscale_r, count, zsum,
                     n, min_consistent, average, out_depth, keep);
  return surf_check_launch();
}
