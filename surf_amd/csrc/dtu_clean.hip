// The DTU evaluation protocol's mesh cleaner on the device (surf_amd/evaluation/clean_dtu.py, backend="device"): the stages of
// the reference's evaluation/clean_mesh.py that the runner's cleaner (mesh_clean.hip) does not have, each equal to its host twin.
//
//  * dtu_dilate_ellipse_kernel: grey dilation (maximum) of uint8 masks with a row-symmetric footprint given as per-row
//    half-widths: row i (dy = i - k/2) covers columns [-half[i], +half[i]]; a negative half-width is an empty row.  Pixels
//    outside the image do not contribute (cv.dilate's default border for a maximum).  One thread per output pixel.
//  * dtu_points_in_masks_kernel: one thread per vertex, all views in one launch.  The library is compiled with
//    -ffp-contract=off; every line is one float64 operation per operator, evaluated left to right as parenthesised, with the
//    float32 projection entries widened first (P = the first three rows of K4 @ E, 12 floats per view, row-major):
//        X = ((P[0]*x + P[1]*y) + P[2]*z) + P[3]          Y, Z likewise with P[4..7], P[8..11]
//        qx = X / Z;  qy = Y / Z                                                              (IEEE float64 division)
//        the view does not count when Z == 0 or !(|qx| <= 2^30) or !(|qy| <= 2^30)          (NaN and inf fail the <=)
//        u = (int64)rint(qx) + 1;  v = (int64)rint(qy) + 1                                    (round half to even)
//        the view does not count unless 0 <= u <= w and 0 <= v <= h                           (w + 1, h + 1: ring, not in range)
//        counts when u == 0 || v == 0 (the ring of ones around the padded mask) or dilated[v - 1][u - 1] > 128
//    Z is not tested for sign (the reference's behaviour).  The guard comes before the double -> integer conversion.
//  * dtu_vertex_face_keep_kernel: vkeep[v] = count[v] > minimal_vis; fkeep[f] = the three vertices of f are kept (read from
//    the counts, not from vkeep: the two halves of the launch do not depend on one another).
// Compaction by vertex flag reuses surf_clean_compact_rows / surf_clean_compact_faces of mesh_clean.hip; the scans between are
// the caller's.  Offline tool, bandwidth-trivial: 256-thread blocks, no LDS.
#include <math.h>

#include "common.h"

namespace {

constexpr int kMaxFootprintRows = 64;

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void dtu_dilate_ellipse_kernel(const uint8_t* __restrict__ in, int nv, int h, int w,
                                                                 const int32_t* __restrict__ half, int k,
                                                                 uint8_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nv * h * w) return;
  const int x = (int)(t % w), y = (int)((t / w) % h);
  const uint8_t* img = in + (t / ((int64_t)h * w)) * ((int64_t)h * w);
  const int r = k / 2;
  uint8_t best = 0;
  for (int i = 0; i < k; ++i) {
    const int yy = y + i - r;
    if (yy < 0 || yy >= h) continue;
    const int dx = min(half[i], w);                      // a half-width beyond the image adds nothing
    const int x0 = max(x - dx, 0), x1 = min(x + dx, w - 1);
    const uint8_t* row = img + (int64_t)yy * w;
    for (int xx = x0; xx <= x1; ++xx) best = max(best, row[xx]);
  }
  out[t] = best;
}

__global__ __launch_bounds__(256) void dtu_points_in_masks_kernel(const double* __restrict__ V, int64_t n,
                                                                  const uint8_t* __restrict__ masks, const float* __restrict__ P,
                                                                  int nv, int h, int w, int32_t* __restrict__ count) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const double x = V[t * 3 + 0], y = V[t * 3 + 1], z = V[t * 3 + 2];
  const double lim = 1073741824.0;                       // 2^30
  int32_t cnt = 0;
  for (int i = 0; i < nv; ++i) {
    const float* p = P + i * 12;
    const uint8_t* m = masks + (int64_t)i * h * w;
    const double X = (((double)p[0] * x + (double)p[1] * y) + (double)p[2] * z) + (double)p[3];
    const double Y = (((double)p[4] * x + (double)p[5] * y) + (double)p[6] * z) + (double)p[7];
    const double Z = (((double)p[8] * x + (double)p[9] * y) + (double)p[10] * z) + (double)p[11];
    const double qx = X / Z, qy = Y / Z;
    if (Z == 0.0 || !(fabs(qx) <= lim) || !(fabs(qy) <= lim)) continue;
    const int64_t u = (int64_t)rint(qx) + 1, v = (int64_t)rint(qy) + 1;
    if (u < 0 || u > w || v < 0 || v > h) continue;
    if (u == 0 || v == 0 || m[(v - 1) * w + (u - 1)] > 128) ++cnt;
  }
  count[t] = cnt;
}

__global__ __launch_bounds__(256) void dtu_vertex_face_keep_kernel(const int32_t* __restrict__ count, int64_t nvert,
                                                                   const int32_t* __restrict__ faces, int64_t nf, int minimal_vis,
                                                                   uint8_t* __restrict__ vkeep, uint8_t* __restrict__ fkeep) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nvert) vkeep[t] = count[t] > minimal_vis;
  if (t < nf) {
    bool keep = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t v = faces[t * 3 + c];
      keep = keep && v >= 0 && v < nvert && count[v] > minimal_vis;
    }
    fkeep[t] = keep;
  }
}

}  // namespace

extern "C" int surf_dtu_clean_dilate(const uint8_t* masks, int n_views, int h, int w, const int32_t* half_widths, int k,
                                     uint8_t* out, void* stream) {
  if (!masks || !out || !half_widths || n_views <= 0 || h <= 0 || w <= 0 || k <= 0 || k % 2 == 0) return SURF_E_ARG;
  if (k > kMaxFootprintRows || (int64_t)n_views * h * w > ((int64_t)1 << 40)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(dtu_dilate_ellipse_kernel, dim3(blocks((int64_t)n_views * h * w)), dim3(256), 0, (hipStream_t)stream, masks,
                     n_views, h, w, half_widths, k, out);
  return surf_check_launch();
}

extern "C" int surf_dtu_clean_points_in_masks(const double* vertices, int64_t n_vertices, const uint8_t* dilated, const float* proj,
                                              int n_views, int h, int w, int32_t* count, void* stream) {
  if (n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!vertices || !dilated || !proj || !count || n_vertices <= 0 || n_views <= 0 || h <= 0 || w <= 0) return SURF_E_ARG;
  if (h > (1 << 20) || w > (1 << 20)) return SURF_E_LIMIT;                                     // well inside the 2^30 guard
  hipLaunchKernelGGL(dtu_points_in_masks_kernel, dim3(blocks(n_vertices)), dim3(256), 0, (hipStream_t)stream, vertices, n_vertices,
                     dilated, proj, n_views, h, w, count);
  return surf_check_launch();
}

extern "C" int surf_dtu_clean_keep(const int32_t* count, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int minimal_vis,
                                   uint8_t* vertex_keep, uint8_t* face_keep, void* stream) {
  if (n_faces >= ((int64_t)1 << 31) || n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!count || !vertex_keep || n_vertices <= 0 || n_faces < 0 || (n_faces > 0 && (!faces || !face_keep))) return SURF_E_ARG;
  hipLaunchKernelGGL(dtu_vertex_face_keep_kernel, dim3(blocks(n_vertices > n_faces ? n_vertices : n_faces)), dim3(256), 0,
                     (hipStream_t)stream, count, n_vertices, faces, n_faces, minimal_vis, vertex_keep, face_keep);
  return surf_check_launch();
}
