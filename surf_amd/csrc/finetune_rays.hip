// Per-scene fine-tuning: the ray batch of one view made on the device (surf_amd/datasets/dtu_finetune.py after `.to(device)`;
// the reference builds it on the host and uploads it, the three full-size images included: datasets/dtu_finetune.py:262-345).
//
//  * finetune_rays_kernel: one thread per ray.  Pixel coordinates (px, py) arrive as fp32 (the validation lattice, built on the
//    host with the reference's own torch.linspace) or as int32 (the training draw; int -> fp32 is exact below 2^24).  The library
//    is compiled with -ffp-contract=off; every line below is one fp32 operation per operator, evaluated left to right as
//    parenthesised (Ki = the view's inverse(K)[:3,:3] row-major, computed on the host; c = the view's c2w[:3,:4] row-major):
//        dx = (Ki[0]*px + Ki[1]*py) + Ki[2]          dy, dz likewise with Ki[3..5], Ki[6..8]     (the homogeneous 1: x * 1 = x)
//        n  = sqrt((dx*dx + dy*dy) + dz*dz)          (IEEE fp32 square root)
//        dx = dx / n;  dy = dy / n;  dz = dz / n      (IEEE fp32 division)
//        rays_d[0] = (c[0]*dx + c[1]*dy) + c[2]*dz    rays_d[1], rays_d[2] likewise with c[4..6], c[8..10]
//        rays_o    = (c[3], c[7], c[11])
//        x = (long)px, y = (long)py                   (truncation towards zero, the reference's .long())
//        color = image[y][x][0..2], pseudo_depth = depth[y][x]      (copies; a pixel outside the image yields zeros)
//    tests/test_finetune_gpu.py mirrors exactly this sequence in numpy fp32.
//  * gather_pts_kernel: out[i] = pts[idx[i]] for rows of three fp32 (the 2048 pseudo surface points of a step; an index outside
//    [0, n_pts) yields zeros).
// Bandwidth-trivial (512 rays a step, 120 000 for a validation image): 64-thread blocks, one wavefront per 64 rays, no LDS.
// What it buys is what no longer crosses the bus every step, not its own speed.
#include <math.h>

#include "common.h"

namespace {

inline unsigned blocks64(int64_t n) { return (unsigned)((n + 63) / 64); }

template <typename Coord>
__global__ __launch_bounds__(64) void finetune_rays_kernel(const Coord* __restrict__ pxs, const Coord* __restrict__ pys, int64_t n,
                                                           const float* __restrict__ kinv, const float* __restrict__ c2w,
                                                           const float* __restrict__ image, const float* __restrict__ depth,
                                                           int h, int w, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                           float* __restrict__ color, float* __restrict__ pseudo_depth) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float px = (float)pxs[t], py = (float)pys[t];
  float dx = (kinv[0] * px + kinv[1] * py) + kinv[2];
  float dy = (kinv[3] * px + kinv[4] * py) + kinv[5];
  float dz = (kinv[6] * px + kinv[7] * py) + kinv[8];
  const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
  dx = dx / nrm;
  dy = dy / nrm;
  dz = dz / nrm;
  rays_d[t * 3 + 0] = (c2w[0] * dx + c2w[1] * dy) + c2w[2] * dz;
  rays_d[t * 3 + 1] = (c2w[4] * dx + c2w[5] * dy) + c2w[6] * dz;
  rays_d[t * 3 + 2] = (c2w[8] * dx + c2w[9] * dy) + c2w[10] * dz;
  rays_o[t * 3 + 0] = c2w[3];
  rays_o[t * 3 + 1] = c2w[7];
  rays_o[t * 3 + 2] = c2w[11];
  const int64_t x = (int64_t)px, y = (int64_t)py;
  const bool inside = x >= 0 && x < w && y >= 0 && y < h;
  const int64_t at = inside ? y * w + x : 0;
  color[t * 3 + 0] = inside ? image[at * 3 + 0] : 0.0f;
  color[t * 3 + 1] = inside ? image[at * 3 + 1] : 0.0f;
  color[t * 3 + 2] = inside ? image[at * 3 + 2] : 0.0f;
  if (pseudo_depth) pseudo_depth[t] = inside ? depth[at] : 0.0f;
}

__global__ __launch_bounds__(64) void gather_pts_kernel(const float* __restrict__ pts, int64_t n_pts, const int32_t* __restrict__ idx,
                                                        int64_t n, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t i = idx[t];
  const bool ok = i >= 0 && i < n_pts;
  const int64_t at = ok ? i : 0;
  out[t * 3 + 0] = ok ? pts[at * 3 + 0] : 0.0f;
  out[t * 3 + 1] = ok ? pts[at * 3 + 1] : 0.0f;
  out[t * 3 + 2] = ok ? pts[at * 3 + 2] : 0.0f;
}

}  // namespace

extern "C" int surf_finetune_rays(const void* px, const void* py, int coords_int32, int64_t n_rays, const float* kinv,
                                  const float* c2w, const float* image, const float* depth, int h, int w, float* rays_o,
                                  float* rays_d, float* color, float* pseudo_depth, void* stream) {
  if (!px || !py || !kinv || !c2w || !image || !rays_o || !rays_d || !color || n_rays <= 0 || h <= 0 || w <= 0) return SURF_E_ARG;
  if (pseudo_depth && !depth) return SURF_E_ARG;
  if (n_rays >= ((int64_t)1 << 31) || h > (1 << 20) || w > (1 << 20)) return SURF_E_LIMIT;      // int32 -> fp32 stays exact
  if (coords_int32)
    hipLaunchKernelGGL(finetune_rays_kernel<int32_t>, dim3(blocks64(n_rays)), dim3(64), 0, (hipStream_t)stream, (const int32_t*)px,
                       (const int32_t*)py, n_rays, kinv, c2w, image, depth, h, w, rays_o, rays_d, color, pseudo_depth);
  else
    hipLaunchKernelGGL(finetune_rays_kernel<float>, dim3(blocks64(n_rays)), dim3(64), 0, (hipStream_t)stream, (const float*)px,
                       (const float*)py, n_rays, kinv, c2w, image, depth, h, w, rays_o, rays_d, color, pseudo_depth);
  return surf_check_launch();
}

extern "C" int surf_finetune_gather_pts(const float* pts, int64_t n_pts, const int32_t* idx, int64_t n, float* out, void* stream) {
  if (!pts || !idx || !out || n_pts <= 0 || n <= 0) return SURF_E_ARG;
  if (n_pts >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(gather_pts_kernel, dim3(blocks64(n)), dim3(64), 0, (hipStream_t)stream, pts, n_pts, idx, n, out);
  return surf_check_launch();
}
