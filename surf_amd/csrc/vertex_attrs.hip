// Per-vertex mesh attributes (ImplicitSurface.vertex_attributes): the glue around the SDF gradient and blend kernels, which
// run unchanged over the vertex list of an extracted mesh.
//
//  * vertex_points_kernel: one thread per COORDINATE (3 n of them, so that consecutive lanes touch consecutive addresses on both
//    sides whatever the row stride).  pts[e] = (float)vertices[e]: float64 -> fp32 by round-to-nearest-even (v_cvt_f32_f64, what
//    torch.Tensor.float() does), fp32 copied.  The first n threads also write idx[t] = t, the identity index list the SDF and
//    blend entry points take (every vertex active, no occupancy mask).
//  * vertex_finish_kernel: one thread per vertex.  The library is compiled with -ffp-contract=off; every line below is one fp32
//    operation per operator, evaluated left to right as parenthesised (g = grad row, c = colour row, k = n_valid):
//        n  = sqrt((gx*gx + gy*gy) + gz*gz)          (IEEE fp32 square root)
//        ok = n > 0 and n <= FLT_MAX                 (false for a zero gradient, for nan / inf components and where the
//                                                     squares overflow: the row is then (0, 0, 0))
//        normal = ok ? (gx / n, gy / n, gz / n) : 0  (IEEE fp32 division)
//        q  = c * 256                                per channel
//        q  = fmin(fmax(q, 0), 255)                  (the non-nan operand wins: a nan colour quantises to 0)
//        colour = (uint8)q                           (truncation towards zero; q is in [0, 255])
//        colour = (128, 128, 128) where k == 0       (no source view sees the vertex)
//    tests/test_vertex_attrs_gpu.py mirrors exactly this sequence in numpy fp32.
// A thread reads its row as three dwords at stride 12 B: a wavefront's three loads together cover 768 contiguous bytes, every
// fetched line is used in full.  Bandwidth-trivial (about 60 B per vertex next to two MLP evaluations): 64-thread blocks, one
// wavefront per block, no LDS.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

inline unsigned blocks64(int64_t n) { return (unsigned)((n + 63) / 64); }

template <typename T>
__global__ __launch_bounds__(64) void vertex_points_kernel(const T* __restrict__ vertices, int64_t n, float* __restrict__ pts,
                                                           int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 3) return;
  pts[t] = (float)vertices[t];
  if (t < n) idx[t] = (int32_t)t;
}

__global__ __launch_bounds__(64) void vertex_finish_kernel(const float* __restrict__ grad, const float* __restrict__ color,
                                                           const uint8_t* __restrict__ n_valid, int64_t n,
                                                           float* __restrict__ normals, uint8_t* __restrict__ colors) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float gx = grad[t * 3 + 0], gy = grad[t * 3 + 1], gz = grad[t * 3 + 2];
  const float nrm = sqrtf((gx * gx + gy * gy) + gz * gz);
  const bool ok = nrm > 0.0f && nrm <= FLT_MAX;
  normals[t * 3 + 0] = ok ? gx / nrm : 0.0f;
  normals[t * 3 + 1] = ok ? gy / nrm : 0.0f;
  normals[t * 3 + 2] = ok ? gz / nrm : 0.0f;
  const bool seen = n_valid[t] != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float q = color[t * 3 + c] * 256.0f;
    q = fminf(fmaxf(q, 0.0f), 255.0f);
    colors[t * 3 + c] = seen ? (uint8_t)q : (uint8_t)128;
  }
}

}  // namespace

extern "C" int surf_vertex_points(const void* vertices, int is_f64, int64_t n, float* pts, int32_t* idx, void* stream) {
  if (!vertices || !pts || !idx || n <= 0) return SURF_E_ARG;
  if (n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;                  // int32 indices; 3 n / 64 blocks stay below 2^27
  if (is_f64)
    hipLaunchKernelGGL(vertex_points_kernel<double>, dim3(blocks64(n * 3)), dim3(64), 0, (hipStream_t)stream, (const double*)vertices,
                       n, pts, idx);
  else
    hipLaunchKernelGGL(vertex_points_kernel<float>, dim3(blocks64(n * 3)), dim3(64), 0, (hipStream_t)stream, (const float*)vertices,
                       n, pts, idx);
  return surf_check_launch();
}

extern "C" int surf_vertex_finish(const float* grad, const float* color, const uint8_t* n_valid, int64_t n, float* normals,
                                  uint8_t* colors, void* stream) {
  if (!grad || !color || !n_valid || !normals || !colors || n <= 0) return SURF_E_ARG;
  if (n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(vertex_finish_kernel, dim3(blocks64(n)), dim3(64), 0, (hipStream_t)stream, grad, color, n_valid, n, normals,
                     colors);
  return surf_check_launch();
}
