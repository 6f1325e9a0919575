// Depth-map fusion (surf_amd/fusion.py): truncated-signed-distance integration of the depth maps that `val` forwards render for
// many reference views into ONE world-frame lattice, the marching-cubes input made from it, and the colours of the extracted
// vertices.  The standard scene-mesh step of this family of methods (VolRecon, ReTR: TSDF fusion of the rendered depths).
//
//  * fuse_integrate_kernel: one thread per lattice point, z fastest, so a wavefront covers 64 consecutive z and reads / writes the
//    state (tsdf, weight, optionally three colour channels) coalesced.  The views of a launch (<= SURF_FUSE_MAX_VIEWS) are looped
//    INSIDE the kernel with the point's state in registers: the state is the large stream (8 to 40 B per point, 134 M points at
//    512^3) and is paid once per launch, not once per view; the depth maps (a few hundred KB each) are gathered through the caches.
//    The view table travels as a kernel argument (16 x 80 B).  Grid: y = the x index, x = 256-point blocks over that x's (y, z)
//    plane (a wavefront still covers 64 consecutive z, straddling rows where nz is no multiple of 64).
//    The library is compiled with -ffp-contract=off; every line below is one fp32 operation per operator, in exactly this order
//    (surf_amd/fusion.py mirrors it in numpy fp32 and the tests demand equality):
//        p  = (ax[i], ay[j], az[k]);  for each view, in the order given:
//        cx = ((P0*px + P1*py) + P2*pz) + P3      cy likewise with P4..P7      cz likewise with P8..P11
//        skip unless cz > 0
//        rx = rintf(cx / cz); ry = rintf(cy / cz)                      (IEEE division, ties to even)
//        skip unless 0 <= rx <= W-1 and 0 <= ry <= H-1                 (float compares: a NaN fails)
//        d  = depth[(int)ry * W + (int)rx] * dscale
//        skip unless d > 0 and d <= FLT_MAX                            (0, negative, NaN, inf = no measurement)
//        diff = d - cz;  skip unless diff >= -trunc                    (further than trunc behind the surface: unobserved)
//        t  = fminf(diff / trunc, 1.0f);  wn = weight + 1.0f
//        tsdf  = (tsdf  * weight + t)     / wn
//        color = (color * weight + img_c) / wn      per channel, when colours are fused
//        weight = wn
//  * fuse_lattice_kernel: u = -tsdf where weight > 0, NaN elsewhere (the sign of sdf_grid's u = -sdf: triangles are oriented like
//    the per-view meshes'; NaN = unobserved, what surf_mc_classify_observed masks).
//  * fuse_vertex_colors_kernel: one thread per vertex of the extracted mesh (lattice-index units, float64).  A vertex lies on one
//    lattice edge; with fl = floor(v) per axis (float64), clamped into the lattice:
//        axis = the first axis with v[axis] - fl[axis] != 0 (none: axis 0)
//        f    = (float)(v[axis] - fl[axis])                             (float64 subtraction, rounded to fp32 once)
//        lo   = (int)fl;  hi = lo with hi[axis] = min(lo[axis] + 1, n[axis] - 1)
//        c    = c_lo + (c_hi - c_lo) * f                                per channel, three fp32 operations
//        q    = c * 256;  q = fmin(fmax(q, 0), 255);  colour = (uint8)q (vertex_finish_kernel's quantisation)
// All three are bandwidth kernels: 256-thread blocks, no LDS.
#include <float.h>
#include <math.h>

#include "common.h"
#include "fuse_rule.h"       // the per-point rules (integration, vertex colour) and the view table, shared with fuse_sparse.hip

namespace {

template <bool COLOR>
__global__ __launch_bounds__(256) void fuse_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                             float* __restrict__ color, const float* __restrict__ ax,
                                                             const float* __restrict__ ay, const float* __restrict__ az, int ny,
                                                             int nz, FuseViews views, int n_views, float trunc) {
  // blockIdx.y = x index, blockIdx.x walks the (y, z) plane of that x: the point's indices cost one 32-bit division, not the
  // three 64-bit ones of a flat index (they were most of a one-view launch)
  const uint32_t plane = (uint32_t)ny * (uint32_t)nz, r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= plane) return;
  const uint32_t j = r / (uint32_t)nz, k = r - j * (uint32_t)nz;
  const int64_t i = (int64_t)blockIdx.y * plane + r;
  surf_fuse_integrate_point<COLOR>(tsdf, weight, color, i, ax[blockIdx.y], ay[j], az[k], views, n_views, trunc);
}

__global__ __launch_bounds__(256) void fuse_lattice_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, int64_t n,
                                                           float* __restrict__ u) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u[i] = weight[i] > 0.0f ? -tsdf[i] : __builtin_nanf("");
}

// the dense colour lattice (nx, ny, nz, 3) as surf_fuse_vertex_color reads it
struct DenseColors {
  const float* __restrict__ color;
  int ny, nz;
  __device__ __forceinline__ int64_t locate(int x, int y, int z) const { return (((int64_t)x * ny + y) * nz + z) * 3; }
  __device__ __forceinline__ float read(int64_t a, int c) const { return color[a + c]; }
};

__global__ __launch_bounds__(256) void fuse_vertex_colors_kernel(const double* __restrict__ vertices, int64_t n_vertices,
                                                                 const float* __restrict__ color, int nx, int ny, int nz,
                                                                 uint8_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_vertices) return;
  surf_fuse_vertex_color(vertices, t, nx, ny, nz, DenseColors{color, ny, nz}, out);
}

inline bool blocks256(int64_t n, unsigned* blocks) {
  const int64_t b = (n + 255) / 256;
  if (b >= ((int64_t)1 << 31)) return false;
  *blocks = (unsigned)b;
  return true;
}

}  // namespace

extern "C" int surf_fuse_integrate(float* tsdf, float* weight, float* color, const float* ax, const float* ay, const float* az,
                                   int nx, int ny, int nz, const float* h_P, const float* const* h_depths,
                                   const float* const* h_images, const int* h_hw, const float* h_dscale, int n_views, float trunc,
                                   void* stream) {
  if (!tsdf || !weight || !ax || !ay || !az || !h_P || !h_depths || !h_hw || !h_dscale) return SURF_E_ARG;
  if (nx < 1 || ny < 1 || nz < 1 || n_views < 1 || !(trunc > 0.0f) || !(trunc <= FLT_MAX)) return SURF_E_ARG;
  if (color && !h_images) return SURF_E_ARG;
  if (n_views > SURF_FUSE_MAX_VIEWS) return SURF_E_LIMIT;
  if (nx > 65535 || (int64_t)ny * nz >= ((int64_t)1 << 31)) return SURF_E_LIMIT;      // grid.y = nx; 32-bit index inside a plane
  unsigned blocks;
  if (!blocks256((int64_t)ny * nz, &blocks)) return SURF_E_LIMIT;
  FuseViews views;
  if (int e = surf_fill_fuse_views(views, color != nullptr, h_P, h_depths, h_images, h_hw, h_dscale, n_views)) return e;
  if (color)
    hipLaunchKernelGGL(fuse_integrate_kernel<true>, dim3(blocks, (unsigned)nx), dim3(256), 0, (hipStream_t)stream, tsdf, weight, color,
                       ax, ay, az, ny, nz, views, n_views, trunc);
  else
    hipLaunchKernelGGL(fuse_integrate_kernel<false>, dim3(blocks, (unsigned)nx), dim3(256), 0, (hipStream_t)stream, tsdf, weight, color,
                       ax, ay, az, ny, nz, views, n_views, trunc);
  return surf_check_launch();
}

extern "C" int surf_fuse_lattice(const float* tsdf, const float* weight, int64_t n, float* u, void* stream) {
  if (!tsdf || !weight || !u || n < 1) return SURF_E_ARG;
  unsigned blocks;
  if (!blocks256(n, &blocks)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(fuse_lattice_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tsdf, weight, n, u);
  return surf_check_launch();
}

extern "C" int surf_fuse_vertex_colors(const double* vertices, int64_t n_vertices, const float* color, int nx, int ny, int nz,
                                       uint8_t* out, void* stream) {
  if (!vertices || !color || !out || n_vertices < 1 || nx < 1 || ny < 1 || nz < 1) return SURF_E_ARG;
  if (n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  unsigned blocks;
  if (!blocks256(n_vertices, &blocks)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(fuse_vertex_colors_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, vertices, n_vertices, color, nx, ny,
                     nz, out);
  return surf_check_launch();
}
