// Brick-sparse depth-map fusion (surf_amd/fusion.py, FusionVolume(sparse=True)): the TSDF state of fuse.hip kept only in the 8^3-point
// bricks that can carry a triangle, in the brick layout of mesh_band.hip, so that a lattice of 2^31 points and more can be fused
// and meshed.  The dense lattice holds 8 to 20 B per point although only the points within trunc of a measured surface ever
// leave tsdf == 1; here the state is n_slots * 512 points, brick-major: slot * 512 + (lx << 6 | ly << 3 | lz).
//
// Geometry: the lattice (nx, ny, nz) is embedded in the cube of side n = max(nx, ny, nz), so that the band kernels of
// mesh_band.hip (keys, rank, emit) run on it unchanged: nbp = ceil(n / 8) bricks per axis in the table (nbp^3 int32, -1 = not
// allocated), brick ids (bx nbp + by) nbp + bz, dense keys (x n + y) n + z - the order of the dense index (x ny + y) nz + z.
//
// Why a subset of the bricks is enough.  Let N be the lattice points that some view updates with diff < trunc (t < 1).  Every
// other observed point ends with tsdf == 1.0f exactly ((1 w + 1) / (w + 1) is exact in fp32), i.e. u = -tsdf = -1.  At an
// isovalue in (-1, 1) an edge changes sign, or a cell carries a triangle, only when one of its corners has u > isovalue > -1:
// that corner is in N.  So the points the mesh reads are N dilated by one lattice step per axis (the 27-neighbourhood), and
// the "needed" bricks are those that hold such a point.  The bricks allocated here are a superset of them; EVERY view is
// integrated over EVERY point of an allocated brick with fuse_integrate_kernel's arithmetic, so the state there equals the dense
// state bit for bit, and a point of a brick that is not allocated reads NaN where the dense lattice holds -1 or NaN - neither
// gives a vertex or a triangle.  (That is why allocation has to see all views before the first one is integrated.)
//
//  * fuse_mark_bricks_kernel: one thread per depth pixel (x, y) of one view; marks (bytes set to 1) every brick that can hold a
//    needed point of that pixel.  A lattice point reads the pixel when rint(cx / cz) = x and rint(cy / cz) = y, i.e. cx / cz in
//    [x - 0.5, x + 0.5], cy / cz likewise, and is in N only with cz in [d - trunc, d + trunc], cz > 0: the truncated pyramid
//    { M^-1 (cz (sx, sy, 1) - t) } of P = [M | t], the convex hull of its eight corners.  L (12 floats) = M^-1 row-major and
//    c = -M^-1 t, formed on the host in float64 and rounded once (fusion.lift_transform: no fp32 subtraction of the large t).
//    fp32, one operation per operator, in exactly this order (fusion.mark_bricks_host mirrors it; equal brick lists):
//        d  = depth[y W + x] * dscale;  skip unless d > 0 and d <= FLT_MAX
//        z0 = fmaxf(d - trunc, 0.0f);  z1 = d + trunc             (cz = 0 is the camera centre: the pyramid's apex)
//        for sz in (z0, z1), sy in ((float)y - 0.5f, (float)y + 0.5f), sx in ((float)x - 0.5f, (float)x + 0.5f):
//            qx = sx * sz;  qy = sy * sz
//            X_k = ((L[3k] * qx + L[3k+1] * qy) + L[3k+2] * sz) + L[9+k]          k = 0, 1, 2
//        lo_k = fminf over the corners, hi_k = fmaxf over them; a corner coordinate that is NaN or inf makes axis k's range the
//        whole axis.  Otherwise i0_k = #{i : a_k[i] < lo_k}, i1_k = #{i : a_k[i] <= hi_k} - 1 (binary search: the axes are
//        strictly increasing), then i0_k = max(i0_k - 2, 0), i1_k = min(i1_k + 2, n_k - 1); skip the pixel when i0_k > i1_k on
//        some axis; mark the bricks i0_k >> 3 .. i1_k >> 3 of every axis.
//    The margin of 2 lattice steps: one is the dilation.  The other covers rounding: the integration kernel decides "reads this
//    pixel" and "within trunc" from cx / cz and d - cz in fp32, and the corners above are fp32 too; each is off by a few ulp of
//    the coordinates' magnitude, which is far below one lattice step on any lattice whose fp32 axis values are still distinct
//    enough to be strictly increasing with even spacing (a step of 2^-18 of the coordinate magnitude leaves 32 ulp per step).
//    A point of N that the exact pyramid misses by such an error is therefore within one index of the index box of the fp32
//    corners.  (The tests check the superset property against the dense host path on every scene they use.)
//  * fuse_integrate_bricks_kernel: one 256-thread workgroup per allocated brick, two points per thread (local points l and
//    l + 256: a wavefront reads 256 contiguous bytes per state array).  The views of a launch (<= SURF_FUSE_MAX_VIEWS) are looped
//    inside the kernel with the point's state in registers; the per-point sequence is fuse.hip's header comment, operation for
//    operation.  A point past an upper face of the lattice (x >= nx, ...) is never updated: its weight stays 0.
//  * band values: u = -tsdf where weight > 0, NaN elsewhere, is surf_fuse_lattice on the flat brick-major arrays.
//  * band_classify_observed_kernel: the flag byte of mc_classify_observed_kernel for every band point, values read through the
//    brick table (a missing brick reads NaN): an edge bit only where both end points are finite, a triangle count only where
//    the eight corners are.  surf_band_keys / _rank / surf_mc_count / surf_band_emit run unchanged on these flags.
//  * fuse_vertex_colors_bricks_kernel: fuse_vertex_colors_kernel's arithmetic (fuse.hip's header) with the two colour reads
//    going through the brick table (a vertex lies between two finite points, so both bricks are allocated; a missing one reads 0).
// Bandwidth kernels, 256-thread blocks, no LDS, plain vector stores only: marks are bytes set to 1 by any number of threads.
#include <float.h>
#include <math.h>

#define MC_TABLE_QUAL __constant__
#include "band.h"             // brick addressing, the observed-corner classification (shared with mesh_band / mcubes / ray_cast)
#include "common.h"
#include "fuse_rule.h"        // the per-point rules and the view table, shared with fuse.hip
#include "mc_tables.h"

namespace {

constexpr int MARK_MARGIN = 2;

struct Lattice {
  typedef int64_t id_t;  // the type brick ids are computed in (band.h)
  int nx, ny, nz;
  int nbp;  // bricks per axis of the table: ceil(max(nx, ny, nz) / 8)
};

struct Lift { float L[12]; };

// #{i : a[i] < v} (strict = true) or #{i : a[i] <= v} of a strictly increasing array
__device__ __forceinline__ int count_below(const float* __restrict__ a, int n, float v, bool strict) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float t = a[mid];
    if (strict ? t < v : t <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void fuse_mark_bricks_kernel(const float* __restrict__ depth, int H, int W, float dscale, Lift lift,
                                                               const float* __restrict__ ax, const float* __restrict__ ay,
                                                               const float* __restrict__ az, Lattice g, float trunc,
                                                               uint8_t* __restrict__ mark) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const float d = depth[i] * dscale;
  if (!(d > 0.0f && d <= FLT_MAX)) return;
  const float zs[2] = {fmaxf(d - trunc, 0.0f), d + trunc};
  const float ys[2] = {(float)y - 0.5f, (float)y + 0.5f}, xs[2] = {(float)x - 0.5f, (float)x + 0.5f};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool fin[3] = {true, true, true};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float sz = zs[c >> 2], sy = ys[(c >> 1) & 1], sx = xs[c & 1];
    const float qx = sx * sz, qy = sy * sz;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float X = ((lift.L[3 * k] * qx + lift.L[3 * k + 1] * qy) + lift.L[3 * k + 2] * sz) + lift.L[9 + k];
      fin[k] = fin[k] && surf_finite_f(X);
      lo[k] = fminf(lo[k], X);
      hi[k] = fmaxf(hi[k], X);
    }
  }
  const float* axes[3] = {ax, ay, az};
  const int n[3] = {g.nx, g.ny, g.nz};
  int b0[3], b1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int i0 = 0, i1 = n[k] - 1;
    if (fin[k]) {
      i0 = count_below(axes[k], n[k], lo[k], true);
      i1 = count_below(axes[k], n[k], hi[k], false) - 1;
    }
    i0 = max(i0 - MARK_MARGIN, 0);
    i1 = min(i1 + MARK_MARGIN, n[k] - 1);
    if (i0 > i1) return;
    b0[k] = i0 >> 3;
    b1[k] = i1 >> 3;                                   // <= (n_k - 1) >> 3 < nbp: every store below is inside the table
  }
  for (int bx = b0[0]; bx <= b1[0]; ++bx)
    for (int by = b0[1]; by <= b1[1]; ++by)
      for (int bz = b0[2]; bz <= b1[2]; ++bz) mark[band_brick_id(g.nbp, bx, by, bz)] = 1;
}

template <bool COLOR>
__global__ __launch_bounds__(256) void fuse_integrate_bricks_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                    float* __restrict__ color, const int32_t* __restrict__ bricks,
                                                                    const float* __restrict__ ax, const float* __restrict__ ay,
                                                                    const float* __restrict__ az, Lattice g, FuseViews views,
                                                                    int n_views, float trunc) {
  const int id = bricks[blockIdx.x];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int l = (int)threadIdx.x + 256 * h;
    int x, y, z;
    band_point_xyz(g.nbp, id, l, x, y, z);
    if (x >= g.nx || y >= g.ny || z >= g.nz) continue;                  // past an upper face: never updated
    surf_fuse_integrate_point<COLOR>(tsdf, weight, color, (int64_t)blockIdx.x * 512 + l, ax[x], ay[y], az[z], views, n_views, trunc);
  }
}

// ---- the observed-corner rule on a band ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void band_classify_observed_kernel(const float* __restrict__ vals, const int32_t* __restrict__ table,
                                                                     const int32_t* __restrict__ bricks, int64_t n_slots, Lattice g,
                                                                     double iso, uint8_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * 512) return;
  int x, y, z;
  band_point_xyz(g.nbp, bricks[t >> 9], (int)(t & 511), x, y, z);
  unsigned f = 0;
  const auto at = [=](int cx, int cy, int cz) { return band_val(g, table, vals, cx, cy, cz); };
  if (x < g.nx && y < g.ny && z < g.nz) f = surf_classify_observed(x, y, z, g.nx, g.ny, g.nz, vals[t], iso, at, MC_NTRI);
  flags[t] = (uint8_t)f;
}

// brick-major colours (n_slots * 512, 3) as surf_fuse_vertex_color reads them: a lattice point of a missing brick reads 0
struct BrickColors {
  const float* __restrict__ color;
  const int32_t* __restrict__ table;
  Lattice g;
  __device__ __forceinline__ int64_t locate(int x, int y, int z) const { return band_pos(g, table, x, y, z); }
  __device__ __forceinline__ float read(int64_t p, int c) const { return p < 0 ? 0.0f : color[p * 3 + c]; }
};

__global__ __launch_bounds__(256) void fuse_vertex_colors_bricks_kernel(const double* __restrict__ vertices, int64_t n_vertices,
                                                                        const float* __restrict__ color,
                                                                        const int32_t* __restrict__ table, Lattice g,
                                                                        uint8_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_vertices) return;
  surf_fuse_vertex_color(vertices, t, g.nx, g.ny, g.nz, BrickColors{color, table, g}, out);
}

// the lattice in its cube: 0 or a status
int lattice_of(int nx, int ny, int nz, Lattice& g) {
  if (nx < 1 || ny < 1 || nz < 1) return SURF_E_ARG;
  const int n = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  if (n < 2) return SURF_E_ARG;
  if (n > SURF_BAND_MAX_RES) return SURF_E_LIMIT;
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  g.nbp = (n + 7) / 8;
  if ((int64_t)g.nbp * g.nbp * g.nbp >= ((int64_t)1 << 31)) return SURF_E_LIMIT;       // int32 brick ids
  return 0;
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int surf_fuse_mark_bricks(const float* depth, int H, int W, float dscale, const float* h_lift, const float* ax,
                                     const float* ay, const float* az, int nx, int ny, int nz, float trunc, uint8_t* mark,
                                     void* stream) {
  if (!depth || !h_lift || !ax || !ay || !az || !mark || H < 1 || W < 1) return SURF_E_ARG;
  if (!(trunc > 0.0f) || !(trunc <= FLT_MAX)) return SURF_E_ARG;
  Lattice g;
  if (int e = lattice_of(nx, ny, nz, g)) return e;
  if ((int64_t)H * W >= ((int64_t)1 << 31) || H > (1 << 24) || W > (1 << 24)) return SURF_E_LIMIT;   // pixel indices are exact floats
  Lift lift;
  for (int e = 0; e < 12; ++e) lift.L[e] = h_lift[e];
  hipLaunchKernelGGL(fuse_mark_bricks_kernel, dim3(blocks256((int64_t)H * W)), dim3(256), 0, (hipStream_t)stream, depth, H, W, dscale,
                     lift, ax, ay, az, g, trunc, mark);
  return surf_check_launch();
}

extern "C" int surf_fuse_integrate_bricks(float* tsdf, float* weight, float* color, const int32_t* bricks, int64_t n_slots,
                                          const float* ax, const float* ay, const float* az, int nx, int ny, int nz,
                                          const float* h_P, const float* const* h_depths, const float* const* h_images,
                                          const int* h_hw, const float* h_dscale, int n_views, float trunc, void* stream) {
  if (!tsdf || !weight || !bricks || !ax || !ay || !az || !h_P || !h_depths || !h_hw || !h_dscale) return SURF_E_ARG;
  if (n_slots < 0 || n_views < 1 || !(trunc > 0.0f) || !(trunc <= FLT_MAX)) return SURF_E_ARG;
  if (color && !h_images) return SURF_E_ARG;
  if (n_views > SURF_FUSE_MAX_VIEWS) return SURF_E_LIMIT;
  Lattice g;
  if (int e = lattice_of(nx, ny, nz, g)) return e;
  if (n_slots * 512 >= ((int64_t)1 << 31)) return SURF_E_LIMIT;                          // int32 band positions
  FuseViews views;
  if (int e = surf_fill_fuse_views(views, color != nullptr, h_P, h_depths, h_images, h_hw, h_dscale, n_views)) return e;
  if (n_slots == 0) return 0;
  if (color)
    hipLaunchKernelGGL(fuse_integrate_bricks_kernel<true>, dim3((unsigned)n_slots), dim3(256), 0, (hipStream_t)stream, tsdf, weight,
                       color, bricks, ax, ay, az, g, views, n_views, trunc);
  else
    hipLaunchKernelGGL(fuse_integrate_bricks_kernel<false>, dim3((unsigned)n_slots), dim3(256), 0, (hipStream_t)stream, tsdf, weight,
                       color, bricks, ax, ay, az, g, views, n_views, trunc);
  return surf_check_launch();
}

extern "C" int surf_band_classify_observed(const float* vals, const int32_t* table, const int32_t* bricks, int64_t n_slots, int nx,
                                           int ny, int nz, double isovalue, uint8_t* flags, void* stream) {
  if (!vals || !table || !bricks || !flags || n_slots < 0) return SURF_E_ARG;
  Lattice g;
  if (int e = lattice_of(nx, ny, nz, g)) return e;
  if (n_slots * 512 >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (n_slots == 0) return 0;
  hipLaunchKernelGGL(band_classify_observed_kernel, dim3(blocks256(n_slots * 512)), dim3(256), 0, (hipStream_t)stream, vals, table,
                     bricks, n_slots, g, isovalue, flags);
  return surf_check_launch();
}

extern "C" int surf_fuse_vertex_colors_bricks(const double* vertices, int64_t n_vertices, const float* color, const int32_t* table,
                                              int nx, int ny, int nz, uint8_t* out, void* stream) {
  if (!vertices || !color || !table || !out || n_vertices < 1) return SURF_E_ARG;
  Lattice g;
  if (int e = lattice_of(nx, ny, nz, g)) return e;
  if (n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  hipLaunchKernelGGL(fuse_vertex_colors_bricks_kernel, dim3(blocks256(n_vertices)), dim3(256), 0, (hipStream_t)stream, vertices,
                     n_vertices, color, table, g, out);
  return surf_check_launch();
}
