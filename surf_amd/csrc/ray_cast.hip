// Ray casting of the fused TSDF (surf_amd/fusion.py, FusionVolume.ray_cast): depth, normal and colour of the fused model from any
// camera, without a mesh.  The dense state of fuse.hip and the brick-major state of fuse_sparse.hip share ONE traversal, templated
// on the corner fetch (dense: 64-bit index; bricks: through the brick table, a corner in an unallocated brick is unobserved).
//
// One ray per lane; a wavefront takes an 8 x 8 pixel tile (lane = ly * 8 + lx) and a 256-thread block a 16 x 16 tile, so the rays of
// a wavefront walk neighbouring cells and their corner gathers fall into few cache lines (z is contiguous in both layouts).  The
// walk is lane-divergent by nature (every ray has its own cell sequence); the loop body is kept branch-poor and the lanes of a tile
// leave the loop at similar counts.  No LDS; registers: eight corner values and eight positions per lane.
//
// Units: lattice-index units, lattice point (i, j, k) at (i, j, k); cell (i, j, k) has the corners i..i+1, j..j+1, k..k+1,
// 0 <= i <= nx - 2 (likewise j, k).  The lattice is uniform: world = lo + voxel * index.
// Camera: the 12 floats of fusion.ray_lift(P, lo, voxel), formed on the host in float64 and rounded once: L (9, row-major)
// = M^-1 / voxel and c (3) = (-M^-1 t - lo) / voxel for P = [M | t].  The ray of pixel (x, y) is p(z) = c + z r with r = L (x, y, 1);
// the parameter z IS the z-depth in world units, so the output is a DepthView depth with dscale = 1.
//
// The library is compiled with -ffp-contract=off; every line below is one fp32 operation per operator, in exactly this order
// (fusion.ray_cast_host mirrors it in numpy fp32 and the tests demand equal arrays).  lerp(a, b, u) = (1.0f - u) * a + u * b.
//     xf = (float)x; yf = (float)y;  r_a = (L[3a] * xf + L[3a+1] * yf) + L[3a+2]                               a = 0, 1, 2
//   clip:  m_a = (float)(n_a - 1).  r_a != 0: t0 = (0.0f - c_a) / r_a; t1 = (m_a - c_a) / r_a; near_a = t0 < t1 ? t0 : t1, far_a the
//     other.  r_a == 0: no bound from axis a when 0 <= c_a <= m_a, else the ray misses.  te = z_min; per axis in order: if
//     near_a > te then te = near_a;  tx = +inf; if far_a < tx then tx = far_a.  The ray misses unless te < tx.
//   first cell:  p_a = c_a + te * r_a;  i_a = (int)fminf(fmaxf(floorf(p_a), 0.0f), m_a - 1.0f);  entry local coordinates
//     u_a = clamp(p_a - (float)i_a, 0, 1) on all three axes.
//   walk, at most nx + ny + nz cells:
//     crossing of axis a: plane_a = r_a > 0 ? i_a + 1 : i_a;  t_a = ((float)plane_a - c_a) / r_a, +inf when r_a == 0 - always from
//       the integer plane index, never accumulated, so a crossing parameter does not depend on the cells walked before.
//     exit: axis = 0, to = t_0; if t_1 < to then axis = 1, to = t_1; if t_2 < to then axis = 2, to = t_2 (ties: x, then y, then z).
//       The walk ends when to is not finite.
//     exit point: on the crossed axis the local coordinate is exactly 1.0f (r_a > 0) or 0.0f; on the other two
//       p_b = c_b + to * r_b;  w_b = fminf(fmaxf(p_b - (float)i_b, 0.0f), 1.0f).
//     the cell COUNTS when all eight corners have weight > 0.  Then v_c = tsdf_c - level per corner (level = -isovalue) and
//       f(u) = lerp over z of (lerp over y of (lerp over x)):  c00 = lerp(v000, v100, ux) c10 = lerp(v010, v110, ux)
//       c01 = lerp(v001, v101, ux) c11 = lerp(v011, v111, ux);  c0 = lerp(c00, c10, uy) c1 = lerp(c01, c11, uy);  f = lerp(c0, c1, uz)
//       f_in = f(entry), f_out = f(exit).  HIT when f_in > 0 and f_out <= 0 (front to inside only).
//     step: i_axis += r_axis > 0 ? 1 : -1; the walk ends when it leaves 0 .. n_axis - 2.  The next cell's entry point is the exit
//       point with the crossed coordinate flipped (1 <-> 0): the other two come from the SAME p_b, and lerp with u = 0 or 1 returns
//       a corner exactly, so the value on a shared face is bit-identical from either cell and a sign change belongs to one cell.
//   refinement in the hit cell - RAY_REFINE_EVALS = 3 evaluations, no data-dependent count: bracket (ta, fa) = (t_in, f_in),
//     (tb, fb) = (to, f_out); three times:  s = fa / (fa - fb);  t = ta + (tb - ta) * s;  g = f(u(t)) with
//     u_a(t) = fminf(fmaxf((c_a + t * r_a) - (float)i_a, 0.0f), 1.0f) on all three axes;  g > 0 ? (ta, fa) = (t, g) : (tb, fb) = (t, g).
//     Then the root z = ta + (tb - ta) * (fa / (fa - fb)) (one more linear interpolation), u = u(z).
//   outputs:  depth = z.  normal = the gradient of the cell's trilinear interpolant at u, normalised:
//       gx = lerp(lerp(v100 - v000, v110 - v010, uy), lerp(v101 - v001, v111 - v011, uy), uz)
//       gy = lerp(lerp(v010 - v000, v110 - v100, ux), lerp(v011 - v001, v111 - v101, ux), uz)
//       gz = lerp(lerp(v001 - v000, v101 - v100, ux), lerp(v011 - v010, v111 - v110, ux), uy)
//       n = sqrtf((gx * gx + gy * gy) + gz * gz);  normal = (gx / n, gy / n, gz / n), zero when n == 0.  tsdf grows towards the camera
//       side of a surface, so the normal points into free space; the lattice axes are the world axes (uniform voxel): world frame.
//     color_ch = f's lerp order on the eight corner colours of the channel, at u.
//     No hit: depth 0 (DepthView's "no measurement"), normal and colour 0.  Every pixel is written.
//
// Dense and brick-sparse state return equal arrays: a cell with a corner at or below level has a corner some view updated with
// diff < trunc, whose 27-neighbourhood is allocated (fuse_sparse.hip's header), so every cell that can hit is fully allocated with
// the dense state bit for bit; a cell that is not fully allocated counts in neither path or holds tsdf == 1 > level at all eight
// corners in the dense one (f_out > 0: no hit, and nothing is carried from cell to cell but the crossing itself).  The brick fetch
// skips only work, never cells: a cell whose own brick is not allocated cannot count (its corner (i, j, k) is in that brick) and
// costs no state read, and the table entry of the brick a ray is in is read once, not once per cell.
#include <float.h>
#include <math.h>

#include "band.h"              // brick ids and local indices of the brick-major state
#include "common.h"

namespace {

constexpr int RAY_REFINE_EVALS = 3;

struct RayCam { float L[9]; float c[3]; };
struct RayDims { int nx, ny, nz; };

// positions of the cell's eight corners, corner index dx * 4 + dy * 2 + dz; false: some corner is not allocated
struct DenseFetch {
  int64_t sy, sx;                                       // strides of y and x: nz, ny * nz
  __device__ __forceinline__ bool corners(int i, int j, int k, int64_t pos[8], int64_t&, int32_t&) const {
    const int64_t base = (int64_t)i * sx + (int64_t)j * sy + k;
#pragma unroll
    for (int c = 0; c < 8; ++c) pos[c] = base + (c >> 2) * sx + ((c >> 1) & 1) * sy + (c & 1);
    return true;
  }
};

struct BrickFetch {
  const int32_t* __restrict__ table;
  int nbp;
  __device__ __forceinline__ int32_t slot(int bx, int by, int bz) const { return table[band_brick_id(nbp, bx, by, bz)]; }
  // last / last_slot: the brick of the previous cell and its table entry, kept by the caller - a ray stays in a brick for several
  // cells, and while that brick is missing its cells cost no read at all
  __device__ __forceinline__ bool corners(int i, int j, int k, int64_t pos[8], int64_t& last, int32_t& last_slot) const {
    const int bx = i >> 3, by = j >> 3, bz = k >> 3;
    const int64_t id = band_brick_id(nbp, bx, by, bz);
    if (id != last) { last = id; last_slot = table[id]; }
    const int32_t s0 = last_slot;
    if (s0 < 0) return false;                           // the cell's own brick is missing: the cell cannot count
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int x = i + (c >> 2), y = j + ((c >> 1) & 1), z = k + (c & 1);
      const int cx = x >> 3, cy = y >> 3, cz = z >> 3;
      const int32_t s = (cx == bx && cy == by && cz == bz) ? s0 : slot(cx, cy, cz);     // x <= n - 1: inside the table
      all = all && s >= 0;
      pos[c] = (int64_t)(s < 0 ? 0 : s) * 512 + band_local(x, y, z);
    }
    return all;
  }
};

__device__ __forceinline__ float lerp1(float a, float b, float u) { return (1.0f - u) * a + u * b; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float trilerp(const float v[8], float ux, float uy, float uz) {
  const float c00 = lerp1(v[0], v[4], ux), c10 = lerp1(v[2], v[6], ux), c01 = lerp1(v[1], v[5], ux), c11 = lerp1(v[3], v[7], ux);
  const float c0 = lerp1(c00, c10, uy), c1 = lerp1(c01, c11, uy);
  return lerp1(c0, c1, uz);
}

template <class Fetch, bool COLOR>
__global__ __launch_bounds__(256) void ray_cast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                       const float* __restrict__ color, Fetch fetch, RayDims g, RayCam cam, int H, int W,
                                                       int tiles_x, float z_min, float level, float* __restrict__ depth,
                                                       float* __restrict__ normal, float* __restrict__ out_color) {
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  const int x = tx * 16 + (wave & 1) * 8 + (lane & 7), y = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (x >= W || y >= H) return;
  const int64_t pix = (int64_t)y * W + x;
  const float xf = (float)x, yf = (float)y;
  const int n[3] = {g.nx, g.ny, g.nz};
  float r[3], c[3], m[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r[a] = (cam.L[3 * a] * xf + cam.L[3 * a + 1] * yf) + cam.L[3 * a + 2];
    c[a] = cam.c[a];
    m[a] = (float)(n[a] - 1);
  }
  float out_d = 0.0f, out_n[3] = {0.0f, 0.0f, 0.0f}, out_c[3] = {0.0f, 0.0f, 0.0f};
  // ---- clip to the box of cells and to z > z_min ----
  float te = z_min, tx_ = INFINITY;
  bool live = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (r[a] != 0.0f) {
      const float t0 = (0.0f - c[a]) / r[a], t1 = (m[a] - c[a]) / r[a];
      const float nr = t0 < t1 ? t0 : t1, fr = t0 < t1 ? t1 : t0;
      if (nr > te) te = nr;
      if (fr < tx_) tx_ = fr;
    } else if (!(c[a] >= 0.0f && c[a] <= m[a])) {
      live = false;
    }
  }
  live = live && te < tx_;
  if (live) {
    int ic[3];
    float u[3];                                         // entry point, cell-local
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float p = c[a] + te * r[a];
      const float fl = fminf(fmaxf(floorf(p), 0.0f), m[a] - 1.0f);
      ic[a] = (int)fl;
      u[a] = clamp01(p - fl);
    }
    float t_in = te;
    int64_t last_brick = -1;
    int32_t last_slot = -1;
    const int max_cells = g.nx + g.ny + g.nz;
    for (int step = 0; step < max_cells; ++step) {
      // ---- the crossing that ends this cell, from the integer plane indices ----
      float tc[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) tc[a] = r[a] != 0.0f ? ((float)(r[a] > 0.0f ? ic[a] + 1 : ic[a]) - c[a]) / r[a] : INFINITY;
      int axis = 0;
      float to = tc[0];
      if (tc[1] < to) { axis = 1; to = tc[1]; }
      if (tc[2] < to) { axis = 2; to = tc[2]; }
      if (!(fabsf(to) <= FLT_MAX)) break;
      float w[3];                                       // exit point, cell-local
      int dir = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (a == axis) {
          dir = r[a] > 0.0f ? 1 : -1;
          w[a] = r[a] > 0.0f ? 1.0f : 0.0f;
        } else {
          const float p = c[a] + to * r[a];
          w[a] = clamp01(p - (float)ic[a]);
        }
      }
      // ---- does the cell count?  all eight corners observed ----
      int64_t pos[8];
      bool counted = fetch.corners(ic[0], ic[1], ic[2], pos, last_brick, last_slot);
      if (counted) {                                    // eight independent reads in flight (every pos is a valid position)
        bool obs = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) obs &= weight[pos[k]] > 0.0f;
        counted = obs;
      }
      if (counted) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = tsdf[pos[k]] - level;
        const float f_in = trilerp(v, u[0], u[1], u[2]), f_out = trilerp(v, w[0], w[1], w[2]);
        if (f_in > 0.0f && f_out <= 0.0f) {
          float ta = t_in, fa = f_in, tb = to, fb = f_out;
          const float fi[3] = {(float)ic[0], (float)ic[1], (float)ic[2]};
          for (int e = 0; e < RAY_REFINE_EVALS; ++e) {
            const float s = fa / (fa - fb);
            const float t = ta + (tb - ta) * s;
            const float gv = trilerp(v, clamp01((c[0] + t * r[0]) - fi[0]), clamp01((c[1] + t * r[1]) - fi[1]),
                                     clamp01((c[2] + t * r[2]) - fi[2]));
            if (gv > 0.0f) { ta = t; fa = gv; } else { tb = t; fb = gv; }
          }
          const float z = ta + (tb - ta) * (fa / (fa - fb));
          const float ux = clamp01((c[0] + z * r[0]) - fi[0]), uy = clamp01((c[1] + z * r[1]) - fi[1]),
                      uz = clamp01((c[2] + z * r[2]) - fi[2]);
          out_d = z;
          const float gx = lerp1(lerp1(v[4] - v[0], v[6] - v[2], uy), lerp1(v[5] - v[1], v[7] - v[3], uy), uz);
          const float gy = lerp1(lerp1(v[2] - v[0], v[6] - v[4], ux), lerp1(v[3] - v[1], v[7] - v[5], ux), uz);
          const float gz = lerp1(lerp1(v[1] - v[0], v[5] - v[4], ux), lerp1(v[3] - v[2], v[7] - v[6], ux), uy);
          const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
          if (len > 0.0f) { out_n[0] = gx / len; out_n[1] = gy / len; out_n[2] = gz / len; }
          if (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              float cv[8];
#pragma unroll
              for (int k = 0; k < 8; ++k) cv[k] = color[pos[k] * 3 + ch];
              out_c[ch] = trilerp(cv, ux, uy, uz);
            }
          }
          break;
        }
      }
      // ---- step through the crossed face ----
      bool inside = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (a == axis) {
          ic[a] += dir;
          inside = ic[a] >= 0 && ic[a] <= n[a] - 2;
          u[a] = 1.0f - w[a];                           // exactly 0 or 1
        } else {
          u[a] = w[a];
        }
      }
      if (!inside) break;
      t_in = to;
    }
  }
  depth[pix] = out_d;
  if (normal) { normal[pix * 3 + 0] = out_n[0]; normal[pix * 3 + 1] = out_n[1]; normal[pix * 3 + 2] = out_n[2]; }
  if (COLOR) { out_color[pix * 3 + 0] = out_c[0]; out_color[pix * 3 + 1] = out_c[1]; out_color[pix * 3 + 2] = out_c[2]; }
}

// 0, or the status of the arguments both entry points share; *launch = false when there is nothing to do
int check_common(const void* tsdf, const void* weight, const void* color, int nx, int ny, int nz, const float* h_lift, int H, int W,
                 float z_min, float level, const void* depth, const void* out_color, bool* launch) {
  *launch = false;
  if (!tsdf || !weight || !h_lift || !depth) return SURF_E_ARG;
  if (nx < 1 || ny < 1 || nz < 1 || H < 0 || W < 0) return SURF_E_ARG;
  if (!(z_min >= 0.0f) || !(z_min <= FLT_MAX) || !(level > -1.0f) || !(level < 1.0f)) return SURF_E_ARG;
  if ((color != nullptr) != (out_color != nullptr)) return SURF_E_ARG;
  // index planes and pixel indices are exact floats
  if (nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24) || H > (1 << 24) || W > (1 << 24)) return SURF_E_LIMIT;
  if ((int64_t)H * W >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  *launch = (int64_t)H * W > 0;
  return 0;
}

template <class Fetch>
int launch(const float* tsdf, const float* weight, const float* color, const Fetch& fetch, int nx, int ny, int nz, const float* h_lift,
           int H, int W, float z_min, float level, float* depth, float* normal, float* out_color, void* stream) {
  RayCam cam;
  for (int e = 0; e < 9; ++e) cam.L[e] = h_lift[e];
  for (int e = 0; e < 3; ++e) cam.c[e] = h_lift[9 + e];
  const RayDims g{nx, ny, nz};
  const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;           // tiles_x * tiles_y <= H W < 2^31 (+ edge tiles: checked)
  if ((int64_t)tiles_x * tiles_y >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  const dim3 grid((unsigned)(tiles_x * tiles_y)), block(256);
  if (color)
    hipLaunchKernelGGL((ray_cast_kernel<Fetch, true>), grid, block, 0, (hipStream_t)stream, tsdf, weight, color, fetch, g, cam, H, W,
                       tiles_x, z_min, level, depth, normal, out_color);
  else
    hipLaunchKernelGGL((ray_cast_kernel<Fetch, false>), grid, block, 0, (hipStream_t)stream, tsdf, weight, color, fetch, g, cam, H, W,
                       tiles_x, z_min, level, depth, normal, out_color);
  return surf_check_launch();
}

}  // namespace

extern "C" int surf_fuse_ray_cast(const float* tsdf, const float* weight, const float* color, int nx, int ny, int nz,
                                  const float* h_lift, int H, int W, float z_min, float level, float* depth, float* normal,
                                  float* out_color, void* stream) {
  bool go;
  if (int e = check_common(tsdf, weight, color, nx, ny, nz, h_lift, H, W, z_min, level, depth, out_color, &go)) return e;
  if (nx > 65535 || (int64_t)ny * nz >= ((int64_t)1 << 31)) return SURF_E_LIMIT;          // surf_fuse_integrate's limits
  if (!go) return 0;
  const DenseFetch fetch{(int64_t)nz, (int64_t)ny * nz};
  return launch(tsdf, weight, color, fetch, nx, ny, nz, h_lift, H, W, z_min, level, depth, normal, out_color, stream);
}

extern "C" int surf_fuse_ray_cast_bricks(const float* tsdf, const float* weight, const float* color, const int32_t* table,
                                         int64_t n_slots, int nx, int ny, int nz, const float* h_lift, int H, int W, float z_min,
                                         float level, float* depth, float* normal, float* out_color, void* stream) {
  bool go;
  if (!table || n_slots < 0) return SURF_E_ARG;
  if (int e = check_common(tsdf, weight, color, nx, ny, nz, h_lift, H, W, z_min, level, depth, out_color, &go)) return e;
  const int res = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  if (res < 2) return SURF_E_ARG;
  if (res > SURF_BAND_MAX_RES) return SURF_E_LIMIT;                                       // surf_fuse_integrate_bricks' limits
  if (n_slots * 512 >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!go) return 0;
  const BrickFetch fetch{table, (res + 7) / 8};
  return launch(tsdf, weight, color, fetch, nx, ny, nz, h_lift, H, W, z_min, level, depth, normal, out_color, stream);
}
