// K13b: narrow-band iso-surface extraction (extract_geometry with render.mesh_extraction = band).
//
// The dense path (mcubes.hip) classifies every point of the resolution^3 lattice, and sdf_grid evaluates the SDF at all of
// them.  Here the lattice is cut into bricks of 8^3 cells and only bricks near the surface are evaluated; the mesh that comes
// out is the dense mesh, array for array, as long as every connected component of it has one brick that passes the screen.
//
// Geometry (resolution n per axis, lattice points 0 .. n-1): brick b owns the points 8b .. 8b+7 on each axis and the cells
// whose origins those are.  nbp = ceil(n / 8) bricks per axis cover the points (the brick table is nbp^3 int32, -1 = not
// evaluated); nbc = ceil((n - 1) / 8) of them hold cells (when n = 8k + 1 the last layer holds only the points n - 1, which
// the cells of the layer below read).  Brick ids are linear, (bx nbp + by) nbp + bz.  A "cell brick" (is_cell[id] = 1) is one
// whose cells are meshed; the others in the table are halo: their values are read by the cells of a cell brick on their -x /
// -y / -z side.  Band values are brick-major: vals[slot * 512 + (lx << 6 | ly << 3 | lz)].
//
//   screen   : coarse lattice (indices 0, 8, 16, .. and n-1, exact lattice values) -> mark the cell bricks whose 8 corners
//              change sign (u <= iso) or whose min |u - iso| <= margin * (brick diagonal) / 2
//   promote  : marked bricks that are not cell bricks yet become cell bricks; they and their 7 forward neighbours that are
//              not in the table are marked "need" (surf_compact of the two mark arrays gives the new lists)
//   assign   : new table slots for the "need" list (the SDF is then evaluated there: surf_sdf_bricks_*, or surf_band_points
//              + the fp32 kernel)
//   grow     : every sign-changing edge of a cell of a new cell brick marks the bricks of all (up to 4) cells incident to it
//   classify : the flag byte of mc_classify_kernel for every band point: edge bits only for edges of a cell of a cell brick,
//              triangle counts only for cells of cell bricks
//   keys / rank : ascending int64 lattice keys of the flagged points (the host sorts them) -> their band positions
//   (surf_mc_count of the flags at those positions gives the vertex / triangle offsets in dense order)
//   emit     : vertices and triangles as mc_vertex_kernel / mc_triangle_kernel, values / flags / first vertex ids found
//              through the brick table
//
// All plain vector stores: marks are bytes set to 1 by any number of threads (the same value), everything else has one writer.
#include <math.h>

#define MC_TABLE_QUAL __constant__
#include "band.h"              // brick ids, local indices, band_pos / band_val (shared with fuse_sparse.hip and ray_cast.hip)
#include "common.h"
#include "mc_tables.h"

namespace {

constexpr int BAND_BLOCK = 1024;  // active entries per workgroup in emit (= MC_BLOCK of mcubes.hip: surf_mc_count's layout)

struct BandDims {
  typedef int id_t;  // brick ids are computed in int (band.h): n <= SURF_BAND_MAX_RES keeps nbp^3 below 2^31
  int n;    // lattice points per axis
  int nbp;  // bricks per axis in the table
  int nbc;  // bricks per axis that hold cells
};

__device__ __forceinline__ bool inside(float v, double iso) { return (double)v <= iso; }

// corners of a cell in table order, the owner corner / axis of the 12 cell edges and their far corner (mcubes.hip's layout)
__constant__ int8_t kCx[8] = {0, 1, 1, 0, 0, 1, 1, 0}, kCy[8] = {0, 0, 1, 1, 0, 0, 1, 1}, kCz[8] = {0, 0, 0, 0, 1, 1, 1, 1};
__constant__ int8_t kEo[12] = {0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3}, kEa[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};
__constant__ int8_t kEe[12] = {1, 2, 2, 3, 5, 6, 6, 7, 4, 5, 6, 7};

// ---- screen ---------------------------------------------------------------------------------------------------------
// uc: (nbc+1)^3 coarse lattice (z fastest) at the lattice indices min(8k, n-1); cax/cay/caz its axis values
__global__ __launch_bounds__(256) void band_screen_kernel(const float* __restrict__ uc, const float* __restrict__ cax,
                                                          const float* __restrict__ cay, const float* __restrict__ caz, BandDims d,
                                                          double iso, double margin, uint8_t* __restrict__ mark) {
  const int64_t nc = (int64_t)d.nbc * d.nbc * d.nbc;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  const int bz = (int)(i % d.nbc), by = (int)((i / d.nbc) % d.nbc), bx = (int)(i / ((int64_t)d.nbc * d.nbc));
  const int m = d.nbc + 1;
  bool any_in = false, any_out = false;
  double amin = INFINITY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float v = uc[((int64_t)(bx + kCx[k]) * m + (by + kCy[k])) * m + (bz + kCz[k])];
    const bool in = inside(v, iso);
    any_in |= in;
    any_out |= !in;
    amin = fmin(amin, fabs((double)v - iso));
  }
  const double ex = (double)cax[bx + 1] - cax[bx], ey = (double)cay[by + 1] - cay[by], ez = (double)caz[bz + 1] - caz[bz];
  const double half_diag = 0.5 * sqrt(ex * ex + ey * ey + ez * ez);
  if ((any_in && any_out) || amin <= margin * half_diag) mark[band_brick_id(d.nbp, bx, by, bz)] = 1;
}

// ---- growth bookkeeping ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void band_promote_kernel(uint8_t* __restrict__ mark, uint8_t* __restrict__ is_cell,
                                                           const int32_t* __restrict__ table, uint8_t* __restrict__ need, BandDims d) {
  const int64_t nt = (int64_t)d.nbp * d.nbp * d.nbp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt || !mark[i]) return;
  if (is_cell[i]) {  // already meshed: nothing new
    mark[i] = 0;
    return;
  }
  is_cell[i] = 1;  // stays marked: the list of new cell bricks is surf_compact(mark)
  int bx, by, bz;
  band_brick_xyz(d.nbp, (int)i, bx, by, bz);
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // itself and the forward halo whose points its upper-face cells read
    const int x = bx + kCx[k], y = by + kCy[k], z = bz + kCz[k];
    if (x >= d.nbp || y >= d.nbp || z >= d.nbp) continue;
    const int64_t j = band_brick_id(d.nbp, x, y, z);
    if (table[j] < 0) need[j] = 1;
  }
}

__global__ __launch_bounds__(256) void band_assign_kernel(const int32_t* __restrict__ ids, int64_t m, int32_t slot0,
                                                          int32_t* __restrict__ table, int32_t* __restrict__ bricks,
                                                          uint8_t* __restrict__ need) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int32_t id = ids[j];
  table[id] = slot0 + (int32_t)j;
  bricks[slot0 + j] = id;
  need[id] = 0;
}

__global__ __launch_bounds__(256) void band_clear_kernel(const int32_t* __restrict__ ids, int64_t m, uint8_t* __restrict__ mark) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) mark[ids[j]] = 0;
}

// one thread per cell of a new cell brick; only cells on a brick face can have an edge whose incident cells lie in other bricks
__global__ __launch_bounds__(256) void band_grow_kernel(const float* __restrict__ vals, const int32_t* __restrict__ table,
                                                        const uint8_t* __restrict__ is_cell, const int32_t* __restrict__ ids, int64_t m,
                                                        BandDims d, double iso, uint8_t* __restrict__ mark) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * 512) return;
  const int id = ids[t >> 9], l = (int)(t & 511);
  const int lx = l >> 6, ly = (l >> 3) & 7, lz = l & 7;
  if (!(lx == 0 || lx == 7 || ly == 0 || ly == 7 || lz == 0 || lz == 7)) return;
  int bx, by, bz;
  band_brick_xyz(d.nbp, id, bx, by, bz);
  const int x = bx * 8 + lx, y = by * 8 + ly, z = bz * 8 + lz;
  const int last = d.n - 2;  // largest cell origin
  if (x > last || y > last || z > last) return;
  unsigned cs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) cs |= (inside(band_val(d, table, vals, x + kCx[k], y + kCy[k], z + kCz[k]), iso) ? 1u : 0u) << k;
  if (cs == 0 || cs == 255) return;
  for (int e = 0; e < 12; ++e) {
    const int oc = kEo[e], a = kEa[e];
    if (((cs >> oc) & 1u) == ((cs >> kEe[e]) & 1u)) continue;
    const int qx = x + kCx[oc], qy = y + kCy[oc], qz = z + kCz[oc];
    // the cells incident to edge (q, a): q minus 0/1 along each of the two other axes
    for (int s = 0; s < 4; ++s) {
      const int sb = s & 1, sc = s >> 1;
      const int cx = qx - (a == 0 ? 0 : sb), cy = qy - (a == 1 ? 0 : (a == 0 ? sb : sc)), cz = qz - (a == 2 ? 0 : sc);
      if (cx < 0 || cy < 0 || cz < 0 || cx > last || cy > last || cz > last) continue;
      const int b = band_brick_of<int>(d.nbp, cx, cy, cz);
      if (!is_cell[b]) mark[b] = 1;
    }
  }
}

// ---- fp32 path: brick points as a point tensor (the same floats the lattice mode reads from the axes) ------------------
__global__ __launch_bounds__(256) void band_points_kernel(const float* __restrict__ ax, const float* __restrict__ ay,
                                                          const float* __restrict__ az, const int32_t* __restrict__ bricks, int64_t m,
                                                          BandDims d, float* __restrict__ pts) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * 512) return;
  int bx, by, bz;
  band_brick_xyz(d.nbp, bricks[t >> 9], bx, by, bz);
  const int l = (int)(t & 511);
  const int last = d.n - 1;  // clipped points repeat the last lattice point (their values are never read)
  const int x = min(bx * 8 + (l >> 6), last), y = min(by * 8 + ((l >> 3) & 7), last), z = min(bz * 8 + (l & 7), last);
  pts[t * 3 + 0] = ax[x];
  pts[t * 3 + 1] = ay[y];
  pts[t * 3 + 2] = az[z];
}

// ---- classify -------------------------------------------------------------------------------------------------------
// does the lattice edge (q, axis a) belong to a cell of a cell brick?
__device__ __forceinline__ bool edge_meshed(const BandDims& d, const uint8_t* __restrict__ is_cell, int qx, int qy, int qz, int a) {
  const int last = d.n - 2;
  for (int s = 0; s < 4; ++s) {
    const int sb = s & 1, sc = s >> 1;
    const int cx = qx - (a == 0 ? 0 : sb), cy = qy - (a == 1 ? 0 : (a == 0 ? sb : sc)), cz = qz - (a == 2 ? 0 : sc);
    if (cx < 0 || cy < 0 || cz < 0 || cx > last || cy > last || cz > last) continue;
    if (is_cell[band_brick_of<int>(d.nbp, cx, cy, cz)]) return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void band_classify_kernel(const float* __restrict__ vals, const int32_t* __restrict__ table,
                                                            const uint8_t* __restrict__ is_cell, const int32_t* __restrict__ bricks,
                                                            int64_t n_slots, BandDims d, double iso, uint8_t* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_slots * 512) return;
  const int id = bricks[t >> 9];
  int x, y, z;
  band_point_xyz(d.nbp, id, (int)(t & 511), x, y, z);
  unsigned f = 0;
  if (x < d.n && y < d.n && z < d.n) {
    const bool cell = is_cell[id] != 0;
    const bool in0 = inside(vals[t], iso);
    const bool h[3] = {x + 1 < d.n, y + 1 < d.n, z + 1 < d.n};
    for (int a = 0; a < 3; ++a) {
      if (!h[a]) continue;
      if (!cell && !edge_meshed(d, is_cell, x, y, z, a)) continue;
      const float v = band_val(d, table, vals, x + (a == 0), y + (a == 1), z + (a == 2));
      if (inside(v, iso) != in0) f |= 1u << a;
    }
    if (cell && h[0] && h[1] && h[2]) {
      unsigned cs = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) cs |= (inside(band_val(d, table, vals, x + kCx[k], y + kCy[k], z + kCz[k]), iso) ? 1u : 0u) << k;
      f |= (unsigned)MC_NTRI[cs] << 3;
    }
  }
  flags[t] = (uint8_t)f;
}

// ---- dense order ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void band_keys_kernel(const int32_t* __restrict__ pos, int64_t m, const int32_t* __restrict__ bricks,
                                                        BandDims d, int64_t* __restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int32_t p = pos[j];
  int bx, by, bz;
  band_brick_xyz(d.nbp, bricks[p >> 9], bx, by, bz);
  const int l = p & 511;
  const int64_t x = bx * 8 + (l >> 6), y = by * 8 + ((l >> 3) & 7), z = bz * 8 + (l & 7);
  keys[j] = (x * d.n + y) * d.n + z;
}

__global__ __launch_bounds__(256) void band_rank_kernel(const int64_t* __restrict__ keys, int64_t m, const int32_t* __restrict__ table,
                                                        BandDims d, int32_t* __restrict__ pos) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int64_t k = keys[j];
  const int z = (int)(k % d.n), y = (int)((k / d.n) % d.n), x = (int)(k / ((int64_t)d.n * d.n));
  pos[j] = (int32_t)band_pos(d, table, x, y, z);  // a flagged point's brick is in the table
}

// ---- emit -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int block_excl_scan_1024(int c, int* s_part /*16*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_part[wave] = incl;
  __syncthreads();
  int off = 0;
  for (int w = 0; w < wave; ++w) off += s_part[w];
  __syncthreads();
  return off + incl - c;
}

__device__ __forceinline__ void key_xyz(const BandDims& d, int64_t k, int& x, int& y, int& z) {
  z = (int)(k % d.n);
  y = (int)((k / d.n) % d.n);
  x = (int)(k / ((int64_t)d.n * d.n));
}

__global__ __launch_bounds__(1024) void band_vertex_kernel(const float* __restrict__ vals, const int32_t* __restrict__ table, BandDims d,
                                                           double iso, const uint8_t* __restrict__ flags, const int64_t* __restrict__ keys,
                                                           const int32_t* __restrict__ pos, int64_t m, const int32_t* __restrict__ ws,
                                                           int32_t* __restrict__ vbase, double* __restrict__ vertices) {
  __shared__ int s_part[16];
  const int64_t e = (int64_t)blockIdx.x * BAND_BLOCK + threadIdx.x;
  const int32_t p = e < m ? pos[e] : 0;
  const unsigned f = e < m ? flags[p] : 0u;
  const int nv = __popc(f & 7u);
  int off = ws[blockIdx.x] + block_excl_scan_1024(nv, s_part);
  if (e >= m) return;
  vbase[p] = off;
  if (nv == 0) return;
  int x, y, z;
  key_xyz(d, keys[e], x, y, z);
  const double f1 = (double)vals[p];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    if (!(f & (1u << axis))) continue;
    const double f2 = (double)band_val(d, table, vals, x + (axis == 0), y + (axis == 1), z + (axis == 2));
    // mc_vertex_kernel's interpolation, operation for operation
    const double t = f2 == f1 ? 0.5 : (1.0 * (iso - f1)) / (f2 - f1);
    double vx = (double)x, vy = (double)y, vz = (double)z;
    if (axis == 0) vx = t + vx;
    else if (axis == 1) vy = t + vy;
    else vz = t + vz;
    vertices[(int64_t)off * 3 + 0] = vx;
    vertices[(int64_t)off * 3 + 1] = vy;
    vertices[(int64_t)off * 3 + 2] = vz;
    ++off;
  }
}

__global__ __launch_bounds__(1024) void band_triangle_kernel(const float* __restrict__ vals, const int32_t* __restrict__ table, BandDims d,
                                                             double iso, const uint8_t* __restrict__ flags, const int64_t* __restrict__ keys,
                                                             const int32_t* __restrict__ pos, int64_t m, int nb,
                                                             const int32_t* __restrict__ ws, const int32_t* __restrict__ vbase,
                                                             int32_t* __restrict__ triangles) {
  __shared__ int s_part[16];
  const int64_t e = (int64_t)blockIdx.x * BAND_BLOCK + threadIdx.x;
  const int32_t p = e < m ? pos[e] : 0;
  const unsigned f = e < m ? flags[p] : 0u;
  const int nt = (int)((f >> 3) & 7u);
  int off = ws[nb + blockIdx.x] + block_excl_scan_1024(nt, s_part);
  if (e >= m || nt == 0) return;
  int x, y, z;
  key_xyz(d, keys[e], x, y, z);
  unsigned cs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) cs |= (inside(band_val(d, table, vals, x + kCx[k], y + kCy[k], z + kCz[k]), iso) ? 1u : 0u) << k;
  for (int t = 0; t < nt; ++t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int edge = MC_TRI[cs][3 * t + k];
      const int oc = kEo[edge], axis = kEa[edge];
      const int64_t q = band_pos(d, table, x + kCx[oc], y + kCy[oc], z + kCz[oc]);
      const unsigned fq = q < 0 ? 0u : flags[q];
      triangles[(int64_t)off * 3 + k] = (q < 0 ? -1 : vbase[q]) + __popc(fq & ((1u << axis) - 1u));
    }
    ++off;
  }
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int dims_of(int n, BandDims& d) {
  if (n < 2 || n > SURF_BAND_MAX_RES) return SURF_E_ARG;
  d.n = n;
  d.nbp = (n + 7) / 8;
  d.nbc = (n - 1 + 7) / 8;
  return 0;
}

}  // namespace

extern "C" int64_t surf_band_table_size(int n) {
  BandDims d;
  if (dims_of(n, d)) return -1;
  return (int64_t)d.nbp * d.nbp * d.nbp;
}

extern "C" int surf_band_screen(const float* uc, const float* cax, const float* cay, const float* caz, int n, double isovalue,
                                double margin, uint8_t* mark, void* stream) {
  BandDims d;
  if (!uc || !cax || !cay || !caz || !mark || !(margin >= 0.0) || dims_of(n, d)) return SURF_E_ARG;
  const int64_t nc = (int64_t)d.nbc * d.nbc * d.nbc;
  hipLaunchKernelGGL(band_screen_kernel, dim3(blocks_of(nc, 256)), dim3(256), 0, (hipStream_t)stream, uc, cax, cay, caz, d, isovalue,
                     margin, mark);
  return surf_check_launch();
}

extern "C" int surf_band_promote(uint8_t* mark, uint8_t* is_cell, const int32_t* table, uint8_t* need, int n, void* stream) {
  BandDims d;
  if (!mark || !is_cell || !table || !need || dims_of(n, d)) return SURF_E_ARG;
  const int64_t nt = (int64_t)d.nbp * d.nbp * d.nbp;
  hipLaunchKernelGGL(band_promote_kernel, dim3(blocks_of(nt, 256)), dim3(256), 0, (hipStream_t)stream, mark, is_cell, table, need, d);
  return surf_check_launch();
}

extern "C" int surf_band_assign(const int32_t* ids, int64_t m, int32_t slot0, int32_t* table, int32_t* bricks, uint8_t* need,
                                void* stream) {
  if (!ids || !table || !bricks || !need || m < 0 || slot0 < 0) return SURF_E_ARG;
  if ((int64_t)slot0 + m > ((int64_t)1 << 31) / 512) return SURF_E_LIMIT;  // int32 band positions
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_assign_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, (hipStream_t)stream, ids, m, slot0, table, bricks, need);
  return surf_check_launch();
}

extern "C" int surf_band_clear(const int32_t* ids, int64_t m, uint8_t* mark, void* stream) {
  if (!ids || !mark || m < 0) return SURF_E_ARG;
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_clear_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, (hipStream_t)stream, ids, m, mark);
  return surf_check_launch();
}

extern "C" int surf_band_grow(const float* vals, const int32_t* table, const uint8_t* is_cell, const int32_t* ids, int64_t m, int n,
                              double isovalue, uint8_t* mark, void* stream) {
  BandDims d;
  if (!vals || !table || !is_cell || !ids || !mark || m < 0 || dims_of(n, d)) return SURF_E_ARG;
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_grow_kernel, dim3(blocks_of(m * 512, 256)), dim3(256), 0, (hipStream_t)stream, vals, table, is_cell, ids, m, d,
                     isovalue, mark);
  return surf_check_launch();
}

extern "C" int surf_band_points(const float* ax, const float* ay, const float* az, const int32_t* bricks, int64_t m, int n, float* pts,
                                void* stream) {
  BandDims d;
  if (!ax || !ay || !az || !bricks || !pts || m < 0 || dims_of(n, d)) return SURF_E_ARG;
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_points_kernel, dim3(blocks_of(m * 512, 256)), dim3(256), 0, (hipStream_t)stream, ax, ay, az, bricks, m, d, pts);
  return surf_check_launch();
}

extern "C" int surf_band_classify(const float* vals, const int32_t* table, const uint8_t* is_cell, const int32_t* bricks, int64_t n_slots,
                                  int n, double isovalue, uint8_t* flags, void* stream) {
  BandDims d;
  if (!vals || !table || !is_cell || !bricks || !flags || n_slots < 0 || dims_of(n, d)) return SURF_E_ARG;
  if (n_slots * 512 >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (n_slots == 0) return 0;
  hipLaunchKernelGGL(band_classify_kernel, dim3(blocks_of(n_slots * 512, 256)), dim3(256), 0, (hipStream_t)stream, vals, table, is_cell,
                     bricks, n_slots, d, isovalue, flags);
  return surf_check_launch();
}

extern "C" int surf_band_keys(const int32_t* pos, int64_t m, const int32_t* bricks, int n, int64_t* keys, void* stream) {
  BandDims d;
  if (!pos || !bricks || !keys || m < 0 || dims_of(n, d)) return SURF_E_ARG;
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_keys_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, (hipStream_t)stream, pos, m, bricks, d, keys);
  return surf_check_launch();
}

extern "C" int surf_band_rank(const int64_t* keys, int64_t m, const int32_t* table, int n, int32_t* pos, void* stream) {
  BandDims d;
  if (!keys || !table || !pos || m < 0 || dims_of(n, d)) return SURF_E_ARG;
  if (m == 0) return 0;
  hipLaunchKernelGGL(band_rank_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, (hipStream_t)stream, keys, m, table, d, pos);
  return surf_check_launch();
}

extern "C" int surf_band_emit(const float* vals, const int32_t* table, int n, double isovalue, const uint8_t* flags, const int64_t* keys,
                              const int32_t* pos, int64_t m, const int32_t* workspace, int32_t* vbase, double* vertices, int32_t* triangles,
                              void* stream) {
  BandDims d;
  if (!vals || !table || !flags || !keys || !pos || !workspace || !vbase || m <= 0 || dims_of(n, d)) return SURF_E_ARG;
  const int nb = (int)((m + BAND_BLOCK - 1) / BAND_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(band_vertex_kernel, dim3(nb), dim3(1024), 0, st, vals, table, d, isovalue, flags, keys, pos, m, workspace, vbase,
                     vertices);
  hipLaunchKernelGGL(band_triangle_kernel, dim3(nb), dim3(1024), 0, st, vals, table, d, isovalue, flags, keys, pos, m, nb, workspace,
                     vbase, triangles);
  return surf_check_launch();
}
