// Mesh simplification on the device (surf_amd/mesh_simplify.py, backend="device"): vertex clustering on a lattice anchored at the
// world origin, one output vertex per cell placed by the cell's error quadric (Lindstrom 2000; Garland-Heckbert quadrics).
//
// THE RULE is written once, in include/surf_hip.h above the surf_simplify_* entry points (rules 1-8); surf_amd/mesh_simplify.py's
// host path mirrors it operation for operation in numpy fp64, and the arrays of the two paths are equal.  What this file adds:
//  * All arithmetic is fp64; the library is compiled with -ffp-contract=off, so every operator below is one IEEE operation, and
//    fp64 division and sqrt are correctly rounded on gfx950 as they are in numpy.
//  * ACCUMULATION: the sequential one.  The caller's stable sorts by cell keep (face, corner) order among a cell's corners and
//    vertex-index order among its vertices; cell_kernel gives one thread to a cell, which walks the two segments from their first
//    entry to their last and adds each term to running sums that start at +0.  A segment may be of any length.  There are no float
//    atomics and no tree: np.add.at on the host adds the same terms in the same order.  (The order-independent int64 fixed-point
//    sum of volume.hip was the allowed alternative; it was not taken.)
//  * SOLVE: (A + s I) x = b + s mean, s = 2^-20 (A00 + A11 + A22), by LDL^T without pivoting in the written-out sequence of the
//    header (ldl3 below); the matrix is symmetric positive definite with pivots >= s, condition <= 2^20 + 1.
//  * keys_kernel / segments_kernel / face_cells_kernel: rule 1 and the two index tables (vertex -> cell, face -> three cells).
//  * face_insert_kernel / face_keep_kernel: rule 7.  mesh_clean.hip's slot table, with the difference that three cell numbers do
//    not fit a 64-bit key: a slot holds a FACE id, claimed by atomicCAS(empty -> f), and "the same key" means "the slot's face has
//    the same sorted cells".  Only faces of that set ever atomicMin into the slot, so its set never changes, a slot never
//    empties, and every face of a set stops at the same slot of its probe sequence; after the pass the slot holds the set's
//    lowest face id, whatever the order in which the atomics landed.
//  * mark_used_kernel, compact_faces_kernel, vertex_map_kernel: rule 8; the scans between them are the caller's (torch.cumsum).
//    cell_kernel writes a used cell straight to its output row, so vertices, normals and colours need no compaction pass.
// One item per thread, 256 threads; fp64 VALU and gather bound.  Offline tool, not part of the training / render hot path.
#include <math.h>

#include "common.h"

namespace {

constexpr int64_t kHalf = int64_t(1) << 20;         // cell indices lie in [-2^20, 2^20)
constexpr int32_t kEmpty = INT32_MAX;
constexpr int64_t kMaxItems = (int64_t)INT32_MAX / 3;

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void keys_kernel(const float* __restrict__ V, int64_t n, double cell, int64_t* __restrict__ keys,
                                                   int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t key = 0;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double f = floor((double)V[i * 3 + a] / cell);
    ok = ok && f >= -(double)kHalf && f < (double)kHalf;            // false for NaN and +-inf
    key = (key << 21) | (ok ? (int64_t)f + kHalf : (int64_t)0);
  }
  keys[i] = ok ? key : 0;
  if (!ok) flag[0] = 1;
}

__global__ __launch_bounds__(256) void segments_kernel(const int64_t* __restrict__ skeys, const int64_t* __restrict__ order,
                                                       const int64_t* __restrict__ rank, int64_t n, int64_t n_cells,
                                                       int32_t* __restrict__ vcell, int64_t* __restrict__ seg) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t r = rank[j], i = order[j];
  if (r < 0 || r >= n_cells || i < 0 || i >= n) return;
  vcell[i] = (int32_t)r;
  if (j == 0 || skeys[j - 1] != skeys[j]) seg[r] = j;
  if (j == n - 1) seg[n_cells] = n;
}

__global__ __launch_bounds__(256) void face_cells_kernel(const int32_t* __restrict__ faces, int64_t m, const int32_t* __restrict__ vcell,
                                                         int64_t n, int32_t* __restrict__ fcell, int32_t* __restrict__ flag) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  const bool ok = i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n;
  fcell[f * 3 + 0] = ok ? vcell[i0] : 0;
  fcell[f * 3 + 1] = ok ? vcell[i1] : 0;
  fcell[f * 3 + 2] = ok ? vcell[i2] : 0;
  if (!ok) flag[0] = 1;
}

// ---- rule 7 ----

struct Cells3 {
  int32_t a, b, c;          // ascending
};

__device__ __forceinline__ Cells3 sorted_cells(const int32_t* __restrict__ fcell, int64_t f) {
  int32_t a = fcell[f * 3 + 0], b = fcell[f * 3 + 1], c = fcell[f * 3 + 2], t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
  return Cells3{a, b, c};
}

__device__ __forceinline__ uint64_t mix64(uint64_t k) {       // murmur3's finaliser
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

__global__ __launch_bounds__(256) void face_insert_kernel(const int32_t* __restrict__ fcell, int64_t m, int32_t* owner,
                                                          uint32_t slot_mask, uint32_t* __restrict__ face_slot) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const Cells3 me = sorted_cells(fcell, f);
  if (me.a == me.b || me.b == me.c) return;                     // fewer than three distinct cells: dropped, never inserted
  uint32_t s = (uint32_t)mix64(mix64(((uint64_t)(uint32_t)me.a << 32) | (uint32_t)me.b) ^ (uint64_t)(uint32_t)me.c) & slot_mask;
  // the table holds at least twice as many slots as there are faces, so an empty slot always ends the probe
  for (;;) {
    int32_t cur = __hip_atomic_load(&owner[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      cur = atomicCAS(&owner[s], kEmpty, (int32_t)f);
      if (cur == kEmpty) break;                                 // claimed: this face is the slot's first
    }
    // cur is a face id < m that was inserted, whatever face holds the slot by now: all of them have the same cells
    const Cells3 it = sorted_cells(fcell, cur);
    if (it.a == me.a && it.b == me.b && it.c == me.c) {
      atomicMin(&owner[s], (int32_t)f);
      break;
    }
    s = (s + 1) & slot_mask;
  }
  face_slot[f] = s;
}

__global__ __launch_bounds__(256) void face_keep_kernel(const int32_t* __restrict__ fcell, int64_t m, const int32_t* __restrict__ owner,
                                                        const uint32_t* __restrict__ face_slot, uint8_t* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const Cells3 me = sorted_cells(fcell, f);
  keep[f] = (me.a != me.b && me.b != me.c && owner[face_slot[f]] == (int32_t)f) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mark_used_kernel(const int32_t* __restrict__ fcell, const uint8_t* __restrict__ keep, int64_t m,
                                                        int64_t n_cells, uint8_t* __restrict__ used) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m || !keep[f]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t c = fcell[f * 3 + k];
    if (c >= 0 && c < n_cells) used[c] = 1;
  }
}

// ---- rules 2-6 ----

struct CellArgs {
  const float* V;             // (n, 3)
  const float* N;             // (n, 3) or null
  const uint8_t* C;           // (n, 3) or null
  int64_t n;
  const int32_t* faces;       // (m, 3)
  int64_t m;
  double cell;
  const int64_t* skeys;       // (n) sorted keys
  const int64_t* vorder;      // (n)
  const int64_t* vstart;      // (n_cells + 1)
  const int64_t* corder;      // (3 m)
  const int64_t* cstart;      // (n_cells + 1)
  int64_t n_cells;
  const uint8_t* used;        // (n_cells)
  const int64_t* scan;        // (n_cells) inclusive scan of used
  float* outV;
  float* outN;
  uint8_t* outC;
};

// (A + s I) x = b + s mean by LDL^T, the header's sequence; A = (A00, A01, A02, A11, A12, A22)
__device__ __forceinline__ void ldl3(const double (&A)[6], const double (&b)[3], double s, const double (&mean)[3], double (&x)[3]) {
  const double m00 = A[0] + s, m11 = A[3] + s, m22 = A[5] + s;
  const double r0 = b[0] + s * mean[0], r1 = b[1] + s * mean[1], r2 = b[2] + s * mean[2];
  const double l10 = A[1] / m00, l20 = A[2] / m00;
  const double d1 = m11 - l10 * A[1];
  const double u21 = A[4] - l20 * A[1];
  const double l21 = u21 / d1;
  const double d2 = (m22 - l20 * A[2]) - l21 * u21;
  const double y1 = r1 - l10 * r0;
  const double y2 = (r2 - l20 * r0) - l21 * y1;
  x[2] = y2 / d2;
  x[1] = y1 / d1 - l21 * x[2];
  x[0] = (r0 / m00 - l10 * x[1]) - l20 * x[2];
}

__global__ __launch_bounds__(256) void cell_kernel(CellArgs a) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.n_cells || !a.used[c]) return;                    // an unused cell has no output row
  const int64_t vb = max(a.vstart[c], (int64_t)0), ve = min(a.vstart[c + 1], a.n);
  if (vb >= ve) return;
  const double cell = a.cell;
  const int64_t key = a.skeys[vb];
  double centre[3];
  centre[0] = ((double)(((key >> 42) & 0x1fffff) - kHalf) + 0.5) * cell;
  centre[1] = ((double)(((key >> 21) & 0x1fffff) - kHalf) + 0.5) * cell;
  centre[2] = ((double)((key & 0x1fffff) - kHalf) + 0.5) * cell;

  // rule 2: the cell's corners in (face, corner) order
  double A[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  const double cell2 = cell * cell;
  const int64_t cb = max(a.cstart[c], (int64_t)0), ce = min(a.cstart[c + 1], a.m * 3);
  for (int64_t q = cb; q < ce; ++q) {
    const int64_t e = a.corder[q];
    if (e < 0 || e >= a.m * 3) continue;
    const int64_t f = e / 3;
    const int64_t i0 = a.faces[f * 3 + 0], i1 = a.faces[f * 3 + 1], i2 = a.faces[f * 3 + 2];
    if (i0 < 0 || i0 >= a.n || i1 < 0 || i1 >= a.n || i2 < 0 || i2 >= a.n) continue;
    if (i0 == i1 || i1 == i2 || i0 == i2) continue;
    const double p0[3] = {(double)a.V[i0 * 3 + 0], (double)a.V[i0 * 3 + 1], (double)a.V[i0 * 3 + 2]};
    const double e1[3] = {(double)a.V[i1 * 3 + 0] - p0[0], (double)a.V[i1 * 3 + 1] - p0[1], (double)a.V[i1 * 3 + 2] - p0[2]};
    const double e2[3] = {(double)a.V[i2 * 3 + 0] - p0[0], (double)a.V[i2 * 3 + 1] - p0[1], (double)a.V[i2 * 3 + 2] - p0[2]};
    const double cx = e1[1] * e2[2] - e1[2] * e2[1];
    const double cy = e1[2] * e2[0] - e1[0] * e2[2];
    const double cz = e1[0] * e2[1] - e1[1] * e2[0];
    const double L = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(L > 0.0) || !(L <= 1.7976931348623157e308)) continue;   // 0, NaN, inf
    const double nx = cx / L, ny = cy / L, nz = cz / L;
    const double w = (L / 2.0) / cell2;
    const double qx = (p0[0] - centre[0]) / cell, qy = (p0[1] - centre[1]) / cell, qz = (p0[2] - centre[2]) / cell;
    const double d = (nx * qx + ny * qy) + nz * qz;
    const double gx = w * nx, gy = w * ny, gz = w * nz, wd = w * d;
    A[0] += gx * nx;
    A[1] += gx * ny;
    A[2] += gx * nz;
    A[3] += gy * ny;
    A[4] += gy * nz;
    A[5] += gz * nz;
    b[0] += wd * nx;
    b[1] += wd * ny;
    b[2] += wd * nz;
  }

  // rule 3: the cell's vertices in index order
  double u[3] = {0, 0, 0}, S[3] = {0, 0, 0};
  int64_t col[3] = {0, 0, 0}, count = 0;
  for (int64_t q = vb; q < ve; ++q) {
    const int64_t i = a.vorder[q];
    if (i < 0 || i >= a.n) continue;
    ++count;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      u[k] += ((double)a.V[i * 3 + k] - centre[k]) / cell;
      if (a.N) S[k] += (double)a.N[i * 3 + k];
      if (a.C) col[k] += (int64_t)a.C[i * 3 + k];
    }
  }
  if (count == 0) return;

  // rule 5
  const double t = (A[0] + A[3]) + A[5];
  const double mean[3] = {u[0] / (double)count, u[1] / (double)count, u[2] / (double)count};
  double x[3] = {mean[0], mean[1], mean[2]};
  if (t > 0.0) ldl3(A, b, 0x1p-20 * t, mean, x);
  const int64_t o = a.scan[c] - 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double xc = fmin(fmax(x[k], -0.5), 0.5);
    a.outV[o * 3 + k] = (float)(centre[k] + xc * cell);
  }
  // rule 6
  if (a.C) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.outC[o * 3 + k] = (uint8_t)((2 * col[k] + count) / (2 * count));
  }
  if (a.N) {
    const double len = sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
    const bool ok = len > 0.0 && len <= 1.7976931348623157e308;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.outN[o * 3 + k] = ok ? (float)(S[k] / len) : 0.0f;
  }
}

// ---- rule 8 ----

__global__ __launch_bounds__(256) void compact_faces_kernel(const int32_t* __restrict__ fcell, const uint8_t* __restrict__ keep,
                                                            const int64_t* __restrict__ fscan, int64_t m,
                                                            const int64_t* __restrict__ cscan, int64_t n_cells,
                                                            int32_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m || !keep[f]) return;
  int32_t* o = out + (fscan[f] - 1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t c = fcell[f * 3 + k];
    o[k] = (c >= 0 && c < n_cells) ? (int32_t)(cscan[c] - 1) : -1;
  }
}

__global__ __launch_bounds__(256) void vertex_map_kernel(const int32_t* __restrict__ vcell, int64_t n, const uint8_t* __restrict__ used,
                                                         const int64_t* __restrict__ cscan, int64_t n_cells,
                                                         int32_t* __restrict__ vmap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = vcell[i];
  vmap[i] = (c >= 0 && c < n_cells && used[c]) ? (int32_t)(cscan[c] - 1) : -1;
}

}  // namespace

extern "C" int surf_simplify_keys(const float* vertices, int64_t n, double cell, int64_t* keys, int32_t* flag, void* stream) {
  if (n > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || !(cell > 0.0) || !(cell * cell > 0.0) || !(cell * cell <= 1.7976931348623157e308)) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!vertices || !keys || !flag) return SURF_E_ARG;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, vertices, n, cell, keys, flag);
  return surf_check_launch();
}

extern "C" int surf_simplify_segments(const int64_t* sorted_keys, const int64_t* order, const int64_t* rank, int64_t n,
                                      int64_t n_cells, int32_t* vertex_cell, int64_t* segment_start, void* stream) {
  if (n > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || n_cells < 0 || n_cells > n) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!sorted_keys || !order || !rank || !vertex_cell || !segment_start || n_cells == 0) return SURF_E_ARG;
  hipLaunchKernelGGL(segments_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, sorted_keys, order, rank, n, n_cells,
                     vertex_cell, segment_start);
  return surf_check_launch();
}

extern "C" int surf_simplify_face_cells(const int32_t* faces, int64_t m, const int32_t* vertex_cell, int64_t n, int32_t* face_cells,
                                        int32_t* flag, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (m == 0) return 0;
  if (!faces || !vertex_cell || !face_cells || !flag || n == 0) return SURF_E_ARG;
  hipLaunchKernelGGL(face_cells_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, faces, m, vertex_cell, n, face_cells, flag);
  return surf_check_launch();
}

extern "C" int surf_simplify_faces(const int32_t* face_cells, int64_t m, int32_t* owner, int64_t slots, uint32_t* face_slot,
                                   uint8_t* keep, void* stream) {
  if (m > kMaxItems) return SURF_E_LIMIT;
  if (m < 0) return SURF_E_ARG;
  if (m == 0) return 0;
  int64_t want = 1024;
  while (want < 2 * m) want <<= 1;
  if (!face_cells || !owner || !face_slot || !keep || slots != want) return SURF_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if ((e = hipMemsetD32Async((hipDeviceptr_t)owner, kEmpty, (size_t)slots, s)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(face_insert_kernel, dim3(blocks(m)), dim3(256), 0, s, face_cells, m, owner, (uint32_t)(slots - 1), face_slot);
  hipLaunchKernelGGL(face_keep_kernel, dim3(blocks(m)), dim3(256), 0, s, face_cells, m, (const int32_t*)owner,
                     (const uint32_t*)face_slot, keep);
  return surf_check_launch();
}

extern "C" int surf_simplify_mark_used(const int32_t* face_cells, const uint8_t* keep, int64_t m, int64_t n_cells, uint8_t* used,
                                       void* stream) {
  if (m > kMaxItems || n_cells > kMaxItems) return SURF_E_LIMIT;
  if (m < 0 || n_cells < 0) return SURF_E_ARG;
  if (m == 0 || n_cells == 0) return 0;
  if (!face_cells || !keep || !used) return SURF_E_ARG;
  hipLaunchKernelGGL(mark_used_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, face_cells, keep, m, n_cells, used);
  return surf_check_launch();
}

extern "C" int surf_simplify_cells(const float* vertices, const float* normals, const uint8_t* colors, int64_t n, const int32_t* faces,
                                   int64_t m, double cell, const int64_t* sorted_keys, const int64_t* vertex_order,
                                   const int64_t* vertex_start, const int64_t* corner_order, const int64_t* corner_start,
                                   int64_t n_cells, const uint8_t* used, const int64_t* cell_scan, float* out_vertices,
                                   float* out_normals, uint8_t* out_colors, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0 || n_cells < 0 || n_cells > n) return SURF_E_ARG;
  if (!(cell > 0.0) || !(cell * cell > 0.0) || !(cell * cell <= 1.7976931348623157e308)) return SURF_E_ARG;
  if (n == 0 || m == 0 || n_cells == 0) return 0;                 // without faces no cell is used
  if (!vertices || !faces || !sorted_keys || !vertex_order || !vertex_start || !corner_order || !corner_start || !used ||
      !cell_scan || !out_vertices)
    return SURF_E_ARG;
  if ((normals != nullptr) != (out_normals != nullptr) || (colors != nullptr) != (out_colors != nullptr)) return SURF_E_ARG;
  CellArgs a{vertices, normals, colors, n, faces, m, cell, sorted_keys, vertex_order, vertex_start, corner_order, corner_start,
             n_cells, used, cell_scan, out_vertices, out_normals, out_colors};
  hipLaunchKernelGGL(cell_kernel, dim3(blocks(n_cells)), dim3(256), 0, (hipStream_t)stream, a);
  return surf_check_launch();
}

extern "C" int surf_simplify_compact(const int32_t* face_cells, const uint8_t* keep, const int64_t* face_scan, int64_t m,
                                     const int32_t* vertex_cell, int64_t n, const uint8_t* used, const int64_t* cell_scan,
                                     int64_t n_cells, int32_t* out_faces, int32_t* vertex_map, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0 || n_cells < 0 || n_cells > n) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!vertex_cell || !used || !cell_scan || !vertex_map || n_cells == 0) return SURF_E_ARG;
  if (m > 0) {
    if (!face_cells || !keep || !face_scan || !out_faces) return SURF_E_ARG;
    hipLaunchKernelGGL(compact_faces_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, face_cells, keep, face_scan, m,
                       cell_scan, n_cells, out_faces);
  }
  hipLaunchKernelGGL(vertex_map_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, vertex_cell, n, used, cell_scan, n_cells,
                     vertex_map);
  return surf_check_launch();
}
