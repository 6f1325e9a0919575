// Mesh smoothing on the device (surf_amd/mesh_smooth.py, backend="device"): Laplacian and Taubin lambda|mu steps with uniform
// weights (Taubin 1995, "A signal processing approach to fair surface design"), an optional displacement cap and area-weighted
// vertex normals of the result.
//
// THE RULE is written once, in include/surf_hip.h above the surf_smooth_* entry points (rules 1-5); surf_amd/mesh_smooth.py's
// host path mirrors it operation for operation in numpy fp64, and the arrays of the two paths are equal.  What this file adds:
//  * All arithmetic is fp64 on fp32 positions; the library is compiled with -ffp-contract=off, so every operator below is one IEEE
//    operation, and fp64 division and sqrt are correctly rounded on gfx950 as they are in numpy.
//  * ADJACENCY: edge_keys_kernel writes two directed 64-bit keys per edge; the caller sorts them (torch.sort) and scans the run
//    heads; adjacency_kernel writes the first key of every run into the neighbour list, which is then a CSR with ascending
//    neighbours per row, and marks the source of every run of length one as boundary.  No atomics of any kind.
//  * THE STEP (the hot path): a sparse gather of degree about 6 from 16-byte position rows, one vertex per lane.  A lane issues its
//    gathers up to eight at a time (only those there are) before it adds them in order, so its loads are in flight together;
//    marching cubes emits vertices in lattice order, so the rows of a wave's neighbours share cache lines.  The sum is SEQUENTIAL
//    in ascending neighbour order: that is the rule, so a vertex of degree d costs d dependent fp64 adds wherever it runs.
//    The neighbour entries of a wave's 64 vertices are one contiguous run of the list and are read once, coalesced, into LDS
//    (16 KiB per block); blocks are dealt so that every XCD's L2 serves one contiguous eighth of the vertices.  Measured on the
//    10 M-vertex height field: 0.198 ms per step with per-lane index loads and padded gathers, 0.176 with the gathers masked and
//    the XCD deal, 0.157 with the LDS run as well.
//    A vertex of more than SURF_SMOOTH_WAVE_DEGREE neighbours (a fan hub) is taken out of the per-lane loop: after the loop the
//    wave serves such vertices one at a time, all 64 lanes gathering 64 neighbours at once (coalesced index reads) and every
//    lane adding the 64 values in lane order from v_readlane - the memory latency is paid once per 64 neighbours, not once per
//    neighbour, the other waves never wait, and no buffer depends on the degree (a wave whose run exceeds its LDS part reads
//    the entries from memory).
//  * Compulsory bytes per step and vertex: 16 (own row) + 16 (row out) + 4 (row_start) + 1 (boundary) + 4 d (indices), 61 at d = 6;
//    the neighbours' rows are re-reads of rows that some lane reads as its own.  DESIGN.md K21 has the measurements.
//  * cap_kernel / sum256_kernel: rule 4 and the movement statistics; the 256-ary sequential tree is one thread per run.
//  * face_normal_kernel / vertex_normal_kernel: rule 5, one thread per face, then one per vertex walking its corners in (face,
//    corner) order (the caller's stable sort of the face array), eight face normals in flight.
// 256 threads per block.  Offline tool, not part of the training / render hot path.
#include <math.h>

#include "common.h"

namespace {

constexpr int64_t kMaxItems = SURF_SMOOTH_MAX_ITEMS;
constexpr int64_t kNoKey = SURF_SMOOTH_NO_KEY;
constexpr int kWaveDegree = SURF_SMOOTH_WAVE_DEGREE;
constexpr int kBatch = 8;                            // gathers a lane has in flight
constexpr int kStageEntries = 1024;                  // neighbour entries of one wave's vertices kept in LDS (mean degree 16)

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// ---- rule 1 ----

__global__ __launch_bounds__(256) void edge_keys_kernel(const int32_t* __restrict__ faces, int64_t m, int64_t n,
                                                        int64_t* __restrict__ keys, int32_t* __restrict__ flag) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t v[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
  const bool ok = v[0] >= 0 && v[0] < n && v[1] >= 0 && v[1] < n && v[2] >= 0 && v[2] < n;
  if (!ok) flag[0] = 1;
  int64_t fwd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t a = v[k], b = v[(k + 1) % 3];
    const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
    fwd[k] = (lo << 32) | hi;
    bool drop = !ok || lo == hi;
    for (int e = 0; e < k; ++e) drop = drop || fwd[e] == fwd[k];     // the face has this edge already
    keys[f * 6 + 2 * k] = drop ? kNoKey : fwd[k];
    keys[f * 6 + 2 * k + 1] = drop ? kNoKey : ((hi << 32) | lo);
  }
}

__global__ __launch_bounds__(256) void adjacency_kernel(const int64_t* __restrict__ skeys, const int64_t* __restrict__ hscan,
                                                        int64_t count, int64_t n, int64_t nnz, int32_t* __restrict__ nbr,
                                                        uint8_t* __restrict__ boundary) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const int64_t key = skeys[j];
  if (key == kNoKey || key < 0) return;
  if (j > 0 && skeys[j - 1] == key) return;                       // not the head of its run
  const int64_t r = hscan[j] - 1, a = key >> 32, b = key & 0xffffffffll;
  if (r < 0 || r >= nnz || a >= n || b >= n) return;
  nbr[r] = (int32_t)b;
  if (j + 1 == count || skeys[j + 1] != key) boundary[a] = 1;     // one face has this edge; every writer stores the same 1
}

// ---- rule 2 ----

// The light lanes' sum: the gathers of up to kBatch neighbours are issued (only for the neighbours there are) before they are
// added in order.  index(q) is entry q of the neighbour list, from LDS or from memory.
template <class Index>
__device__ __forceinline__ void gather_sum(const f32x4* __restrict__ P, int64_t n, int64_t i, int32_t b, int32_t e, Index index,
                                           double (&S)[3]) {
  for (int32_t q = b; q < e; q += kBatch) {
    f32x4 v[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (q + k < e) {
        int64_t j = index(q + k);
        if (j < 0 || j >= n) j = i;                                  // never taken with the caller's adjacency: a bounds guard only
        v[k] = P[j];
      }
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (q + k < e) {
        S[0] = S[0] + (double)v[k][0];
        S[1] = S[1] + (double)v[k][1];
        S[2] = S[2] + (double)v[k][2];
      }
    }
  }
}

__global__ __launch_bounds__(256) void step_kernel(const f32x4* __restrict__ P, f32x4* __restrict__ Q, int64_t n,
                                                   const int32_t* __restrict__ row, const int32_t* __restrict__ nbr, int32_t nnz,
                                                   const uint8_t* __restrict__ boundary, int pin, double s) {
  // Consecutive block ids go round the 8 XCDs, each with an L2 of its own, while a vertex's neighbours sit one lattice row away,
  // a dozen blocks on: give every XCD one contiguous run of the vertices, so that those rows are in ITS L2.  Speed only.
  const unsigned per = gridDim.x / 8, rest = gridDim.x % 8, xcd = blockIdx.x % 8;
  const unsigned block = xcd * per + min(xcd, rest) + blockIdx.x / 8;
  const int64_t i = (int64_t)block * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (SURF_WAVE - 1);
  const bool live = i < n;
  int32_t b = 0, e = 0;
  f32x4 self = {0.f, 0.f, 0.f, 0.f};
  bool fixed = true;
  if (live) {
    b = max(row[i], 0);
    e = max(min(row[i + 1], nnz), b);
    self = P[i];
    fixed = e == b || (pin && boundary[i]);
  }
  // The neighbour entries of a wave's 64 vertices are one contiguous run of the list: read it once, coalesced, into the wave's
  // part of LDS.  Read by each lane for itself the entries are 4-byte loads 24 bytes apart, and every one of a lane's loads
  // passes the same dozen cache lines through the vector cache again.  A run that does not fit (a hub) is read from memory.
  __shared__ int32_t stage[4][kStageEntries];
  const int wave = threadIdx.x >> 6;
  int32_t wb = 0, we = 0;
  const int64_t i0 = i - lane;
  if (i0 < n) {
    wb = __builtin_amdgcn_readfirstlane(max(min(row[i0], nnz), 0));
    we = __builtin_amdgcn_readfirstlane(max(min(row[min(i0 + SURF_WAVE, n)], nnz), wb));
  }
  const bool staged = we - wb <= kStageEntries;
  if (staged)
    for (int32_t t = lane; t < we - wb; t += SURF_WAVE) stage[wave][t] = nbr[wb + t];
  __syncthreads();                                                   // every thread of the block arrives: nobody has returned
  const bool heavy = !fixed && e - b > kWaveDegree;
  double S[3] = {0.0, 0.0, 0.0};
  if (!fixed && !heavy) {
    if (staged && b >= wb && e <= we)
      gather_sum(P, n, i, b, e, [&](int32_t q) { return (int64_t)stage[wave][q - wb]; }, S);
    else
      gather_sum(P, n, i, b, e, [&](int32_t q) { return (int64_t)nbr[q]; }, S);
  }
  // vertices of large degree, one after the other, by the whole wave; every lane of the wave arrives here
  unsigned long long todo = __ballot(heavy);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int32_t hb = __builtin_amdgcn_readlane(b, owner), he = __builtin_amdgcn_readlane(e, owner);
    double T[3] = {0.0, 0.0, 0.0};
    for (int32_t base = hb; base < he; base += SURF_WAVE) {
      const int32_t q = base + lane;
      const int64_t j = q < he ? (int64_t)nbr[q] : -1;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (j >= 0 && j < n) v = P[j];
      const int cnt = min(SURF_WAVE, he - base);
      for (int k = 0; k < cnt; ++k) {                              // k is wave-uniform: three v_readlane per neighbour
        T[0] = T[0] + (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[0]), k));
        T[1] = T[1] + (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[1]), k));
        T[2] = T[2] + (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[2]), k));
      }
    }
    if (lane == owner) {
      S[0] = T[0];
      S[1] = T[1];
      S[2] = T[2];
    }
  }
  if (!live) return;
  f32x4 out = self;
  if (!fixed) {
    const double d = (double)(e - b);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double x = (double)self[a];
      const double mean = S[a] / d;
      out[a] = (float)(x + s * (mean - x));
    }
  }
  Q[i] = out;
}

// ---- rule 4 ----

__global__ __launch_bounds__(256) void cap_kernel(const f32x4* __restrict__ P, const float* __restrict__ V0, int64_t n, double M,
                                                  float* __restrict__ out, double* __restrict__ moved2, uint8_t* __restrict__ capped) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f32x4 p = P[i];
  float x[3] = {p[0], p[1], p[2]};
  const double x0[3] = {(double)V0[i * 3 + 0], (double)V0[i * 3 + 1], (double)V0[i * 3 + 2]};
  double d[3] = {(double)x[0] - x0[0], (double)x[1] - x0[1], (double)x[2] - x0[2]};
  double q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const bool cap = M > 0.0 && q > M * M;
  if (cap) {
    const double r = M / sqrt(q);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      x[a] = (float)(x0[a] + d[a] * r);
      d[a] = (double)x[a] - x0[a];
    }
    q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  }
  out[i * 3 + 0] = x[0];
  out[i * 3 + 1] = x[1];
  out[i * 3 + 2] = x[2];
  moved2[i] = q;
  capped[i] = cap ? 1 : 0;
}

__global__ __launch_bounds__(256) void sum256_kernel(const double* __restrict__ values, int64_t count, double* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t lo = r * 256;
  if (lo >= count) return;
  const int64_t hi = min(lo + 256, count);
  double s = 0.0;
  for (int64_t k = lo; k < hi; ++k) s = s + values[k];
  out[r] = s;
}

// ---- rule 5 ----

__global__ __launch_bounds__(256) void face_normal_kernel(const float* __restrict__ V, int64_t n, const int32_t* __restrict__ faces,
                                                          int64_t m, double* __restrict__ F) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  double c[3] = {0.0, 0.0, 0.0};
  if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {
    const double p0[3] = {(double)V[i0 * 3 + 0], (double)V[i0 * 3 + 1], (double)V[i0 * 3 + 2]};
    const double e1[3] = {(double)V[i1 * 3 + 0] - p0[0], (double)V[i1 * 3 + 1] - p0[1], (double)V[i1 * 3 + 2] - p0[2]};
    const double e2[3] = {(double)V[i2 * 3 + 0] - p0[0], (double)V[i2 * 3 + 1] - p0[1], (double)V[i2 * 3 + 2] - p0[2]};
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
  }
  F[f * 3 + 0] = c[0];
  F[f * 3 + 1] = c[1];
  F[f * 3 + 2] = c[2];
}

__global__ __launch_bounds__(256) void vertex_normal_kernel(const double* __restrict__ F, int64_t m, const int64_t* __restrict__ corder,
                                                            const int64_t* __restrict__ cstart, int64_t n,
                                                            const float* __restrict__ given, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t b = max(cstart[i], (int64_t)0), e = min(cstart[i + 1], m * 3);
  double S[3] = {0.0, 0.0, 0.0};
  for (int64_t q = b; q < e; q += kBatch) {
    double t[kBatch][3];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      int64_t c = q + k < e ? corder[q + k] : 0;
      if (c < 0 || c >= m * 3) c = 0;                                // a bounds guard only
      const int64_t f = c / 3;
      t[k][0] = F[f * 3 + 0];
      t[k][1] = F[f * 3 + 1];
      t[k][2] = F[f * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (q + k < e) {
        S[0] = S[0] + t[k][0];
        S[1] = S[1] + t[k][1];
        S[2] = S[2] + t[k][2];
      }
    }
  }
  const double L2 = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2];
  float nrm[3] = {0.f, 0.f, 0.f};
  if (L2 > 0.0 && L2 <= 1.7976931348623157e308) {                   // false for 0, NaN and inf
    const double L = sqrt(L2);
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[a] = (float)(S[a] / L);
    if (given) {
      const double t = ((double)nrm[0] * (double)given[i * 3 + 0] + (double)nrm[1] * (double)given[i * 3 + 1]) +
                       (double)nrm[2] * (double)given[i * 3 + 2];
      if (t < 0.0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) nrm[a] = -nrm[a];
      }
    }
  }
  out[i * 3 + 0] = nrm[0];
  out[i * 3 + 1] = nrm[1];
  out[i * 3 + 2] = nrm[2];
}

inline bool finite_f64(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

}  // namespace

extern "C" int surf_smooth_edge_keys(const int32_t* faces, int64_t m, int64_t n, int64_t* keys, int32_t* flag, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (m == 0) return 0;
  if (!faces || !keys || !flag) return SURF_E_ARG;
  hipLaunchKernelGGL(edge_keys_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, faces, m, n, keys, flag);
  return surf_check_launch();
}

extern "C" int surf_smooth_adjacency(const int64_t* sorted_keys, const int64_t* head_scan, int64_t m, int64_t n, int64_t nnz,
                                     int32_t* neighbours, uint8_t* boundary, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0 || nnz < 0 || nnz > 6 * m) return SURF_E_ARG;
  if (m == 0 || n == 0 || nnz == 0) return 0;
  if (!sorted_keys || !head_scan || !neighbours || !boundary) return SURF_E_ARG;
  hipLaunchKernelGGL(adjacency_kernel, dim3(blocks(6 * m)), dim3(256), 0, (hipStream_t)stream, sorted_keys, head_scan, 6 * m, n, nnz,
                     neighbours, boundary);
  return surf_check_launch();
}

extern "C" int surf_smooth_step(const float* positions_in, float* positions_out, int64_t n, const int32_t* row_start,
                                const int32_t* neighbours, int64_t nnz, const uint8_t* boundary, int pin_boundary, double s,
                                void* stream) {
  if (n > kMaxItems || nnz > 6 * kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || nnz < 0 || !finite_f64(s)) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!positions_in || !positions_out || positions_in == positions_out || !row_start || !boundary || (nnz > 0 && !neighbours))
    return SURF_E_ARG;
  hipLaunchKernelGGL(step_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)positions_in, (f32x4*)positions_out,
                     n, row_start, neighbours, (int32_t)nnz, boundary, pin_boundary ? 1 : 0, s);
  return surf_check_launch();
}

extern "C" int surf_smooth_cap(const float* positions, const float* vertices0, int64_t n, double max_move, float* out_vertices,
                               double* moved2, uint8_t* capped, void* stream) {
  if (n > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || !finite_f64(max_move) || !finite_f64(max_move * max_move)) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!positions || !vertices0 || !out_vertices || !moved2 || !capped) return SURF_E_ARG;
  hipLaunchKernelGGL(cap_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)positions, vertices0, n, max_move,
                     out_vertices, moved2, capped);
  return surf_check_launch();
}

extern "C" int surf_smooth_sum256(const double* values, int64_t count, double* out, void* stream) {
  if (count > kMaxItems) return SURF_E_LIMIT;
  if (count < 0) return SURF_E_ARG;
  if (count == 0) return 0;
  if (!values || !out || values == out) return SURF_E_ARG;
  hipLaunchKernelGGL(sum256_kernel, dim3(blocks((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values, count, out);
  return surf_check_launch();
}

extern "C" int surf_smooth_normals(const float* vertices, int64_t n, const int32_t* faces, int64_t m, const int64_t* corner_order,
                                   const int64_t* corner_start, const float* given_normals, double* face_normals, float* normals,
                                   void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!vertices || !normals || !corner_start || (m > 0 && (!faces || !corner_order || !face_normals))) return SURF_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (m > 0) hipLaunchKernelGGL(face_normal_kernel, dim3(blocks(m)), dim3(256), 0, s, vertices, n, faces, m, face_normals);
  hipLaunchKernelGGL(vertex_normal_kernel, dim3(blocks(n)), dim3(256), 0, s, (const double*)face_normals, m, corner_order,
                     corner_start, n, given_normals, normals);
  return surf_check_launch();
}
