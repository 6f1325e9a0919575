// Feature-preserving mesh denoising on the device (surf_amd/mesh_denoise.py, backend="device"): two-stage bilateral normal
// filtering - face normals filtered over the faces that share a vertex (Zheng et al. 2011, local iterative scheme), then vertices
// moved to fit them (Sun et al. 2007).
//
// THE RULE is written once, in include/surf_hip.h above the surf_denoise_* entry points (rules 1-6); surf_amd/mesh_denoise.py's
// host path mirrors it operation for operation in numpy fp64, and the arrays of the two paths are equal.  What this file adds:
//  * All arithmetic is fp64 on fp32 data; the library is compiled with -ffp-contract=off, so every operator below is one IEEE
//    operation, and fp64 division and sqrt are correctly rounded on gfx950 as they are in numpy.
//  * RECORDS: a face is a 32-byte row (nx, ny, nz, area | cx, cy, cz, unused), two aligned 16-byte loads per gathered neighbour;
//    a normal iteration writes the first half only.  The zero normal marks the degenerate faces (rule 1).
//  * NEIGHBOURS: one face per lane walks the corner lists of its three vertices twice, once to count and once to write, with the
//    caller's scan between; the list is built once and the normal iterations gather records through it.  No atomics of any kind.
//  * THE STEPS: sequential sums in the rule's order, one face (normal step) or one vertex (vertex step) per lane, the gathers of
//    kBatch rows issued before they are added.  Blocks are dealt so that every XCD's L2 serves one contiguous eighth of the items,
//    as in mesh_smooth.hip.  A row of more than SURF_DENOISE_WAVE_ROW entries is taken out of the per-lane loop: the wave serves
//    such rows one at a time, every lane gathering and weighting one entry, and all lanes adding the 64 terms in lane order from
//    v_readlane, so that the memory latency is paid once per 64 entries.
//  * GUARDS: the caller refuses faces outside the vertex list before any launch, so no index below is ever out of range.  Each
//    index read from memory is still compared with its array's size before it becomes an address, because a stray write can
//    take the device down for everybody; an entry that fails adds nothing, in the per-lane and in the wave path alike.
// 256 threads per block.  Offline tool, not part of the training / render hot path.
#include <math.h>

#include "common.h"

namespace {

constexpr int64_t kMaxItems = SURF_SMOOTH_MAX_ITEMS;
constexpr int64_t kMaxTotal = 2147483647ll;
constexpr int kWaveRow = SURF_DENOISE_WAVE_ROW;
constexpr int kBatch = 4;                            // rows a lane has in flight
constexpr double kMaxF64 = 1.7976931348623157e308;

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
inline bool finite_f64(double x) { return x >= -kMaxF64 && x <= kMaxF64; }

__device__ __forceinline__ double readlane_f64(double x, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), k), hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float readlane_f32(float x, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k));
}

// the item a thread serves: every XCD (consecutive block ids go round the 8 of them) gets one contiguous run.  Speed only.
__device__ __forceinline__ int64_t dealt_item() {
  const unsigned per = gridDim.x / 8, rest = gridDim.x % 8, xcd = blockIdx.x % 8;
  const unsigned block = xcd * per + min(xcd, rest) + blockIdx.x / 8;
  return (int64_t)block * blockDim.x + threadIdx.x;
}

// ---- rules 1 and 2 ----

__global__ __launch_bounds__(256) void face_record_kernel(const float* __restrict__ V, int64_t n, const int32_t* __restrict__ faces,
                                                          int64_t m, f32x4* __restrict__ records, double* __restrict__ sides) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  f32x4 head = {0.f, 0.f, 0.f, 0.f}, tail = {0.f, 0.f, 0.f, 0.f};
  double len[3] = {0.0, 0.0, 0.0};
  if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {
    const double p0[3] = {(double)V[i0 * 3 + 0], (double)V[i0 * 3 + 1], (double)V[i0 * 3 + 2]};
    const double p1[3] = {(double)V[i1 * 3 + 0], (double)V[i1 * 3 + 1], (double)V[i1 * 3 + 2]};
    const double p2[3] = {(double)V[i2 * 3 + 0], (double)V[i2 * 3 + 1], (double)V[i2 * 3 + 2]};
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double F[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double L2 = (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2];
    if (L2 > 0.0 && L2 <= kMaxF64) {                                  // false for 0, NaN and inf
      const double L = sqrt(L2);
      head = f32x4{(float)(F[0] / L), (float)(F[1] / L), (float)(F[2] / L), (float)(0.5 * L)};
      tail = f32x4{(float)(((p0[0] + p1[0]) + p2[0]) / 3.0), (float)(((p0[1] + p1[1]) + p2[1]) / 3.0),
                   (float)(((p0[2] + p1[2]) + p2[2]) / 3.0), 0.f};
    }
    const double d12[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double d20[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
    len[0] = sqrt((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]);            // the side p0p1 is e1
    len[1] = sqrt((d12[0] * d12[0] + d12[1] * d12[1]) + d12[2] * d12[2]);
    len[2] = sqrt((d20[0] * d20[0] + d20[1] * d20[1]) + d20[2] * d20[2]);
  }
  records[f * 2 + 0] = head;
  records[f * 2 + 1] = tail;
  if (sides) {
    sides[f * 3 + 0] = len[0];
    sides[f * 3 + 1] = len[1];
    sides[f * 3 + 2] = len[2];
  }
}

// ---- rule 3 ----

// The walk of rule 3 for face f; take(g) is called for every member of N(f) in order.
template <class Take>
__device__ __forceinline__ void walk_neighbours(const int32_t* __restrict__ faces, int64_t m, int64_t n, int64_t f,
                                                const int64_t* __restrict__ corder, const int64_t* __restrict__ cstart, Take take) {
  const int32_t fv[3] = {faces[f * 3 + 0], faces[f * 3 + 1], faces[f * 3 + 2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t v = fv[k];
    if (v < 0 || v >= n) continue;                                     // GUARDS
    if ((k >= 1 && v == fv[0]) || (k == 2 && v == fv[1])) continue;    // the slot was walked
    const int64_t b = max(cstart[v], (int64_t)0), e = min(cstart[v + 1], m * 3);
    for (int64_t q = b; q < e; ++q) {
      const int64_t c = corder[q];
      if (c < 0 || c >= m * 3) continue;                               // GUARDS
      const int64_t g = c / 3;
      const int j = (int)(c - g * 3);
      const int32_t g0 = faces[g * 3 + 0], g1 = faces[g * 3 + 1], g2 = faces[g * 3 + 2];
      if ((j >= 1 && g0 == v) || (j == 2 && g1 == v)) continue;        // not g's first corner that names v
      if (k >= 1 && (g0 == fv[0] || g1 == fv[0] || g2 == fv[0])) continue;   // taken at slot 0
      if (k == 2 && (g0 == fv[1] || g1 == fv[1] || g2 == fv[1])) continue;   // taken at slot 1
      take((int32_t)g);
    }
  }
}

__global__ __launch_bounds__(256) void neighbour_count_kernel(const int32_t* __restrict__ faces, int64_t m, int64_t n,
                                                              const int64_t* __restrict__ corder, const int64_t* __restrict__ cstart,
                                                              int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  int64_t count = 0;
  walk_neighbours(faces, m, n, f, corder, cstart, [&](int32_t) { ++count; });
  counts[f] = count;
}

__global__ __launch_bounds__(256) void neighbour_emit_kernel(const int32_t* __restrict__ faces, int64_t m, int64_t n,
                                                             const int64_t* __restrict__ corder, const int64_t* __restrict__ cstart,
                                                             const int32_t* __restrict__ row, int64_t total, int32_t* __restrict__ nbr) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t b = max((int64_t)row[f], (int64_t)0), e = min((int64_t)row[f + 1], total);
  int64_t at = b;
  walk_neighbours(faces, m, n, f, corder, cstart, [&](int32_t g) {
    if (at < e) nbr[at] = g;                                           // never past the row the scan gave this face
    ++at;
  });
}

// ---- rule 4 ----

// the term of neighbour record (gh, gt) for a face with normal nf and centroid cf: false if it is skipped
__device__ __forceinline__ bool normal_term(const f32x4 gh, const f32x4 gt, const double (&nf)[3], const double (&cf)[3], double is,
                                            double ir, double (&term)[3]) {
  const double ng[3] = {(double)gh[0], (double)gh[1], (double)gh[2]};
  const double d[3] = {(double)gt[0] - cf[0], (double)gt[1] - cf[1], (double)gt[2] - cf[2]};
  const double ds2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const double us = 1.0 - ds2 * is;
  const double e[3] = {ng[0] - nf[0], ng[1] - nf[1], ng[2] - nf[2]};
  const double dn2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  const double ur = 1.0 - dn2 * ir;
  if (!(us > 0.0) || !(ur > 0.0)) return false;
  const double w = ((double)gh[3] * ((us * us) * (us * us))) * ((ur * ur) * (ur * ur));
  term[0] = w * ng[0];
  term[1] = w * ng[1];
  term[2] = w * ng[2];
  return true;
}

__global__ __launch_bounds__(256) void normal_step_kernel(const f32x4* __restrict__ R, f32x4* __restrict__ Q, int64_t m,
                                                          const int32_t* __restrict__ row, const int32_t* __restrict__ nbr,
                                                          int32_t total, double is, double ir) {
  const int64_t f = dealt_item();
  const int lane = threadIdx.x & (SURF_WAVE - 1);
  const bool live = f < m;
  int32_t b = 0, e = 0;
  f32x4 head = {0.f, 0.f, 0.f, 0.f}, tail = head;
  bool fixed = true;
  if (live) {
    b = min(max(row[f], 0), total);
    e = max(min(row[f + 1], total), b);
    head = R[f * 2 + 0];
    tail = R[f * 2 + 1];
    fixed = e == b || (head[0] == 0.f && head[1] == 0.f && head[2] == 0.f);      // a degenerate face keeps its zero normal
  }
  const double nf[3] = {(double)head[0], (double)head[1], (double)head[2]};
  const double cf[3] = {(double)tail[0], (double)tail[1], (double)tail[2]};
  const bool heavy = !fixed && e - b > kWaveRow;
  double S[3] = {0.0, 0.0, 0.0};
  if (!fixed && !heavy) {
    for (int32_t q = b; q < e; q += kBatch) {
      f32x4 gh[kBatch], gt[kBatch];
      bool there[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        gh[k] = gt[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        there[k] = false;
        if (q + k < e) {
          const int64_t g = nbr[q + k];
          there[k] = g >= 0 && g < m;                                  // GUARDS
          if (there[k]) {
            gh[k] = R[g * 2 + 0];
            gt[k] = R[g * 2 + 1];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        double term[3];
        if (there[k] && normal_term(gh[k], gt[k], nf, cf, is, ir, term)) {
          S[0] = S[0] + term[0];
          S[1] = S[1] + term[1];
          S[2] = S[2] + term[2];
        }
      }
    }
  }
  // long rows, one after the other, by the whole wave; every lane of the wave arrives here
  unsigned long long todo = __ballot(heavy);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int32_t hb = __builtin_amdgcn_readlane(b, owner), he = __builtin_amdgcn_readlane(e, owner);
    const double onf[3] = {(double)readlane_f32(head[0], owner), (double)readlane_f32(head[1], owner),
                           (double)readlane_f32(head[2], owner)};
    const double ocf[3] = {(double)readlane_f32(tail[0], owner), (double)readlane_f32(tail[1], owner),
                           (double)readlane_f32(tail[2], owner)};
    double T[3] = {0.0, 0.0, 0.0};
    for (int32_t base = hb; base < he; base += SURF_WAVE) {
      const int32_t q = base + lane;
      double term[3] = {0.0, 0.0, 0.0};
      bool use = false;
      if (q < he) {
        const int64_t g = nbr[q];
        if (g >= 0 && g < m) use = normal_term(R[g * 2 + 0], R[g * 2 + 1], onf, ocf, is, ir, term);
      }
      const unsigned long long used = __ballot(use);
      const int cnt = min(SURF_WAVE, he - base);
      for (int k = 0; k < cnt; ++k) {                                  // k is wave-uniform
        if ((used >> k) & 1ull) {
          T[0] = T[0] + readlane_f64(term[0], k);
          T[1] = T[1] + readlane_f64(term[1], k);
          T[2] = T[2] + readlane_f64(term[2], k);
        }
      }
    }
    if (lane == owner) {
      S[0] = T[0];
      S[1] = T[1];
      S[2] = T[2];
    }
  }
  if (!live) return;
  f32x4 out = head;
  if (!fixed) {
    const double L2 = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2];
    if (L2 > 0.0 && L2 <= kMaxF64) {
      const double L = sqrt(L2);
      out[0] = (float)(S[0] / L);
      out[1] = (float)(S[1] / L);
      out[2] = (float)(S[2] / L);
    }
  }
  Q[f * 2 + 0] = out;
}

// ---- rule 5 ----

struct Corner {
  f32x4 nrm, xa, xb, xc;
};

// the rows of corner list entry q (face normal and the three current positions); a zero normal if the entry is not usable
__device__ __forceinline__ Corner load_corner(const f32x4* __restrict__ P, int64_t n, const int32_t* __restrict__ faces, int64_t m,
                                              const f32x4* __restrict__ R, const int64_t* __restrict__ corder, int64_t q) {
  Corner c;
  c.nrm = c.xa = c.xb = c.xc = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t id = corder[q];
  if (id < 0 || id >= m * 3) return c;                                 // GUARDS: a zero normal adds nothing
  const int64_t g = id / 3;
  const int64_t ia = faces[g * 3 + 0], ib = faces[g * 3 + 1], ic = faces[g * 3 + 2];
  if (ia < 0 || ia >= n || ib < 0 || ib >= n || ic < 0 || ic >= n) return c;
  c.nrm = R[g * 2 + 0];
  c.xa = P[ia];
  c.xb = P[ib];
  c.xc = P[ic];
  return c;
}

__device__ __forceinline__ bool vertex_term(const Corner& c, const double (&x)[3], double (&term)[3]) {
  if (c.nrm[0] == 0.f && c.nrm[1] == 0.f && c.nrm[2] == 0.f) return false;      // a degenerate face
  const double nr[3] = {(double)c.nrm[0], (double)c.nrm[1], (double)c.nrm[2]};
  const double cen[3] = {(((double)c.xa[0] + (double)c.xb[0]) + (double)c.xc[0]) / 3.0,
                         (((double)c.xa[1] + (double)c.xb[1]) + (double)c.xc[1]) / 3.0,
                         (((double)c.xa[2] + (double)c.xb[2]) + (double)c.xc[2]) / 3.0};
  const double d = ((cen[0] - x[0]) * nr[0] + (cen[1] - x[1]) * nr[1]) + (cen[2] - x[2]) * nr[2];
  term[0] = nr[0] * d;
  term[1] = nr[1] * d;
  term[2] = nr[2] * d;
  return true;
}

__global__ __launch_bounds__(256) void vertex_step_kernel(const f32x4* __restrict__ P, f32x4* __restrict__ Q, int64_t n,
                                                          const int32_t* __restrict__ faces, int64_t m, const f32x4* __restrict__ R,
                                                          const int64_t* __restrict__ corder, const int64_t* __restrict__ cstart,
                                                          const uint8_t* __restrict__ boundary, int pin) {
  const int64_t i = dealt_item();
  const int lane = threadIdx.x & (SURF_WAVE - 1);
  const bool live = i < n;
  int64_t b = 0, e = 0;
  f32x4 self = {0.f, 0.f, 0.f, 0.f};
  bool fixed = true;
  if (live) {
    b = min(max(cstart[i], (int64_t)0), m * 3);
    e = max(min(cstart[i + 1], m * 3), b);
    self = P[i];
    fixed = e == b || (pin && boundary[i]);
  }
  const double x[3] = {(double)self[0], (double)self[1], (double)self[2]};
  const bool heavy = !fixed && e - b > kWaveRow;
  double T[3] = {0.0, 0.0, 0.0};
  int64_t count = 0;
  if (!fixed && !heavy) {
    for (int64_t q = b; q < e; q += kBatch) {
      Corner c[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        c[k].nrm = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q + k < e) c[k] = load_corner(P, n, faces, m, R, corder, q + k);
      }
#pragma unroll
      for (int k = 0; k < kBatch; ++k) {
        double term[3];
        if (q + k < e && vertex_term(c[k], x, term)) {
          T[0] = T[0] + term[0];
          T[1] = T[1] + term[1];
          T[2] = T[2] + term[2];
          ++count;
        }
      }
    }
  }
  // vertices of many corners, one after the other, by the whole wave; every lane of the wave arrives here
  unsigned long long todo = __ballot(heavy);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t hb = ((int64_t)__builtin_amdgcn_readlane((int)(b >> 32), owner) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), owner);
    const int64_t he = ((int64_t)__builtin_amdgcn_readlane((int)(e >> 32), owner) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(e & 0xffffffffll), owner);
    const double ox[3] = {(double)readlane_f32(self[0], owner), (double)readlane_f32(self[1], owner),
                          (double)readlane_f32(self[2], owner)};
    double U[3] = {0.0, 0.0, 0.0};
    int64_t ucount = 0;
    for (int64_t base = hb; base < he; base += SURF_WAVE) {
      const int64_t q = base + lane;
      double term[3] = {0.0, 0.0, 0.0};
      bool use = false;
      if (q < he) use = vertex_term(load_corner(P, n, faces, m, R, corder, q), ox, term);
      const unsigned long long used = __ballot(use);
      const int cnt = (int)min((int64_t)SURF_WAVE, he - base);
      for (int k = 0; k < cnt; ++k) {                                  // k is wave-uniform
        if ((used >> k) & 1ull) {
          U[0] = U[0] + readlane_f64(term[0], k);
          U[1] = U[1] + readlane_f64(term[1], k);
          U[2] = U[2] + readlane_f64(term[2], k);
        }
      }
      ucount += __popcll(used);
    }
    if (lane == owner) {
      T[0] = U[0];
      T[1] = U[1];
      T[2] = U[2];
      count = ucount;
    }
  }
  if (!live) return;
  f32x4 out = self;
  if (!fixed && count > 0) {
    const double k = (double)count;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = (float)(x[a] + T[a] / k);
  }
  Q[i] = out;
}

}  // namespace

extern "C" int surf_denoise_face_records(const float* vertices, int64_t n, const int32_t* faces, int64_t m, float* records,
                                         double* side_lengths, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (n == 0 || m == 0) return 0;
  if (!vertices || !faces || !records) return SURF_E_ARG;
  hipLaunchKernelGGL(face_record_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, vertices, n, faces, m, (f32x4*)records,
                     side_lengths);
  return surf_check_launch();
}

extern "C" int surf_denoise_neighbour_count(const int32_t* faces, int64_t m, int64_t n, const int64_t* corner_order,
                                            const int64_t* corner_start, int64_t* counts, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (n == 0 || m == 0) return 0;
  if (!faces || !corner_order || !corner_start || !counts) return SURF_E_ARG;
  hipLaunchKernelGGL(neighbour_count_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, faces, m, n, corner_order,
                     corner_start, counts);
  return surf_check_launch();
}

extern "C" int surf_denoise_neighbour_emit(const int32_t* faces, int64_t m, int64_t n, const int64_t* corner_order,
                                           const int64_t* corner_start, const int32_t* face_row_start, int64_t total,
                                           int32_t* face_neighbours, void* stream) {
  if (n > kMaxItems || m > kMaxItems || total > kMaxTotal) return SURF_E_LIMIT;
  if (n < 0 || m < 0 || total < 0) return SURF_E_ARG;
  if (n == 0 || m == 0 || total == 0) return 0;
  if (!faces || !corner_order || !corner_start || !face_row_start || !face_neighbours) return SURF_E_ARG;
  hipLaunchKernelGGL(neighbour_emit_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, faces, m, n, corner_order,
                     corner_start, face_row_start, total, face_neighbours);
  return surf_check_launch();
}

extern "C" int surf_denoise_normal_step(const float* records_in, float* records_out, int64_t m, const int32_t* face_row_start,
                                        const int32_t* face_neighbours, int64_t total, double inv_s, double inv_r, void* stream) {
  if (m > kMaxItems || total > kMaxTotal) return SURF_E_LIMIT;
  if (m < 0 || total < 0 || !finite_f64(inv_s) || !finite_f64(inv_r) || inv_s < 0.0 || inv_r < 0.0) return SURF_E_ARG;
  if (m == 0) return 0;
  if (!records_in || !records_out || records_in == records_out || !face_row_start || (total > 0 && !face_neighbours))
    return SURF_E_ARG;
  hipLaunchKernelGGL(normal_step_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)records_in,
                     (f32x4*)records_out, m, face_row_start, face_neighbours, (int32_t)total, inv_s, inv_r);
  return surf_check_launch();
}

extern "C" int surf_denoise_vertex_step(const float* positions_in, float* positions_out, int64_t n, const int32_t* faces, int64_t m,
                                        const float* records, const int64_t* corner_order, const int64_t* corner_start,
                                        const uint8_t* boundary, int pin_boundary, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (n == 0) return 0;
  if (!positions_in || !positions_out || positions_in == positions_out || !corner_start || !boundary ||
      (m > 0 && (!faces || !records || !corner_order)))
    return SURF_E_ARG;
  hipLaunchKernelGGL(vertex_step_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)positions_in,
                     (f32x4*)positions_out, n, faces, m, (const f32x4*)records, corner_order, corner_start, boundary,
                     pin_boundary ? 1 : 0);
  return surf_check_launch();
}
