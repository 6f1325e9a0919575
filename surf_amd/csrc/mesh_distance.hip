// The exact distance from a point to a triangle mesh on the device (surf_amd/mesh_distance.py, backend="device"): per query the
// least point-to-triangle distance over ALL faces, the smallest face index that attains it and the closest point on that face.
//
// THE RULE is written once, in include/surf_hip.h above the surf_meshdist_* entry points; surf_amd/mesh_distance.py's host path
// mirrors it operation for operation in numpy fp64, and the arrays of the two paths are equal.  What this file adds:
//  * All arithmetic is fp64 on fp32 coordinates; the library is compiled with -ffp-contract=off, so every operator below is one
//    IEEE operation, and fp64 division and sqrt are correctly rounded on gfx950 as they are in numpy.
//  * THE TABLE: pairs_count_kernel writes one 48-byte record per face (its corners and its index) and counts the cells its box
//    overlaps; after the caller's scan pairs_emit_kernel lists the face under each of them; the caller sorts the list by cell and
//    gathers the records into that order.  No atomics of any kind, so the table is the same on every run.
//  * THE QUERY (the hot path), one query per lane.  The walk is surf_nearest_kernel<true>'s (nearest_shell.h): shells of cells
//    around the query's cell until the best squared distance is STRICTLY inside the visited reach.  A cell's records are
//    consecutive and a record is three 16-byte loads; the caller hands the queries over sorted by cell, so the lanes of a
//    wavefront mostly stand in the same few cells and their loads fall on the same lines.  The pair rule costs about 110 fp64
//    operations; its one division is taken in the region's own branch, and the square root once after the walk.
//    A face is evaluated again in every cell that lists it: the result is a minimum, so repeats change nothing, and the pair
//    budget of the header keeps them few.
//  * Compulsory bytes of the query kernel: 12 (point) + 8 (order) in and 8 + 8 + 24 out per query, and every record once, 48 per
//    pair.  Measured on an MI355X (scripts/time_mesh_distance.py, profiles/mesh_distance.txt), 299 k queries against 589 k faces:
//    1.3 ms, 240 pairs evaluated per query, about a hundred times the copy-rate time of those bytes: the kernel is fp64
//    arithmetic, not a copy.  The point-to-point search over the same vertex sets takes 0.16 ms.
// 256 threads per block.  Offline tool, not part of the training / render hot path.
#include <math.h>

#include "common.h"

namespace {

constexpr int64_t kMaxItems = 2147483647;
constexpr int64_t kMaxAxis = SURF_MESHDIST_MAX_AXIS_CELLS;
constexpr int64_t kMaxCells = SURF_MESHDIST_MAX_CELLS;

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

struct Table {
  double lo[3], cell;
  int64_t nc[3];
};

__device__ __forceinline__ double dot3(const double (&u)[3], const double (&v)[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

// The pair value of the header: q, and c* in cs.
__device__ __forceinline__ double pair_value(const double (&p)[3], const double (&a)[3], const double (&b)[3], const double (&c)[3],
                                             double (&cs)[3]) {
  double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = b[k] - a[k];
    ac[k] = c[k] - a[k];
    ap[k] = p[k] - a[k];
    bp[k] = p[k] - b[k];
    cp[k] = p[k] - c[k];
  }
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e1 = d4 - d3, e2 = d5 - d6;
  if (d1 <= 0.0 && d2 <= 0.0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = a[k];
  } else if (d3 >= 0.0 && d4 <= d3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = b[k];
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && d1 > d3) {
    const double t = d1 / (d1 - d3);
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = a[k] + ab[k] * t;
  } else if (d6 >= 0.0 && d5 <= d6) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = c[k];
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double t = d2 / (d2 - d6);
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = a[k] + ac[k] * t;
  } else if (va <= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
    const double t = e1 / (e1 + e2);
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = b[k] + (c[k] - b[k]) * t;
  } else {
    const double den = 1.0 / ((va + vb) + vc);
    const double v = vb * den, w = vc * den;
#pragma unroll
    for (int k = 0; k < 3; ++k) cs[k] = (a[k] + ab[k] * v) + ac[k] * w;
  }
  const double e[3] = {p[0] - cs[0], p[1] - cs[1], p[2] - cs[2]};
  return dot3(e, e);
}

// The cells [c0, c1] per axis that the box of a record's corners overlaps, clamped to the table.
__device__ __forceinline__ void record_cells(const f32x4 r0, const f32x4 r1, const f32x4 r2, const Table& g, int64_t (&c0)[3],
                                             int64_t (&c1)[3]) {
  const float x[3][3] = {{r0[0], r0[3], r1[2]}, {r0[1], r1[0], r1[3]}, {r0[2], r1[1], r2[0]}};      // per axis: a, b, c
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mn = (double)fminf(fminf(x[k][0], x[k][1]), x[k][2]), mx = (double)fmaxf(fmaxf(x[k][0], x[k][1]), x[k][2]);
    const double top = (double)(g.nc[k] - 1);
    c0[k] = (int64_t)fmin(fmax(floor((mn - g.lo[k]) / g.cell), 0.0), top);
    c1[k] = (int64_t)fmin(fmax(floor((mx - g.lo[k]) / g.cell), 0.0), top);
  }
}

__global__ __launch_bounds__(256) void pairs_count_kernel(const float* __restrict__ V, int64_t n, const int32_t* __restrict__ faces,
                                                          int64_t m, Table g, f32x4* __restrict__ records,
                                                          int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
  f32x4 r0 = {0.f, 0.f, 0.f, 0.f}, r1 = r0, r2 = r0;
  int64_t count = 0;
  if (i0 >= 0 && i0 < n && i1 >= 0 && i1 < n && i2 >= 0 && i2 < n) {
    r0 = f32x4{V[i0 * 3 + 0], V[i0 * 3 + 1], V[i0 * 3 + 2], V[i1 * 3 + 0]};
    r1 = f32x4{V[i1 * 3 + 1], V[i1 * 3 + 2], V[i2 * 3 + 0], V[i2 * 3 + 1]};
    r2 = f32x4{V[i2 * 3 + 2], __int_as_float((int32_t)f), 0.f, 0.f};
    int64_t c0[3], c1[3];
    record_cells(r0, r1, r2, g, c0, c1);
    count = (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  }
  records[f * 3 + 0] = r0;
  records[f * 3 + 1] = r1;
  records[f * 3 + 2] = r2;
  counts[f] = count;
}

__global__ __launch_bounds__(256) void pairs_emit_kernel(const f32x4* __restrict__ records, int64_t m, Table g,
                                                         const int64_t* __restrict__ starts, int64_t pairs,
                                                         int64_t* __restrict__ pair_cell, int32_t* __restrict__ pair_face) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m) return;
  const int64_t begin = starts[f], end = f + 1 < m ? starts[f + 1] : pairs;      // the face's part of the list, by the caller's scan
  if (begin < 0 || end > pairs || begin >= end) return;
  int64_t c0[3], c1[3];
  record_cells(records[f * 3 + 0], records[f * 3 + 1], records[f * 3 + 2], g, c0, c1);
  int64_t at = begin;
  for (int64_t x = c0[0]; x <= c1[0]; ++x)
    for (int64_t y = c0[1]; y <= c1[1]; ++y)
      for (int64_t z = c0[2]; z <= c1[2]; ++z) {
        if (at >= end) return;                                       // never taken with the caller's scan: a bounds guard only
        pair_cell[at] = (x * g.nc[1] + y) * g.nc[2] + z;
        pair_face[at] = (int32_t)f;
        ++at;
      }
}

__global__ __launch_bounds__(256) void query_kernel(const float* __restrict__ points, const int64_t* __restrict__ order, int64_t nq,
                                                    const f32x4* __restrict__ records, int64_t pairs,
                                                    const int32_t* __restrict__ cstart, Table g, double max_dist,
                                                    double* __restrict__ distance, int64_t* __restrict__ face,
                                                    double* __restrict__ closest) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const int64_t q = order[t];
  if (q < 0 || q >= nq) return;                                      // never taken with a permutation: a bounds guard only
  const double p[3] = {(double)points[q * 3 + 0], (double)points[q * 3 + 1], (double)points[q * 3 + 2]};
  // shells beyond kmax lie farther than max_dist (with a margin for the rounding of the cell coordinates)
  const double kmaxd = ceil(max_dist / (g.cell * (1.0 - 1e-6))) + 1.0;
  // Cell coordinates are kept within +-kFar cells of the table.  A query farther out than that (and still within max_dist) is
  // walked as if it stood there: the reach is then understated, which only delays the stop, and the walk ends at the shell
  // that takes in the last cell of the table, after which every face has been seen.
  constexpr double kFar = 1099511627776.0;                           // 2^40
  int64_t c[3];
  int64_t gap = 0;                                                   // Chebyshev distance in cells from the query's cell to the table
  int64_t kall = 0;                                                  // the shell that takes in the table's last cell
  bool far = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor((p[k] - g.lo[k]) / g.cell);
    const double away = f < 0.0 ? -f : f - (double)(g.nc[k] - 1);
    if (!(away <= kmaxd)) far = true;                                // far outside (or NaN): nothing within max_dist
    c[k] = far ? 0 : (int64_t)fmin(fmax(f, -kFar), kFar);
    gap = max(gap, c[k] < 0 ? -c[k] : max(c[k] - (g.nc[k] - 1), (int64_t)0));
    kall = max(kall, max(c[k], g.nc[k] - 1 - c[k]));
  }
  const int64_t kmax = min((int64_t)fmin(kmaxd, 4.0 * kFar), kall);
  double best = INFINITY, bc[3] = {INFINITY, INFINITY, INFINITY};
  int32_t besti = INT32_MAX;
  const int64_t zlo = 0, zhi = g.nc[2] - 1;
  for (int64_t k = gap; k <= kmax && !far; ++k) {
    // shells 0 .. k-1 are visited (those below `gap` miss the table): every face not yet seen lies more than k-1 cells away.
    // Stop once the best is STRICTLY within that reach, or the reach is max_dist.
    const double reach = (double)(k > 0 ? k - 1 : 0) * g.cell * (1.0 - 1e-6);
    if (best < reach * reach || reach >= max_dist) break;
    const int64_t x0 = max(c[0] - k, (int64_t)0), x1 = min(c[0] + k, g.nc[0] - 1);
    const int64_t y0 = max(c[1] - k, (int64_t)0), y1 = min(c[1] + k, g.nc[1] - 1);
    // A query far outside the table sees a shell whose z faces (and perhaps y faces) miss the table altogether: then only the
    // columns on the rim of the x-y square (only its two x sides) can hold cells of the shell, and the sweep goes over those alone.
    const bool zfaces = k == 0 || c[2] - k >= zlo || c[2] + k <= zhi;
    const bool yfaces = c[1] - k >= 0 || c[1] + k <= g.nc[1] - 1;
    const int64_t xstep = zfaces || yfaces ? 1 : 2 * k;
    for (int64_t x = xstep == 1 ? x0 : c[0] - k; x <= x1; x += xstep) {
      if (x < x0) continue;
      const int64_t ystep = zfaces || x == c[0] - k || x == c[0] + k ? 1 : 2 * k;
      for (int64_t y = ystep == 1 ? y0 : c[1] - k; y <= y1; y += ystep) {
        if (y < y0) continue;
        // on the rim of the shell's x-y square the whole z column belongs to the shell, inside it only the two z faces
        const bool rim = x == c[0] - k || x == c[0] + k || y == c[1] - k || y == c[1] + k;
        const int64_t z0 = rim ? max(c[2] - k, zlo) : c[2] - k, z1 = rim ? min(c[2] + k, zhi) : c[2] + k;
        for (int64_t z = z0; z <= z1; z += rim || k == 0 ? 1 : 2 * k) {
          if (z < zlo || z > zhi) continue;
          const int64_t cell = (x * g.nc[1] + y) * g.nc[2] + z;
          const int64_t sb = max((int64_t)cstart[cell], (int64_t)0), se = min((int64_t)cstart[cell + 1], pairs);
          for (int64_t s = sb; s < se; ++s) {
            const f32x4 r0 = records[s * 3 + 0], r1 = records[s * 3 + 1], r2 = records[s * 3 + 2];
            const double a[3] = {(double)r0[0], (double)r0[1], (double)r0[2]};
            const double b[3] = {(double)r0[3], (double)r1[0], (double)r1[1]};
            const double cc[3] = {(double)r1[2], (double)r1[3], (double)r2[0]};
            const int32_t j = __float_as_int(r2[1]);
            double cs[3];
            const double d = pair_value(p, a, b, cc, cs);
            if (d < best || (d == best && j < besti)) {               // false for a NaN d
              best = d;
              besti = j;
              bc[0] = cs[0];
              bc[1] = cs[1];
              bc[2] = cs[2];
            }
          }
        }
      }
    }
  }
  const double d = sqrt(best);
  const bool near = d < max_dist;
  distance[q] = near ? d : INFINITY;
  face[q] = near ? (int64_t)besti : -1;
  closest[q * 3 + 0] = near ? bc[0] : INFINITY;
  closest[q * 3 + 1] = near ? bc[1] : INFINITY;
  closest[q * 3 + 2] = near ? bc[2] : INFINITY;
}

inline bool finite_f64(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// 0, or the status that refuses the table's parameters
inline int check_table(double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, Table& g) {
  if (!finite_f64(lo_x) || !finite_f64(lo_y) || !finite_f64(lo_z) || !finite_f64(cell) || !(cell > 0.0)) return SURF_E_ARG;
  if (nx < 1 || ny < 1 || nz < 1) return SURF_E_ARG;
  if (nx > kMaxAxis || ny > kMaxAxis || nz > kMaxAxis || nx * ny * nz > kMaxCells) return SURF_E_LIMIT;
  g = Table{{lo_x, lo_y, lo_z}, cell, {nx, ny, nz}};
  return 0;
}

}  // namespace

extern "C" int surf_meshdist_pairs_count(const float* vertices, int64_t n, const int32_t* faces, int64_t m, double lo_x, double lo_y,
                                         double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, float* records,
                                         int64_t* counts, void* stream) {
  if (n > kMaxItems || m > kMaxItems) return SURF_E_LIMIT;
  if (n < 0 || m < 0) return SURF_E_ARG;
  if (m == 0) return 0;
  Table g;
  if (const int bad = check_table(lo_x, lo_y, lo_z, cell, nx, ny, nz, g)) return bad;
  if (!vertices || !faces || !records || !counts) return SURF_E_ARG;
  hipLaunchKernelGGL(pairs_count_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, vertices, n, faces, m, g, (f32x4*)records,
                     counts);
  return surf_check_launch();
}

extern "C" int surf_meshdist_pairs_emit(const float* records, int64_t m, double lo_x, double lo_y, double lo_z, double cell,
                                        int64_t nx, int64_t ny, int64_t nz, const int64_t* starts, int64_t pairs, int64_t* pair_cell,
                                        int32_t* pair_face, void* stream) {
  if (m > kMaxItems || pairs > kMaxItems) return SURF_E_LIMIT;
  if (m < 0 || pairs < 0) return SURF_E_ARG;
  if (m == 0 || pairs == 0) return 0;
  Table g;
  if (const int bad = check_table(lo_x, lo_y, lo_z, cell, nx, ny, nz, g)) return bad;
  if (!records || !starts || !pair_cell || !pair_face) return SURF_E_ARG;
  hipLaunchKernelGGL(pairs_emit_kernel, dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)records, m, g, starts, pairs,
                     pair_cell, pair_face);
  return surf_check_launch();
}

extern "C" int surf_meshdist_query(const float* points, const int64_t* order, int64_t k, const float* cell_records, int64_t pairs,
                                   const int32_t* cell_start, double lo_x, double lo_y, double lo_z, double cell, int64_t nx,
                                   int64_t ny, int64_t nz, double max_dist, double* distance, int64_t* face, double* closest,
                                   void* stream) {
  if (k > kMaxItems || pairs > kMaxItems) return SURF_E_LIMIT;
  if (k < 0 || pairs < 0 || !finite_f64(max_dist) || !(max_dist > 0.0)) return SURF_E_ARG;
  if (k == 0) return 0;
  Table g;
  if (const int bad = check_table(lo_x, lo_y, lo_z, cell, nx, ny, nz, g)) return bad;
  if (!points || !order || !cell_start || !distance || !face || !closest || (pairs > 0 && !cell_records)) return SURF_E_ARG;
  hipLaunchKernelGGL(query_kernel, dim3(blocks(k)), dim3(256), 0, (hipStream_t)stream, points, order, k, (const f32x4*)cell_records,
                     pairs, cell_start, g, max_dist, distance, face, closest);
  return surf_check_launch();
}
