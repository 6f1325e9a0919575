// Point-cloud clean-up (surf_amd/point_filter.py, backend="device"): the k nearest neighbours of every point of a cloud within the
// cloud itself, the outlier statistic and the normals taken from them.  The rule is written once, above the surf_points_knn*
// entry points of include/surf_hip.h (rules 1-5); in short:
//  * neighbours: dx = P[j].x - P[i].x ..., d2 = (dx*dx + dy*dy) + dz*dz in fp32, admitted iff d2 <= md2 = max_dist * max_dist (fp32,
//    from the host); only the index i itself is excluded; a non-finite point neither has nor is a neighbour; the list is the
//    first k admitted candidates in ascending (d2, j) order.
//  * statistic: the fp32 sum of sqrtf(d2_m) in list order over (float)k, +inf unless count == k.
//  * normals: fp64 S1 / S2 sums of the fp32 offsets in list order, covariance with the point itself counted, a fixed number of
//    cyclic Jacobi sweeps (+ - * / sqrt only), the column of the smallest diagonal entry, oriented to the centre of the point's
//    view; one rounding to fp32.
//  * statistic sums: the fixed-slot partial sums of slot_sums.h, which fscore.hip's ICP reductions use too; no float atomics.
//
// The search structure is dtu_eval.hip's / fscore.hip's: a dense cell table (the caller sorts the keys and scans the counts), the
// points permuted into cell order, ridx = their index in the caller's order so that the tie rule speaks the caller's indices.
// One thread per query IN CELL ORDER: neighbouring lanes walk neighbouring cells and share their cache lines.  Shells of cells
// r = 0, 1, ... around the query's own cell are walked.  Before shell r (r >= 2) every unvisited point lies at least (r - 1) cells
// away; with R2 = ((r - 1) * cell * (1 - 1e-5))^2 (the factor covers the rounding of d2 in fp32, 5 * 2^-24 relative, and that of
// the cell coordinates in fp64) every unvisited point has d2 > R2, so the walk stops when the list is full and its last d2 is
// STRICTLY below R2 - an unvisited point can then neither beat nor tie an entry, whatever its index - or when R2 > md2 (no
// unvisited point is admitted: this bounds the work of an isolated outlier), or when the shell has left the grid.
//
// The k-slot list.  A per-thread array indexed by a run-time position lives in scratch; the list is kept in LDS instead, one
// column per lane (slot m of lane l at word m * 64 + l: a wavefront's access to one slot is 512 contiguous bytes, free of bank
// conflicts for 8-byte accesses).  A slot is ONE 64-bit word, d2's bits above the index: d2 >= +0 and finite, so unsigned integer
// order on the word is the (d2, j) order and an insertion is a run of 8-byte moves.  Workgroups are one wavefront (64 threads,
// k * 512 B of LDS, 16 KB at k = 32): no barrier is needed, and a wavefront that drew a long walk holds up no other.
// surf_points_knn writes the lists out; surf_points_knn_reduce reads them out of LDS for the statistic and the normals and
// never writes them (at 10 M points and k = 16 they would be 1.3 GB).
#include <math.h>

#include "common.h"
#include "slot_sums.h"         // block_partial, slot_finish_kernel, slots_for, shared with fscore.hip

namespace {

constexpr int kLanes = 64;                                   // threads of a search workgroup = columns of its LDS list
constexpr int kMaxK = SURF_POINTS_KNN_MAX_K;
constexpr int kSlots = SURF_POINTS_STAT_SLOTS;
constexpr double kShrink = 1.0 - 1e-5;                       // see the stop test above

struct Grid {
  double lo[3], cell;
  int nc[3];
};

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cell coordinate of a FINITE value: the key kernel and the search must agree, so both call this
__device__ __forceinline__ int cell_coord(float p, double lo, double cell, int nc) {
  const double f = floor(((double)p - lo) / cell);
  return (int)fmin(fmax(f, 0.0), (double)(nc - 1));
}

__global__ __launch_bounds__(256) void knn_keys_kernel(const float* __restrict__ P, int64_t n, Grid g, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
  if (!finite3(x, y, z)) {
    keys[i] = (int64_t)g.nc[0] * g.nc[1] * g.nc[2];
    return;
  }
  const int64_t cx = cell_coord(x, g.lo[0], g.cell, g.nc[0]), cy = cell_coord(y, g.lo[1], g.cell, g.nc[1]);
  keys[i] = (cx * g.nc[1] + cy) * g.nc[2] + cell_coord(z, g.lo[2], g.cell, g.nc[2]);
}

struct SearchArgs {
  const float* spts;       // (n, 3) points in cell order
  const int32_t* ridx;     // (n) their index in the caller's order
  const int32_t* cstart;   // (cells + 1) first row of every cell; cstart[cells] = the number of finite points
  int64_t n;
  Grid g;
  int k;
  float md2;
};

__device__ __forceinline__ float slot_d2(uint64_t w) { return __uint_as_float((uint32_t)(w >> 32)); }
__device__ __forceinline__ int32_t slot_index(uint64_t w) { return (int32_t)(uint32_t)(w & 0xffffffffu); }

// The neighbour list of sorted row t (a finite point) into L[m * kLanes], m = 0 .. count - 1, ascending; returns count.
__device__ __forceinline__ int knn_search(const SearchArgs& a, int32_t t, uint64_t* __restrict__ L) {
  const float px = a.spts[(int64_t)t * 3 + 0], py = a.spts[(int64_t)t * 3 + 1], pz = a.spts[(int64_t)t * 3 + 2];
  const int nc0 = a.g.nc[0], nc1 = a.g.nc[1], nc2 = a.g.nc[2];
  const int c0 = cell_coord(px, a.g.lo[0], a.g.cell, nc0), c1 = cell_coord(py, a.g.lo[1], a.g.cell, nc1),
            c2 = cell_coord(pz, a.g.lo[2], a.g.cell, nc2);
  const int rgrid = max(max(max(c0, nc0 - 1 - c0), max(c1, nc1 - 1 - c1)), max(c2, nc2 - 1 - c2));   // the last shell inside the grid
  const int k = a.k;
  const double md2 = (double)a.md2;
  int cnt = 0;
  uint64_t worst = ~uint64_t(0);       // the list's last word once it is full: a candidate enters iff its word is smaller
  float wd2 = INFINITY;                // its d2
  for (int r = 0; r <= rgrid; ++r) {
    if (r > 1) {
      const double reach = (double)(r - 1) * a.g.cell * kShrink;
      const double R2 = reach * reach;
      if ((double)wd2 < R2 || R2 > md2) break;
    }
    const int x0 = max(c0 - r, 0), x1 = min(c0 + r, nc0 - 1);
    const int y0 = max(c1 - r, 0), y1 = min(c1 + r, nc1 - 1);
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) {
        // on the rim of the shell's x-y square the whole z column belongs to the shell, inside it only the two z faces
        const bool rim = x == c0 - r || x == c0 + r || y == c1 - r || y == c1 + r;
        const int z0 = rim ? max(c2 - r, 0) : c2 - r, z1 = rim ? min(c2 + r, nc2 - 1) : c2 + r;
        for (int z = z0; z <= z1; z += (rim || r == 0) ? 1 : 2 * r) {
          if (z < 0 || z > nc2 - 1) continue;
          const int64_t cell = ((int64_t)x * nc1 + y) * nc2 + z;
          const int32_t e = a.cstart[cell + 1];
          for (int32_t s = a.cstart[cell]; s < e; ++s) {
            if (s == t) continue;                                     // only the query's own index is excluded
            const float dx = a.spts[(int64_t)s * 3 + 0] - px, dy = a.spts[(int64_t)s * 3 + 1] - py, dz = a.spts[(int64_t)s * 3 + 2] - pz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= a.md2) || d2 > wd2) continue;
            const uint64_t w = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)a.ridx[s];
            if (!(w < worst)) continue;
            int m = cnt < k ? cnt : k - 1;                            // the slot that opens (or the last one, which falls out)
            while (m > 0) {
              const uint64_t prev = L[(m - 1) * kLanes];
              if (prev < w) break;
              L[m * kLanes] = prev;
              --m;
            }
            L[m * kLanes] = w;
            if (cnt < k) ++cnt;
            if (cnt == k) {
              worst = L[(k - 1) * kLanes];
              wd2 = slot_d2(worst);
            }
          }
        }
      }
  }
  return cnt;
}

__global__ __launch_bounds__(kLanes) void knn_lists_kernel(SearchArgs a, int32_t* __restrict__ index, float* __restrict__ d2,
                                                           int32_t* __restrict__ count) {
  extern __shared__ uint64_t knn_lds[];
  const int64_t t = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (t >= a.n) return;
  const int32_t i = a.ridx[t];
  if (i < 0 || i >= a.n) return;
  uint64_t* L = knn_lds + threadIdx.x;
  const int64_t cells = (int64_t)a.g.nc[0] * a.g.nc[1] * a.g.nc[2];
  const int cnt = t < a.cstart[cells] ? knn_search(a, (int32_t)t, L) : 0;
  for (int m = 0; m < a.k; ++m) {
    const uint64_t w = m < cnt ? L[m * kLanes] : 0;
    index[(int64_t)i * a.k + m] = m < cnt ? slot_index(w) : -1;
    d2[(int64_t)i * a.k + m] = m < cnt ? slot_d2(w) : INFINITY;
  }
  count[i] = cnt;
}

// one Jacobi rotation of rule 5 in the (p, q) plane; (arp, arq) are the two entries of the third row / column
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq != 0.0) {
    const double theta = (aqq - app) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
    v0p = c * a0 - s * b0;
    v0q = s * a0 + c * b0;
    v1p = c * a1 - s * b1;
    v1q = s * a1 + c * b1;
    v2p = c * a2 - s * b2;
    v2q = s * a2 + c * b2;
  }
}

struct ReduceArgs {
  const float* pts;        // (n, 3) points in the caller's order
  const int32_t* view;     // (n) view of every point, or null
  const double* centres;   // (n_views, 3), or null
  int n_views;
  float* stat;             // (n)
  int32_t* count;          // (n)
  float* normal;           // (n, 3), or null
};

__global__ __launch_bounds__(kLanes) void knn_reduce_kernel(SearchArgs a, ReduceArgs o) {
  extern __shared__ uint64_t knn_lds[];
  const int64_t t = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  if (t >= a.n) return;
  const int32_t i = a.ridx[t];
  if (i < 0 || i >= a.n) return;
  uint64_t* L = knn_lds + threadIdx.x;
  const int64_t cells = (int64_t)a.g.nc[0] * a.g.nc[1] * a.g.nc[2];
  const int cnt = t < a.cstart[cells] ? knn_search(a, (int32_t)t, L) : 0;
  float sum = 0.0f;
  for (int m = 0; m < cnt; ++m) sum += sqrtf(slot_d2(L[m * kLanes]));
  o.stat[i] = cnt == a.k ? sum / (float)a.k : INFINITY;
  o.count[i] = cnt;
  if (!o.normal) return;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (cnt >= 2) {
    const float px = a.spts[t * 3 + 0], py = a.spts[t * 3 + 1], pz = a.spts[t * 3 + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, q00 = 0.0, q01 = 0.0, q02 = 0.0, q11 = 0.0, q12 = 0.0, q22 = 0.0;
    for (int m = 0; m < cnt; ++m) {
      const int32_t j = slot_index(L[m * kLanes]);
      if (j < 0 || j >= a.n) continue;                                // cannot happen with a well-formed sorted_index
      const double ex = (double)(o.pts[(int64_t)j * 3 + 0] - px), ey = (double)(o.pts[(int64_t)j * 3 + 1] - py),
                   ez = (double)(o.pts[(int64_t)j * 3 + 2] - pz);
      s0 += ex;
      s1 += ey;
      s2 += ez;
      q00 += ex * ex;
      q01 += ex * ey;
      q02 += ex * ez;
      q11 += ey * ey;
      q12 += ey * ez;
      q22 += ez * ez;
    }
    const double mm = (double)(cnt + 1);
    const double m0 = s0 / mm, m1 = s1 / mm, m2 = s2 / mm;
    double a00 = q00 / mm - m0 * m0, a01 = q01 / mm - m0 * m1, a02 = q02 / mm - m0 * m2, a11 = q11 / mm - m1 * m1,
           a12 = q12 / mm - m1 * m2, a22 = q22 / mm - m2 * m2;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < SURF_POINTS_NORMAL_SWEEPS; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0, 1), r = 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2), r = 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2), r = 0
    }
    // the column of the smallest diagonal entry, the lowest on ties (selects: a run-time column index would go through scratch)
    const bool g1 = a11 < a00;
    const bool g2 = a22 < (g1 ? a11 : a00);
    double x = g2 ? v02 : (g1 ? v01 : v00), y = g2 ? v12 : (g1 ? v11 : v10), z = g2 ? v22 : (g1 ? v21 : v20);
    const double len = sqrt((x * x + y * y) + z * z);
    x = x / len;
    y = y / len;
    z = z / len;
    double d = 0.0;
    if (o.view && o.centres) {
      const int32_t v = o.view[i];
      if (v >= 0 && v < o.n_views)
        d = (x * (o.centres[(int64_t)v * 3 + 0] - (double)px) + y * (o.centres[(int64_t)v * 3 + 1] - (double)py)) +
            z * (o.centres[(int64_t)v * 3 + 2] - (double)pz);
    }
    bool flip = d < 0.0;
    if (d == 0.0) {
      double big = x;
      if (fabs(y) > fabs(big)) big = y;
      if (fabs(z) > fabs(big)) big = z;
      flip = big < 0.0;
    }
    if (flip) {
      x = -x;
      y = -y;
      z = -z;
    }
    if (isfinite(x) && isfinite(y) && isfinite(z) && !(d != d)) {
      nx = (float)x;
      ny = (float)y;
      nz = (float)z;
    }
  }
  o.normal[(int64_t)i * 3 + 0] = nx;
  o.normal[(int64_t)i * 3 + 1] = ny;
  o.normal[(int64_t)i * 3 + 2] = nz;
}

// ---- rule 3's sums: [number, sum, sum of squares] of the finite statistics, in fixed slots (slot_sums.h) ----

__global__ __launch_bounds__(256) void stat_sums_kernel(const float* __restrict__ stat, int64_t n, double* __restrict__ part) {
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = stat[i];
    if (!isfinite(s)) continue;
    const double v = (double)s;
    acc[0] += 1.0;
    acc[1] += v;
    acc[2] += v * v;
  }
  block_partial<3>(acc, part);
}

// the checks every entry point over the table shares; 0 or a status
int check_table(int64_t n, double cell, int64_t nx, int64_t ny, int64_t nz) {
  if (!(cell > 0.0) || !(cell < INFINITY) || nx <= 0 || ny <= 0 || nz <= 0) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  const int64_t cap = SURF_POINTS_KNN_MAX_CELLS;
  if (nx > cap || ny > cap || nz > cap || nx * ny > cap || nx * ny * nz > cap) return SURF_E_LIMIT;
  return 0;
}

int check_search(int k, float max_dist, float* md2) {
  if (k < 1 || k > kMaxK) return SURF_E_ARG;
  if (!(max_dist > 0.0f) || !(max_dist < INFINITY)) return SURF_E_ARG;
  *md2 = max_dist * max_dist;
  if (!(*md2 > 0.0f) || !(*md2 < INFINITY)) return SURF_E_ARG;
  return 0;
}

}  // namespace

extern "C" int surf_points_knn_keys(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double cell, int64_t nx,
                                    int64_t ny, int64_t nz, int64_t* keys, void* stream) {
  if (n == 0) return 0;
  if (!points || !keys || n < 0 || !isfinite(lo_x) || !isfinite(lo_y) || !isfinite(lo_z)) return SURF_E_ARG;
  if (const int st = check_table(n, cell, nx, ny, nz)) return st;
  const Grid g{{lo_x, lo_y, lo_z}, cell, {(int)nx, (int)ny, (int)nz}};
  hipLaunchKernelGGL(knn_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, n, g, keys);
  return surf_check_launch();
}

extern "C" int surf_points_knn(const float* sorted_points, const int32_t* sorted_index, const int32_t* cell_start, int64_t n,
                               double lo_x, double lo_y, double lo_z, double cell, int64_t nx, int64_t ny, int64_t nz, int k,
                               float max_dist, int32_t* index, float* d2, int32_t* count, void* stream) {
  if (n == 0) return 0;
  float md2;
  if (const int st = check_search(k, max_dist, &md2)) return st;
  if (!sorted_points || !sorted_index || !cell_start || !index || !d2 || !count || n < 0 || !isfinite(lo_x) || !isfinite(lo_y) ||
      !isfinite(lo_z))
    return SURF_E_ARG;
  if (const int st = check_table(n, cell, nx, ny, nz)) return st;
  const SearchArgs a{sorted_points, sorted_index, cell_start, n, {{lo_x, lo_y, lo_z}, cell, {(int)nx, (int)ny, (int)nz}}, k, md2};
  hipLaunchKernelGGL(knn_lists_kernel, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), (size_t)k * kLanes * sizeof(uint64_t),
                     (hipStream_t)stream, a, index, d2, count);
  return surf_check_launch();
}

extern "C" int surf_points_knn_reduce(const float* points, const float* sorted_points, const int32_t* sorted_index,
                                      const int32_t* cell_start, int64_t n, double lo_x, double lo_y, double lo_z, double cell,
                                      int64_t nx, int64_t ny, int64_t nz, int k, float max_dist, const int32_t* view,
                                      const double* centres, int n_views, float* stat, int32_t* count, float* normal, void* stream) {
  if (n == 0) return 0;
  float md2;
  if (const int st = check_search(k, max_dist, &md2)) return st;
  if (!points || !sorted_points || !sorted_index || !cell_start || !stat || !count || n < 0 || !isfinite(lo_x) || !isfinite(lo_y) ||
      !isfinite(lo_z))
    return SURF_E_ARG;
  if ((view != nullptr) != (centres != nullptr) || (centres && n_views < 1) || (view && !normal)) return SURF_E_ARG;
  if (const int st = check_table(n, cell, nx, ny, nz)) return st;
  const SearchArgs a{sorted_points, sorted_index, cell_start, n, {{lo_x, lo_y, lo_z}, cell, {(int)nx, (int)ny, (int)nz}}, k, md2};
  const ReduceArgs o{points, view, centres, n_views, stat, count, normal};
  hipLaunchKernelGGL(knn_reduce_kernel, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), (size_t)k * kLanes * sizeof(uint64_t),
                     (hipStream_t)stream, a, o);
  return surf_check_launch();
}

extern "C" int surf_points_stat_sums(const float* stat, int64_t n, double* partials, double* out, void* stream) {
  if (!partials || !out || n < 0 || (n > 0 && !stat)) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  const int slots = slots_for(n, kSlots);                            // n == 0: no slots, the finish writes zeros
  if (slots) hipLaunchKernelGGL(stat_sums_kernel, dim3(slots), dim3(256), 0, (hipStream_t)stream, stat, n, partials);
  hipLaunchKernelGGL(slot_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, slots, 3, out);
  return surf_check_launch();
}
