// The capped nearest-neighbour search over a dense cell table, ONE copy for dtu_eval.hip (distance only: scikit-learn's kd-tree
// value, bit for bit) and fscore.hip (distance and WHICH reference point).  Shells of cells around the query's cell are walked
// until the best squared distance is within the shell radius or the shell radius reaches max_dist; +inf (and index -1) when
// nothing is nearer than max_dist.  The minimum of the fp64 squared distances (dx*dx + dy*dy) + dz*dz, then one sqrt.
#pragma once
#include <math.h>

#include "common.h"

constexpr int64_t kGridAxis = int64_t(1) << 21;   // cells per axis, at most: keys (x << 42) | (y << 21) | z

struct NearestArgs {
  const double* q;         // (m, 3) queries
  int64_t m;
  const double* ref;       // (r, 3) reference points in cell order
  const int32_t* cstart;   // (nx*ny*nz + 1) first point of every cell
  double lo[3], cell, max_dist;
  int64_t nc[3];
  double* out;             // (m) distance, +inf where >= max_dist
};
struct NearestIndexArgs {
  const double* q;
  int64_t m;
  const double* ref;
  const int32_t* ridx;     // (r) the reference points' index in the caller's order
  const int32_t* cstart;
  double lo[3], cell, max_dist;
  int64_t nc[3];
  double* out;
  int64_t* index;          // (m) index of the nearest reference point, -1 where the distance is +inf
};

// One thread per query; Args = NearestArgs (WITH_INDEX = false) or NearestIndexArgs (true).  With the index, equal squared
// distances go to the smaller index, so the walk may stop only once the best is STRICTLY within the visited reach (a point at
// exactly the reach could still tie with a smaller index); without it, a tie changes nothing and `<=` stops one shell earlier.
template <bool WITH_INDEX, class Args>
__global__ __launch_bounds__(256) void surf_nearest_kernel(Args a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.m) return;
  const double p[3] = {a.q[t * 3 + 0], a.q[t * 3 + 1], a.q[t * 3 + 2]};
  // shells beyond kmax lie farther than max_dist (with a margin for the rounding of the cell coordinates)
  const int64_t kmax = (int64_t)ceil(a.max_dist / (a.cell * (1.0 - 1e-6))) + 1;
  int64_t c[3];
  int64_t gap = 0;                           // Chebyshev distance in cells from the query's cell to the grid
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor((p[k] - a.lo[k]) / a.cell);
    const double g = f < 0.0 ? -f : f - (double)(a.nc[k] - 1);
    if (!(g <= (double)kmax)) {              // far outside (or NaN): nothing within max_dist
      a.out[t] = INFINITY;
      if constexpr (WITH_INDEX) a.index[t] = -1;
      return;
    }
    c[k] = (int64_t)f;
    gap = max(gap, (int64_t)max(g, 0.0));
  }
  const int64_t zlo = 0, zhi = a.nc[2] - 1;
  double best = INFINITY;
  int32_t besti = INT32_MAX;
  for (int64_t k = gap; k <= kmax; ++k) {
    // shells 0 .. k-1 are visited (those below `gap` miss the grid): every other point lies more than k-1 cells away.  Stop
    // once the best is within that reach, or the reach is max_dist.
    const double reach = (double)(k > 0 ? k - 1 : 0) * a.cell * (1.0 - 1e-6);
    if ((WITH_INDEX ? best < reach * reach : best <= reach * reach) || reach >= a.max_dist) break;
    const int64_t x0 = max(c[0] - k, (int64_t)0), x1 = min(c[0] + k, a.nc[0] - 1);
    const int64_t y0 = max(c[1] - k, (int64_t)0), y1 = min(c[1] + k, a.nc[1] - 1);
    for (int64_t x = x0; x <= x1; ++x)
      for (int64_t y = y0; y <= y1; ++y) {
        // on the rim of the shell's x-y square the whole z column belongs to the shell, inside it only the two z faces
        const bool rim = x == c[0] - k || x == c[0] + k || y == c[1] - k || y == c[1] + k;
        const int64_t z0 = rim ? max(c[2] - k, zlo) : c[2] - k, z1 = rim ? min(c[2] + k, zhi) : c[2] + k;
        for (int64_t z = z0; z <= z1; z += rim ? 1 : 2 * k) {
          if (z < zlo || z > zhi) continue;
          const int64_t cell = (x * a.nc[1] + y) * a.nc[2] + z;
          const int32_t e = a.cstart[cell + 1];
          for (int32_t s = a.cstart[cell]; s < e; ++s) {
            const double dx = p[0] - a.ref[(int64_t)s * 3 + 0], dy = p[1] - a.ref[(int64_t)s * 3 + 1], dz = p[2] - a.ref[(int64_t)s * 3 + 2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if constexpr (WITH_INDEX) {
              const int32_t j = a.ridx[s];
              if (d2 < best || (d2 == best && j < besti)) {
                best = d2;
                besti = j;
              }
            } else {
              best = fmin(best, d2);
            }
          }
        }
      }
  }
  const double d = sqrt(best);
  const bool near = d < a.max_dist;
  a.out[t] = near ? d : INFINITY;
  if constexpr (WITH_INDEX) a.index[t] = near ? (int64_t)besti : -1;
}
