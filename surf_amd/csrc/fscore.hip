// Tanks and Temples / ETH3D F-score evaluation on the device (surf_amd/evaluation/fscore.py, device="gpu"): rigid transform,
// polygon-volume crop, voxel mean, capped nearest neighbour WITH index and the two reductions of a point-to-point ICP step.
//
// All arithmetic is fp64 in the numpy path's operation order, and the library is compiled with -ffp-contract=off, so that the
// transform, the crop, the voxel means and the nearest distances / indices equal the host path's arrays:
//  * transform: p'[k] = ((R[k,0]*x + R[k,1]*y) + R[k,2]*z) + t[k].
//  * crop: axis_min <= p[a] <= axis_max and an odd crossing number over the polygon's edges (i, j = i - 1) in the plane (u, v) of
//    the two other axes: ((v_i > v) != (v_j > v)) and u < (u_j - u_i) * (v - v_i) / (v_j - v_i) + u_i.
//  * voxel mean: the members of a voxel are summed sequentially in input-index order (the caller's stable sort by cell key keeps
//    that order inside a segment), one thread per (voxel, coordinate); then sum / count.  A segment may be of any length.
//  * nearest: the shell walk of nearest_shell.h, which dtu_eval.hip runs too (the same shells over the same dense cell table, the
//    same (dx*dx + dy*dy) + dz*dz and one sqrt), here tracking the reference point's index in the caller's order as well; equal
//    squared distances go to the smaller index.
//  * ICP sums: the fixed-slot partial sums of slot_sums.h (the same bits on every run, no float atomics).  Pass 1: pair count, sum of source, sum of target, sum of d*d; pass 2: the CENTRED 3x3 cross-covariance.
// Offline evaluation: gather- and fp64-VALU bound, one item per thread, 256 threads.
#include <math.h>

#include "common.h"
#include "nearest_shell.h"     // the shell walk and kGridAxis, shared with dtu_eval.hip
#include "slot_sums.h"         // block_partial, slot_finish_kernel, slots_for, shared with point_knn.hip

namespace {

constexpr int kSlots = SURF_FSCORE_ICP_SLOTS;    // workgroups (= partial-sum slots) of an ICP reduction, at most

struct Rigid {
  double r[9], t[3];
};

__global__ __launch_bounds__(256) void transform_kernel(const double* __restrict__ P, int64_t n, Rigid T, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = ((T.r[k * 3 + 0] * x + T.r[k * 3 + 1] * y) + T.r[k * 3 + 2] * z) + T.t[k];
}

__global__ __launch_bounds__(256) void crop_kernel(const double* __restrict__ P, int64_t n, int axis, int ua, int va, double amin,
                                                   double amax, const double* __restrict__ poly, int n_poly,
                                                   uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = P[i * 3 + axis], u = P[i * 3 + ua], v = P[i * 3 + va];
  bool inside = false;
  for (int e = 0, j = n_poly - 1; e < n_poly; j = e++) {
    const double ui = poly[e * 2 + 0], vi = poly[e * 2 + 1], uj = poly[j * 2 + 0], vj = poly[j * 2 + 1];
    if (((vi > v) != (vj > v)) && u < (uj - ui) * (v - vi) / (vj - vi) + ui) inside = !inside;
  }
  keep[i] = (amin <= a && a <= amax && inside) ? 1 : 0;
}

__global__ __launch_bounds__(256) void voxel_keys_kernel(const double* __restrict__ P, int64_t n, double ox, double oy, double oz,
                                                         double voxel, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // the entry point has checked the box: the clamp only keeps a NaN or a point outside the stated box inside the key's fields
  const int64_t cx = min(max((int64_t)floor((P[i * 3 + 0] - ox) / voxel), (int64_t)0), kGridAxis - 1);
  const int64_t cy = min(max((int64_t)floor((P[i * 3 + 1] - oy) / voxel), (int64_t)0), kGridAxis - 1);
  const int64_t cz = min(max((int64_t)floor((P[i * 3 + 2] - oz) / voxel), (int64_t)0), kGridAxis - 1);
  keys[i] = (cx << 42) | (cy << 21) | cz;
}

// one thread per (voxel, coordinate): the members are added one after the other in sorted (= input-index) order
__global__ __launch_bounds__(256) void voxel_mean_kernel(const double* __restrict__ P, int64_t n, const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ seg, int64_t m, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * 3) return;
  const int64_t s = t / 3;
  const int k = (int)(t - s * 3);
  const int64_t b = max(seg[s], (int64_t)0), e = min(seg[s + 1], n);
  double acc = 0.0;
  for (int64_t q = b; q < e; ++q) {
    const int64_t i = order[q];
    if (i >= 0 && i < n) acc += P[i * 3 + k];
  }
  out[t] = acc / (double)(e - b);
}

// ---- the ICP reductions ----

struct PairArgs {
  const double* src;       // (n, 3) transformed source points
  const double* tgt;       // (r, 3) target points
  const int64_t* index;    // (n) nearest target of every source point, < 0: none
  const double* dist;      // (n) its distance
  int64_t n, r;
  double cs[3], ct[3];     // pass 2: the centroids of the paired source / target points
  double* part;            // (gridDim.x, K) partial sums
};

// pass 1: [pairs, sum sx, sy, sz, sum tx, ty, tz, sum d*d]
__global__ __launch_bounds__(256) void icp_sums_kernel(PairArgs a) {
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = a.index[i];
    if (j < 0 || j >= a.r) continue;
    const double d = a.dist[i];
    acc[0] += 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[1 + k] += a.src[i * 3 + k];
      acc[4 + k] += a.tgt[j * 3 + k];
    }
    acc[7] += d * d;
  }
  block_partial<8>(acc, a.part);
}

// pass 2: H[r][c] = sum (s[r] - cs[r]) * (t[c] - ct[c])
__global__ __launch_bounds__(256) void icp_cov_kernel(PairArgs a) {
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = a.index[i];
    if (j < 0 || j >= a.r) continue;
    double s[3], t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s[k] = a.src[i * 3 + k] - a.cs[k];
      t[k] = a.tgt[j * 3 + k] - a.ct[k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[r * 3 + c] += s[r] * t[c];
  }
  block_partial<9>(acc, a.part);
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int surf_fscore_transform(const double* points, int64_t n, const double* h_T, double* out, void* stream) {
  if (!points || !h_T || !out || n <= 0) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  Rigid T;
  for (int k = 0; k < 3; ++k) {
    for (int c = 0; c < 3; ++c) T.r[k * 3 + c] = h_T[k * 4 + c];
    T.t[k] = h_T[k * 4 + 3];
  }
  hipLaunchKernelGGL(transform_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, T, out);
  return surf_check_launch();
}

extern "C" int surf_fscore_crop(const double* points, int64_t n, int axis, double axis_min, double axis_max, const double* polygon,
                                int n_polygon, uint8_t* keep, void* stream) {
  if (!points || !polygon || !keep || n <= 0 || axis < 0 || axis > 2 || n_polygon < 3) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;
  hipLaunchKernelGGL(crop_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, axis, ua, va, axis_min, axis_max,
                     polygon, n_polygon, keep);
  return surf_check_launch();
}

extern "C" int surf_fscore_voxel_keys(const double* points, int64_t n, const double* h_lo, const double* h_hi, double voxel,
                                      int64_t* keys, void* stream) {
  if (!points || !h_lo || !h_hi || !keys || n <= 0 || !(voxel > 0.0)) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  double origin[3];
  for (int k = 0; k < 3; ++k) {
    if (!(h_lo[k] <= h_hi[k])) return SURF_E_ARG;                     // NaN included
    origin[k] = h_lo[k] - voxel / 2;
    if (!(floor((h_hi[k] - origin[k]) / voxel) < (double)kGridAxis)) return SURF_E_LIMIT;
  }
  hipLaunchKernelGGL(voxel_keys_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, points, n, origin[0], origin[1], origin[2],
                     voxel, keys);
  return surf_check_launch();
}

extern "C" int surf_fscore_voxel_mean(const double* points, int64_t n, const int64_t* order, const int64_t* segment_start,
                                      int64_t n_voxels, double* out, void* stream) {
  if (!points || !order || !segment_start || !out || n <= 0 || n_voxels <= 0 || n_voxels > n) return SURF_E_ARG;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  hipLaunchKernelGGL(voxel_mean_kernel, dim3(blocks(n_voxels * 3)), dim3(256), 0, (hipStream_t)stream, points, n, order, segment_start,
                     n_voxels, out);
  return surf_check_launch();
}

extern "C" int surf_fscore_nearest(const double* queries, int64_t m, const double* sorted_ref, const int32_t* sorted_index,
                                   const int32_t* cell_start, double lo_x, double lo_y, double lo_z, double cell, int64_t nx,
                                   int64_t ny, int64_t nz, double max_dist, double* out, int64_t* index, void* stream) {
  if (!queries || !sorted_ref || !sorted_index || !cell_start || !out || !index || m <= 0 || !(cell > 0.0) || !(max_dist > 0.0))
    return SURF_E_ARG;
  if (nx <= 0 || ny <= 0 || nz <= 0) return SURF_E_ARG;
  if (m > INT32_MAX || nx > kGridAxis || ny > kGridAxis || nz > kGridAxis) return SURF_E_LIMIT;
  NearestIndexArgs a{queries, m, sorted_ref, sorted_index, cell_start, {lo_x, lo_y, lo_z}, cell, max_dist, {nx, ny, nz}, out, index};
  hipLaunchKernelGGL((surf_nearest_kernel<true, NearestIndexArgs>), dim3(blocks(m)), dim3(256), 0, (hipStream_t)stream, a);
  return surf_check_launch();
}

extern "C" int surf_fscore_icp_sums(const double* source, const double* target, int64_t n_target, const int64_t* index,
                                    const double* dist, int64_t n, double* partials, double* out, void* stream) {
  if (!source || !target || !index || !dist || !partials || !out || n <= 0 || n_target <= 0) return SURF_E_ARG;
  if (n > INT32_MAX || n_target > INT32_MAX) return SURF_E_LIMIT;
  PairArgs a{source, target, index, dist, n, n_target, {0, 0, 0}, {0, 0, 0}, partials};
  const int slots = slots_for(n, kSlots);
  hipLaunchKernelGGL(icp_sums_kernel, dim3(slots), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(slot_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, slots, 8, out);
  return surf_check_launch();
}

extern "C" int surf_fscore_icp_cov(const double* source, const double* target, int64_t n_target, const int64_t* index, int64_t n,
                                   const double* h_centroids, double* partials, double* out, void* stream) {
  if (!source || !target || !index || !h_centroids || !partials || !out || n <= 0 || n_target <= 0) return SURF_E_ARG;
  if (n > INT32_MAX || n_target > INT32_MAX) return SURF_E_LIMIT;
  PairArgs a{source, target, index, nullptr, n, n_target, {h_centroids[0], h_centroids[1], h_centroids[2]},
             {h_centroids[3], h_centroids[4], h_centroids[5]}, partials};
  const int slots = slots_for(n, kSlots);
  hipLaunchKernelGGL(icp_cov_kernel, dim3(slots), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(slot_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partials, slots, 9, out);
  return surf_check_launch();
}
