// Reproducible sums of K running fp64 sums over n items, ONE copy for fscore.hip (the ICP reductions, K = 8 and 9) and
// point_knn.hip (the outlier statistic, K = 3): per-workgroup partial sums into fixed slots (the grid depends on n alone, every
// thread adds its items in index order, the workgroup's tree is fixed), then one workgroup adds the slots in slot order: the
// same bits on every run, no float atomics.
#pragma once
#include "common.h"

// K running sums of a thread of a 256-thread workgroup -> the workgroup's sums in part[blockIdx.x * K ..]: xor butterflies inside
// the four wavefronts (a fixed tree; every lane ends with the same bits), then the wavefronts' sums added in wavefront order.
template <int K>
__device__ __forceinline__ void block_partial(double (&acc)[K], double* __restrict__ part) {
  __shared__ double wave[4][K];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) wave[w][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < K) part[(int64_t)blockIdx.x * K + threadIdx.x] = ((wave[0][threadIdx.x] + wave[1][threadIdx.x]) + wave[2][threadIdx.x]) + wave[3][threadIdx.x];
}

// one workgroup: thread k adds slot 0, 1, ... of sum k (0 slots: zeros).  static: every file that includes this has its own
static __global__ __launch_bounds__(64) void slot_finish_kernel(const double* __restrict__ part, int slots, int K,
                                                                double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= K) return;
  double acc = 0.0;
  for (int s = 0; s < slots; ++s) acc += part[(int64_t)s * K + k];
  out[k] = acc;
}

// workgroups (= slots) of a reduction over n items, at most max_slots
inline int slots_for(int64_t n, int max_slots) { return (int)((n + 255) / 256 < max_slots ? (n + 255) / 256 : max_slots); }
