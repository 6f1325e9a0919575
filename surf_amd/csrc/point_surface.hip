// Point-set surface (surf_amd/point_surface.py, backend="device"): a signed distance on the lattice nodes near an oriented point
// cloud, Kolluri's implicit moving-least-squares surface with the compact weight (1 - q^2)^4, stored as fusion state (tsdf, weight,
// colour in 8^3-point bricks) so that marching cubes, vertex colours, ray casting and simplification run on it unchanged.  The
// rule is written once, above the surf_cloud_* entry points of include/surf_hip.h (rules 1-6); in short:
//  * a point takes part iff its coordinates and normal are finite and the normal is not (0,0,0); its lattice coordinate is
//    u = ((double)p - lo) / voxel per axis, its brick b = floor(u / 8), kept while -ring <= b < bricks + ring.
//  * a node's sums run over the points taking part in ascending (bx, by, bz, caller index) order - the order of the composite
//    keys surf_cloud_brick_keys writes - all in fp32: d2 = (dx*dx + dy*dy) + dz*dz, admitted iff d2 < R2, w = (1 - d2 / R2)^4,
//    g = (dx*nx + dy*ny) + dz*nz; count, sw, sf and the colour sums are sequential.
//  * reach (lattice steps, fp64, from the caller) is R / voxel plus the written-out margin; ring = ceil(reach / 8); the nodes a
//    point can be admitted at lie in [ceil(u - reach), floor(u + reach)] per axis.  surf_cloud_mark_bricks allocates the bricks
//    that box meets; the field kernel drops a candidate whose box misses the brick.  Both are the same integers on the host.
//
// The field kernel is an n-body tile.  One workgroup of 256 threads per allocated brick; thread t owns the two nodes of local
// index t and t + 256 (lx and lx + 4 at the same ly, lz: they share dy, dz and the four products made of them).  All 512 nodes
// share one candidate set: the points of the (2 ring + 1)^3 neighbouring bricks.  Bricks that differ only in bz are adjacent in
// key order, so the set is (2 ring + 1)^2 runs of the sorted keys, found by two binary searches each (threads 0 .. 2 rows - 1,
// log2(n) dependent loads; no start table - at res = 4096 a table over the extended brick grid would be 520^3 int32 = 562 MB, as
// much as the brick table itself).  The runs are walked in ascending key order, 256 raw candidates at a time: each thread loads
// one, tests its reach box against the brick, and the kept ones are appended to an LDS tile in their order (a ballot and a prefix
// over the four wavefronts).  Once the tile holds more than 256 candidates (or at the end) every thread runs through it
// sequentially: a candidate is three 16-byte LDS reads at an address all lanes share (a broadcast, no bank conflicts), the
// accumulators stay in registers, a rejected pair adds +0 (which leaves a sum that started at +0 as it is).  No atomics, no
// run-time indexed per-thread arrays, no scratch.
#include <math.h>

#include "band.h"

namespace {

constexpr int kThreads = 256;                       // threads of a field workgroup; raw candidates per staging step
constexpr int kTile = 2 * kThreads;                 // capacity of the LDS tile: it is run once it holds more than kThreads
constexpr int kMaxRing = SURF_CLOUD_MAX_RING;
constexpr int kMaxRows = (2 * kMaxRing + 1) * (2 * kMaxRing + 1);
constexpr int64_t kIndexBits = 31;                  // the caller index in the low bits of a composite key

struct Frame {                // the lattice as the point-side rules see it
  double lo[3], voxel;
  int n[3];                   // nodes per axis
  int nb[3];                  // bricks per axis that hold nodes
  int nbp;                    // bricks per axis of the table's cube
  int ring;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }

// lattice coordinate of a finite value
__device__ __forceinline__ double lattice_coord(float p, double lo, double voxel) { return ((double)p - lo) / voxel; }

// a brick coordinate as an int: u / 8 is exact; the clamp only keeps the conversion defined (the range test follows)
__device__ __forceinline__ int brick_coord(double u) { return (int)fmin(fmax(floor(u / 8.0), -2147483000.0), 2147483000.0); }

// the node interval [i0, i1] of one axis a point at lattice coordinate u can be admitted in (unclamped; empty when i0 > i1)
__device__ __forceinline__ void reach_interval(double u, double reach, int& i0, int& i1) {
  i0 = (int)fmin(fmax(ceil(u - reach), -2147483000.0), 2147483000.0);
  i1 = (int)fmin(fmax(floor(u + reach), -2147483000.0), 2147483000.0);
}

__global__ __launch_bounds__(256) void cloud_keys_kernel(const float* __restrict__ P, const float* __restrict__ N, int64_t n, Frame f,
                                                         int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int ex = f.nb[0] + 2 * f.ring, ey = f.nb[1] + 2 * f.ring, ez = f.nb[2] + 2 * f.ring;
  int64_t key = (int64_t)ex * ey * ez;                                   // behind every brick: takes no part
  const float x = P[i * 3 + 0], y = P[i * 3 + 1], z = P[i * 3 + 2];
  const float nx = N[i * 3 + 0], ny = N[i * 3 + 1], nz = N[i * 3 + 2];
  const bool fin = finite_f(x) && finite_f(y) && finite_f(z) && finite_f(nx) && finite_f(ny) && finite_f(nz);
  if (fin && !(nx == 0.0f && ny == 0.0f && nz == 0.0f)) {
    const int bx = brick_coord(lattice_coord(x, f.lo[0], f.voxel)), by = brick_coord(lattice_coord(y, f.lo[1], f.voxel)),
              bz = brick_coord(lattice_coord(z, f.lo[2], f.voxel));
    if (bx >= -f.ring && bx < f.nb[0] + f.ring && by >= -f.ring && by < f.nb[1] + f.ring && bz >= -f.ring && bz < f.nb[2] + f.ring)
      key = ((int64_t)(bx + f.ring) * ey + (by + f.ring)) * ez + (bz + f.ring);
  }
  keys[i] = (key << kIndexBits) | i;
}

__global__ __launch_bounds__(256) void cloud_mark_kernel(const float* __restrict__ SP, int64_t m, Frame f, double reach,
                                                         uint8_t* __restrict__ mark) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  int b0[3], b1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = SP[s * 3 + a];
    if (!finite_f(p)) return;                                            // cannot happen with the sorted points of rule 1
    int i0, i1;
    reach_interval(lattice_coord(p, f.lo[a], f.voxel), reach, i0, i1);
    i0 = max(i0, 0);
    i1 = min(i1, f.n[a] - 1);
    if (i0 > i1) return;
    b0[a] = i0 >> 3;
    b1[a] = i1 >> 3;
  }
  for (int bx = b0[0]; bx <= b1[0]; ++bx)
    for (int by = b0[1]; by <= b1[1]; ++by)
      for (int bz = b0[2]; bz <= b1[2]; ++bz) mark[band_brick_id<int64_t>(f.nbp, bx, by, bz)] = 1;
}

struct FieldArgs {
  const int64_t* skeys;       // (m) composite keys of the points taking part, ascending
  const float* spts;          // (m, 3) their coordinates, in that order
  const float* snrm;          // (m, 3) their normals
  const uint8_t* scol;        // (m, 3) their colours, or null
  int64_t m;
  const int32_t* bricks;      // (n_bricks) allocated brick ids
  const float *ax, *ay, *az;
  Frame f;
  double reach;
  float R, R2, inv;
  int min_points;
  float *tsdf, *weight, *color;
  int32_t* staged;            // (n_bricks) candidates that passed the reach test, or null
};

// the first position in [0, m) whose key is >= v
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ keys, int64_t m, int64_t v) {
  int64_t a = 0, b = m;
  while (a < b) {
    const int64_t c = a + ((b - a) >> 1);
    if (keys[c] < v) a = c + 1;
    else b = c;
  }
  return a;
}

struct Node {
  float x;
  int cnt;
  float sw, sf, c0, c1, c2;
};

template <bool COLOR>
__device__ __forceinline__ void pair(Node& q, float px, float nx, float dydy, float dzdz, float dyny, float dznz, float R2, float inv,
                                     float cr, float cg, float cb) {
  const float dx = q.x - px;
  const float d2 = (dx * dx + dydy) + dzdz;
  const bool in = d2 < R2;
  const float t = 1.0f - d2 * inv;
  const float t2 = t * t;
  const float w = in ? t2 * t2 : 0.0f;
  const float g = (dx * nx + dyny) + dznz;
  q.cnt += in ? 1 : 0;
  q.sw += w;
  q.sf += in ? w * g : 0.0f;
  if (COLOR) {
    q.c0 += w * cr;
    q.c1 += w * cg;
    q.c2 += w * cb;
  }
}

template <bool COLOR>
__global__ __launch_bounds__(kThreads) void cloud_field_kernel(FieldArgs a) {
  __shared__ float4 tp[kTile];                        // (px, py, pz, nx)
  __shared__ float4 tn[kTile];                        // (ny, nz, cr, cg)
  __shared__ float tc[COLOR ? kTile : 1];             // cb
  __shared__ int64_t row_lo[kMaxRows];                // first sorted position of every run
  __shared__ int64_t row_end[kMaxRows];               // raw candidates up to and including the run (a running total)
  __shared__ int wave_kept[kThreads / SURF_WAVE];

  const int tid = threadIdx.x;
  const int64_t slot = blockIdx.x;
  const Frame& f = a.f;
  const int id = a.bricks[slot];
  int Bx, By, Bz;
  band_brick_xyz(f.nbp, id, Bx, By, Bz);
  const bool brick_ok = id >= 0 && Bx < f.nb[0] && By < f.nb[1] && Bz < f.nb[2];     // (a well-formed brick list has no other)
  const int side = 2 * f.ring + 1, rows = brick_ok ? side * side : 0;
  const int ey = f.nb[1] + 2 * f.ring, ez = f.nb[2] + 2 * f.ring;

  // the runs: row r = (jx, jy) covers the extended bricks (Bx + jx, By + jy, Bz .. Bz + 2 ring), contiguous in key order
  if (tid < 2 * rows) {
    const int r = tid >> 1, jx = r / side, jy = r % side;
    const int64_t k0 = ((int64_t)(Bx + jx) * ey + (By + jy)) * ez + Bz;
    const int64_t pos = lower_bound(a.skeys, a.m, (k0 + ((tid & 1) ? side : 0)) << kIndexBits);
    if (tid & 1) row_end[r] = pos;
    else row_lo[r] = pos;
  }
  __syncthreads();
  if (tid == 0) {
    int64_t total = 0;
    for (int r = 0; r < rows; ++r) {
      total += row_end[r] - row_lo[r];
      row_end[r] = total;
    }
  }
  __syncthreads();
  const int64_t total = rows ? row_end[rows - 1] : 0;

  const int lx = tid >> 6, ly = (tid >> 3) & 7, lz = tid & 7;
  const int ix = Bx * 8 + lx, iy = By * 8 + ly, iz = Bz * 8 + lz;
  const bool in_yz = brick_ok && iy < f.n[1] && iz < f.n[2];
  const bool in0 = in_yz && ix < f.n[0], in1 = in_yz && ix + 4 < f.n[0];
  Node q0{in0 ? a.ax[ix] : 0.0f, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, q1{in1 ? a.ax[ix + 4] : 0.0f, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const float y = in_yz ? a.ay[iy] : 0.0f, z = in_yz ? a.az[iz] : 0.0f;

  int fill = 0, kept_all = 0;
  int row = 0;                                          // the run that holds this thread's raw candidate: it only moves forward
  for (int64_t v0 = 0; v0 < total; v0 += kThreads) {
    const int64_t v = v0 + tid;
    bool keep = false;
    int64_t s = 0;
    if (v < total) {
      while (row_end[row] <= v) ++row;                  // v < total = row_end[rows - 1]: row stays below rows
      s = row_lo[row] + (v - (row ? row_end[row - 1] : 0));
      keep = true;
#pragma unroll
      for (int ax3 = 0; ax3 < 3; ++ax3) {
        int i0, i1;
        reach_interval(lattice_coord(a.spts[s * 3 + ax3], f.lo[ax3], f.voxel), a.reach, i0, i1);
        const int B = ax3 == 0 ? Bx : (ax3 == 1 ? By : Bz);
        keep = keep && i0 <= B * 8 + 7 && i1 >= B * 8;
      }
    }
    // append the kept candidates in their order
    const uint64_t ballot = __ballot(keep);
    const int lane = tid & (SURF_WAVE - 1), wave = tid / SURF_WAVE;
    if (lane == 0) wave_kept[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, step = 0;
#pragma unroll
    for (int w = 0; w < kThreads / SURF_WAVE; ++w) {
      const int c = wave_kept[w];
      before += w < wave ? c : 0;
      step += c;
    }
    if (keep) {
      const int at = fill + before + __popcll(ballot & ((uint64_t(1) << lane) - 1));
      float cr = 0.0f, cg = 0.0f, cb = 0.0f;
      if (COLOR) {
        cr = ((float)a.scol[s * 3 + 0] + 0.5f) * 0.00390625f;
        cg = ((float)a.scol[s * 3 + 1] + 0.5f) * 0.00390625f;
        cb = ((float)a.scol[s * 3 + 2] + 0.5f) * 0.00390625f;
        tc[at] = cb;
      }
      tp[at] = make_float4(a.spts[s * 3 + 0], a.spts[s * 3 + 1], a.spts[s * 3 + 2], a.snrm[s * 3 + 0]);
      tn[at] = make_float4(a.snrm[s * 3 + 1], a.snrm[s * 3 + 2], cr, cg);
    }
    fill += step;                                       // <= kThreads + kThreads = kTile
    kept_all += step;
    __syncthreads();
    if (fill > kThreads || v0 + kThreads >= total) {
      for (int c = 0; c < fill; ++c) {
        const float4 P = tp[c], Q = tn[c];
        const float dy = y - P.y, dz = z - P.z;
        const float dydy = dy * dy, dzdz = dz * dz, dyny = dy * Q.x, dznz = dz * Q.y;
        const float cb = COLOR ? tc[c] : 0.0f;
        pair<COLOR>(q0, P.x, P.w, dydy, dzdz, dyny, dznz, a.R2, a.inv, Q.z, Q.w, cb);
        pair<COLOR>(q1, P.x, P.w, dydy, dzdz, dyny, dznz, a.R2, a.inv, Q.z, Q.w, cb);
      }
      fill = 0;
      __syncthreads();
    }
  }

  // node state in fusion's conventions
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const Node& q = h ? q1 : q0;
    const bool inside = h ? in1 : in0;
    const bool obs = inside && q.cnt >= a.min_points && q.sw > 0.0f;
    const int64_t o = slot * 512 + tid + h * kThreads;
    a.tsdf[o] = obs ? fminf(fmaxf((q.sf / q.sw) / a.R, -1.0f), 1.0f) : 0.0f;
    a.weight[o] = obs ? (float)q.cnt : 0.0f;
    if (COLOR) {
      a.color[o * 3 + 0] = obs ? q.c0 / q.sw : 0.0f;
      a.color[o * 3 + 1] = obs ? q.c1 / q.sw : 0.0f;
      a.color[o * 3 + 2] = obs ? q.c2 / q.sw : 0.0f;
    }
  }
  if (a.staged && tid == 0) a.staged[slot] = kept_all;
}

// the lattice checks every entry point shares; 0 or a status
int frame_of(double lo_x, double lo_y, double lo_z, double voxel, int64_t nx, int64_t ny, int64_t nz, int ring, Frame& f) {
  if (!isfinite(lo_x) || !isfinite(lo_y) || !isfinite(lo_z) || !(voxel > 0.0) || !(voxel < INFINITY)) return SURF_E_ARG;
  if (nx < 1 || ny < 1 || nz < 1 || ring < 1) return SURF_E_ARG;
  const int64_t res = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  if (res < 2) return SURF_E_ARG;
  if (res > SURF_BAND_MAX_RES || ring > kMaxRing) return SURF_E_LIMIT;
  f.lo[0] = lo_x;
  f.lo[1] = lo_y;
  f.lo[2] = lo_z;
  f.voxel = voxel;
  const int64_t n[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    f.n[a] = (int)n[a];
    f.nb[a] = (int)((n[a] + 7) / 8);
  }
  f.nbp = (int)((res + 7) / 8);
  f.ring = ring;
  return 0;
}

// ring by rule 2 from reach; 0 when reach is no positive finite number
int ring_of(double reach) {
  if (!(reach > 0.0) || !(reach < 1e9)) return 0;
  return (int)ceil(reach / 8.0);
}

}  // namespace

extern "C" int surf_cloud_brick_keys(const float* points, const float* normals, int64_t n, double lo_x, double lo_y, double lo_z,
                                     double voxel, int64_t nx, int64_t ny, int64_t nz, double reach, int64_t* keys, void* stream) {
  if (n == 0) return 0;
  if (!points || !normals || !keys || n < 0) return SURF_E_ARG;
  Frame f;
  if (const int st = frame_of(lo_x, lo_y, lo_z, voxel, nx, ny, nz, ring_of(reach), f)) return st;
  if (n > INT32_MAX) return SURF_E_LIMIT;
  hipLaunchKernelGGL(cloud_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, normals, n, f, keys);
  return surf_check_launch();
}

extern "C" int surf_cloud_mark_bricks(const float* sorted_points, int64_t m, double lo_x, double lo_y, double lo_z, double voxel,
                                      int64_t nx, int64_t ny, int64_t nz, double reach, uint8_t* mark, void* stream) {
  if (m == 0) return 0;
  if (!sorted_points || !mark || m < 0) return SURF_E_ARG;
  Frame f;
  if (const int st = frame_of(lo_x, lo_y, lo_z, voxel, nx, ny, nz, ring_of(reach), f)) return st;
  if (m > INT32_MAX) return SURF_E_LIMIT;
  hipLaunchKernelGGL(cloud_mark_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sorted_points, m, f, reach,
                     mark);
  return surf_check_launch();
}

extern "C" int surf_cloud_field_bricks(const int64_t* sorted_keys, const float* sorted_points, const float* sorted_normals,
                                       const uint8_t* sorted_colors, int64_t m, const int32_t* bricks, int64_t n_bricks,
                                       const float* ax, const float* ay, const float* az, int64_t nx, int64_t ny, int64_t nz,
                                       double lo_x, double lo_y, double lo_z, double voxel, double reach, float radius, int min_points,
                                       float* tsdf, float* weight, float* color, int32_t* staged, void* stream) {
  if (n_bricks == 0) return 0;
  if (!bricks || !ax || !ay || !az || !tsdf || !weight || n_bricks < 0 || m < 0 || min_points < 1) return SURF_E_ARG;
  if (m > 0 && (!sorted_keys || !sorted_points || !sorted_normals)) return SURF_E_ARG;
  if ((sorted_colors != nullptr) != (color != nullptr)) return SURF_E_ARG;
  if (!(radius > 0.0f) || !(radius < INFINITY)) return SURF_E_ARG;
  const float R2 = radius * radius;
  if (!(R2 > 0.0f) || !(R2 < INFINITY)) return SURF_E_ARG;
  Frame f;
  if (const int st = frame_of(lo_x, lo_y, lo_z, voxel, nx, ny, nz, ring_of(reach), f)) return st;
  if (m > INT32_MAX || n_bricks * 512 >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  const FieldArgs a{sorted_keys, sorted_points, sorted_normals, sorted_colors, m, bricks, ax, ay, az, f, reach, radius, R2, 1.0f / R2,
                    min_points, tsdf, weight, color, staged};
  if (color)
    hipLaunchKernelGGL(cloud_field_kernel<true>, dim3((unsigned)n_bricks), dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cloud_field_kernel<false>, dim3((unsigned)n_bricks), dim3(kThreads), 0, (hipStream_t)stream, a);
  return surf_check_launch();
}
