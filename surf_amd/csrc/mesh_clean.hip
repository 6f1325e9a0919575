// Mesh cleaning on the device (surf_amd/evaluation/clean_mesh.py, backend="device"): every stage of the host cleaner as a
// kernel whose result equals the host stage's.  raster.hip's z-buffer is reused unchanged.
//
//  * dilate_kernel: binary dilation with skimage's disk footprint dx*dx + dy*dy <= r*r, integer arithmetic, outside the image
//    unset (scipy.ndimage.binary_dilation's border): equal to dilate_disk bit for bit.
//  * hull_kernel: the visual-hull vertex test, one thread per vertex, all views in one launch.  The library is compiled with
//    -ffp-contract=off; every line below is one fp32 operation per operator, evaluated left to right as parenthesised:
//        cx = ((w[0]*X + w[1]*Y) + w[2]*Z) + w[3]        cy, cz likewise with w[4..7], w[8..11]   (w = inverse(c2w)[:3,:4])
//        u  = (K[0]*cx + K[1]*cy) + K[2]*cz              v, d likewise with K[3..5], K[6..8]
//        dc = max(d, 1e-8f);  px = u / dc;  py = v / dc                                          (IEEE fp32 division)
//        inside = px >= 0 && px <= w-1 && py >= 0 && py <= h-1 && d > 1e-8f
//        qx = min(max(px, -far), far), qy likewise, far = 10 * max(h, w)
//        x0 = floor(qx), fx = qx - x0, y0 = floor(qy), fy = qy - y0
//        total = 0; for (dy, wy) in ((0, 1-fy), (1, fy)): for (dx, wx) in ((0, 1-fx), (1, fx)):
//            total += (m[y0+dy][x0+dx] * wx) * wy      where the texel lies inside the image (m = 1.0f set, 0.0f unset)
//        seen by this view = inside && total > 0
//    tests/test_clean_mesh_gpu.py mirrors exactly this sequence in numpy fp32.
//  * face_keep_kernel: keep[f] = every vertex of f has n_seen > min_nb_visible.
//  * mark_kernel: seen[face] = 1 for every sample of the z-buffer that holds a hit and whose mask texel is set.  Sample (i, j)
//    of the up-scaled lattice reads texel (i / upscale, j / upscale) (integer division), the mapping of
//    F.interpolate(scale_factor=upscale, mode="nearest") for integer factors.
//  * face connected components: a lock-free union-find over faces.
//      1. cc_insert: every face puts its three undirected edges, keyed (min(v) << 32) | max(v), into an open-addressing table
//         (linear probing, 64-bit atomicCAS on the key), atomicMin's its id into the slot's owner and remembers the slot.  An
//         arrival that finds the owner already set marks the slot as shared.
//      2. cc_union: every face-edge whose slot is shared gives its face a neighbour and unites the face with the slot's owner
//         (the smallest face on that edge, so a fan of k faces on one edge becomes one set, as the host's consecutive pairing of
//         the sorted edge list does; an edge that one face lists twice gives that face itself as neighbour, as there).
//         INVARIANT: parent[x] <= x at all times.  A root is only ever hooked, by atomicCAS(parent[r], r, s) with s < r, under
//         a smaller face; path compression replaces parent[x] of a non-root by one of its ancestors.  So there are no cycles,
//         a non-root never becomes a root again, and the root of a finished set is its smallest face id whatever the order
//         in which the atomics landed.
//      3. cc_flatten: parent[f] = find(f) without compression (one writer per entry), size[root] += 1 (integer atomicAdd: exact).
//      4. cc_keep: keep[f] = size[root[f]] >= min_len && f has a neighbour.
//    HBM- and atomic-bound (no arithmetic to speak of): 256-thread blocks, no LDS, few registers, full occupancy.
//  * mark_used / compact_faces / compact_rows: update_faces (used-vertex flags, remap, order-preserving gather); the inclusive
//    scans between them are the caller's (torch.cumsum).
// Offline tool, not part of the training / render hot path.
#include <math.h>

#include "common.h"

namespace {

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int32_t kNoOwner = INT32_MAX;
constexpr int64_t kMaxSlots = int64_t(1) << 31;      // slot numbers are kept as uint32

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

__global__ __launch_bounds__(256) void dilate_kernel(const uint8_t* __restrict__ in, int nv, int h, int w, int r,
                                                     uint8_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nv * h * w) return;
  const int x = (int)(t % w), y = (int)((t / w) % h);
  const uint8_t* img = in + (t / ((int64_t)h * w)) * ((int64_t)h * w);
  uint8_t hit = 0;
  for (int dy = -r; dy <= r && !hit; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= h) continue;
    for (int dx = -r; dx <= r; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= w || dx * dx + dy * dy > r * r) continue;
      if (img[(int64_t)yy * w + xx]) { hit = 1; break; }
    }
  }
  out[t] = hit;
}

// cams: per view K (9, row-major) then inverse(c2w)[:3,:4] (12, row-major)
__global__ __launch_bounds__(256) void hull_kernel(const float* __restrict__ V, int64_t n, const uint8_t* __restrict__ masks,
                                                   const float* __restrict__ cams, int nv, int h, int w,
                                                   int32_t* __restrict__ n_seen) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const float X = V[t * 3 + 0], Y = V[t * 3 + 1], Z = V[t * 3 + 2];
  const float wm1 = (float)(w - 1), hm1 = (float)(h - 1), far = 10.0f * (float)max(h, w);
  int32_t cnt = 0;
  for (int i = 0; i < nv; ++i) {
    const float* K = cams + i * 21;
    const float* W = K + 9;
    const uint8_t* m = masks + (int64_t)i * h * w;
    const float cx = ((W[0] * X + W[1] * Y) + W[2] * Z) + W[3];
    const float cy = ((W[4] * X + W[5] * Y) + W[6] * Z) + W[7];
    const float cz = ((W[8] * X + W[9] * Y) + W[10] * Z) + W[11];
    const float u = (K[0] * cx + K[1] * cy) + K[2] * cz;
    const float v = (K[3] * cx + K[4] * cy) + K[5] * cz;
    const float d = (K[6] * cx + K[7] * cy) + K[8] * cz;
    const float dc = fmaxf(d, 1e-8f);
    const float px = u / dc, py = v / dc;
    const bool inside = px >= 0.0f && px <= wm1 && py >= 0.0f && py <= hm1 && d > 1e-8f;
    const float qx = fminf(fmaxf(px, -far), far), qy = fminf(fmaxf(py, -far), far);
    const float x0 = floorf(qx), y0 = floorf(qy);
    const float fx = qx - x0, fy = qy - y0;
    const int xi = (int)x0, yi = (int)y0;
    float total = 0.0f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const float wy = dy ? fy : 1.0f - fy;
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const float wx = dx ? fx : 1.0f - fx;
        const int xx = xi + dx, yy = yi + dy;
        if (xx >= 0 && xx < w && yy >= 0 && yy < h) total += ((m[(int64_t)yy * w + xx] ? 1.0f : 0.0f) * wx) * wy;
      }
    }
    cnt += (inside && total > 0.0f) ? 1 : 0;
  }
  n_seen[t] = cnt;
}

__global__ __launch_bounds__(256) void face_keep_kernel(const int32_t* __restrict__ n_seen, const int32_t* __restrict__ faces,
                                                        int64_t nf, int min_nb_visible, uint8_t* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  keep[f] = n_seen[faces[f * 3 + 0]] > min_nb_visible && n_seen[faces[f * 3 + 1]] > min_nb_visible &&
            n_seen[faces[f * 3 + 2]] > min_nb_visible;
}

__global__ __launch_bounds__(256) void mark_kernel(const unsigned long long* __restrict__ zbuf, int Hup, int Wup,
                                                   const uint8_t* __restrict__ mask, int w, int upscale, int64_t nf,
                                                   uint8_t* __restrict__ seen) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Hup * Wup) return;
  const unsigned long long z = zbuf[t];
  if (z == kEmptyKey) return;
  const int i = (int)(t / Wup), j = (int)(t % Wup);
  if (!mask[(int64_t)(i / upscale) * w + j / upscale]) return;
  const int64_t f = (int64_t)(z & 0xffffffffull);
  if (f < nf) seen[f] = 1;
}

// ---- connected components ----

__device__ __forceinline__ int32_t ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint64_t mix64(uint64_t k) {       // murmur3's finaliser
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

struct CcArgs {
  const int32_t* faces;
  int64_t nf;
  unsigned long long* keys;   // (slots) ~0 = empty
  int32_t* owner;             // (slots) smallest face id on the edge, INT32_MAX = none yet
  uint8_t* shared;            // (slots) 1 = the edge was listed more than once
  uint32_t slot_mask;         // slots - 1 (slots a power of two <= 2^31)
  uint32_t* edge_slot;        // (3 nf) slot of every face-edge
  int32_t* parent;            // (nf)
  uint8_t* has_nb;            // (nf)
  int32_t* size;              // (nf)
  int64_t min_len;
  uint8_t* keep;              // (nf)
};

__global__ __launch_bounds__(256) void cc_insert_kernel(CcArgs a) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.nf) return;
  uint32_t v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = (uint32_t)a.faces[f * 3 + k];
  a.parent[f] = (int32_t)f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t p = v[k], q = v[(k + 1) % 3];
    const unsigned long long key = ((unsigned long long)min(p, q) << 32) | (unsigned long long)max(p, q);
    uint32_t s = (uint32_t)mix64(key) & a.slot_mask;
    // the table holds more slots than there are face-edges, so an empty slot always ends the probe
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&a.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kEmptyKey) cur = atomicCAS(&a.keys[s], kEmptyKey, key);
      if (cur == kEmptyKey || cur == key) break;
      s = (s + 1) & a.slot_mask;
    }
    if (atomicMin(&a.owner[s], (int32_t)f) != kNoOwner) a.shared[s] = 1;
    a.edge_slot[f * 3 + k] = s;
  }
}

template <bool kCompress = true>
__device__ __forceinline__ int32_t cc_find(int32_t* parent, int32_t x) {
  int32_t p = ld(&parent[x]);
  while (p != x) {
    const int32_t g = ld(&parent[p]);
    if (kCompress && g != p) st(&parent[x], g);       // halving: an ancestor replaces the parent of a non-root
    x = p;
    p = g;
  }
  return x;
}

__global__ __launch_bounds__(256) void cc_union_kernel(CcArgs a) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.nf * 3) return;
  const uint32_t s = a.edge_slot[e];
  if (!a.shared[s]) return;
  const int32_t f = (int32_t)(e / 3);
  a.has_nb[f] = 1;
  int32_t x = cc_find(a.parent, f), y = cc_find(a.parent, a.owner[s]);
  while (x != y) {
    if (x < y) { const int32_t t = x; x = y; y = t; }          // hook the larger root x under the smaller y
    const int32_t old = atomicCAS(&a.parent[x], x, y);
    if (old == x) break;
    x = cc_find(a.parent, old);                                  // x was hooked meanwhile: continue from its new root
    y = cc_find(a.parent, y);
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(CcArgs a) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.nf) return;
  // no compression here: parent[f] has one writer in this pass, its own thread, so the root written below stays (a halving
  // store of another walk, formed from an older read, could put a non-root ancestor back over it)
  const int32_t r = cc_find<false>(a.parent, (int32_t)f);
  st(&a.parent[f], r);                   // r is f's root: still an ancestor, concurrent walks stay correct
  atomicAdd(&a.size[r], 1);
}

__global__ __launch_bounds__(256) void cc_keep_kernel(CcArgs a) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.nf) return;
  a.keep[f] = a.has_nb[f] && (int64_t)a.size[a.parent[f]] >= a.min_len;
}

// ---- compaction ----

__global__ __launch_bounds__(256) void mark_used_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                        int64_t nf, int64_t nv, uint8_t* __restrict__ used) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf || !keep[f]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t v = faces[f * 3 + k];
    if (v >= 0 && v < nv) used[v] = 1;
  }
}

// out[fscan[f] - 1] = (vscan ? vscan[faces[f]] - 1 : faces[f]) for the kept faces; scans are INCLUSIVE
__global__ __launch_bounds__(256) void compact_faces_kernel(const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep,
                                                            const int64_t* __restrict__ fscan, const int64_t* __restrict__ vscan,
                                                            int64_t nf, int64_t nv, int32_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf || !keep[f]) return;
  int32_t* o = out + (fscan[f] - 1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int32_t v = faces[f * 3 + k];
    o[k] = vscan ? ((v >= 0 && v < nv) ? (int32_t)(vscan[v] - 1) : -1) : v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void compact_rows_kernel(const T* __restrict__ src, const uint8_t* __restrict__ flags,
                                                           const int64_t* __restrict__ scan, int64_t n, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flags[i]) return;
  T* o = out + (scan[i] - 1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = src[i * 3 + k];
}

}  // namespace

extern "C" int surf_clean_dilate(const uint8_t* masks, int n_views, int h, int w, int radius, uint8_t* out, void* stream) {
  if (!masks || !out || n_views <= 0 || h <= 0 || w <= 0 || radius < 0) return SURF_E_ARG;
  if (radius > 16384 || (int64_t)n_views * h * w > ((int64_t)1 << 40)) return SURF_E_LIMIT;   // r*r and the grid stay in range
  hipLaunchKernelGGL(dilate_kernel, dim3(blocks((int64_t)n_views * h * w)), dim3(256), 0, (hipStream_t)stream, masks, n_views, h, w,
                     radius, out);
  return surf_check_launch();
}

extern "C" int surf_clean_hull_count(const float* vertices, int64_t n_vertices, const uint8_t* masks, const float* cams,
                                     int n_views, int h, int w, int32_t* n_seen, void* stream) {
  if (n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!vertices || !masks || !cams || !n_seen || n_vertices <= 0 || n_views <= 0 || h <= 0 || w <= 0) return SURF_E_ARG;
  if (h > (1 << 20) || w > (1 << 20)) return SURF_E_LIMIT;                                     // 10 * max(h, w) as an int
  hipLaunchKernelGGL(hull_kernel, dim3(blocks(n_vertices)), dim3(256), 0, (hipStream_t)stream, vertices, n_vertices, masks, cams,
                     n_views, h, w, n_seen);
  return surf_check_launch();
}

extern "C" int surf_clean_face_keep(const int32_t* n_seen, const int32_t* faces, int64_t n_faces, int min_nb_visible,
                                    uint8_t* keep, void* stream) {
  if (n_faces >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!n_seen || !faces || !keep || n_faces <= 0) return SURF_E_ARG;
  hipLaunchKernelGGL(face_keep_kernel, dim3(blocks(n_faces)), dim3(256), 0, (hipStream_t)stream, n_seen, faces, n_faces,
                     min_nb_visible, keep);
  return surf_check_launch();
}

extern "C" int surf_clean_mark_visible(const unsigned long long* zbuf, int Hup, int Wup, const uint8_t* mask, int h, int w,
                                       int upscale, int64_t n_faces, uint8_t* seen, void* stream) {
  if (!zbuf || !mask || !seen || h <= 0 || w <= 0 || upscale < 1 || n_faces <= 0) return SURF_E_ARG;
  if (Hup != h * upscale || Wup != w * upscale) return SURF_E_ARG;
  hipLaunchKernelGGL(mark_kernel, dim3(blocks((int64_t)Hup * Wup)), dim3(256), 0, (hipStream_t)stream, zbuf, Hup, Wup, mask, w,
                     upscale, n_faces, seen);
  return surf_check_launch();
}

extern "C" int64_t surf_clean_components_slots(int64_t n_faces) {
  if (n_faces <= 0) return SURF_E_ARG;
  if (n_faces >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  int64_t slots = 1024;
  while (slots < 4 * n_faces) slots <<= 1;          // > 3 n_faces keys at most: load <= 0.75, 0.375 on a closed manifold
  return slots <= kMaxSlots ? slots : (int64_t)SURF_E_LIMIT;
}

extern "C" int surf_clean_components(const int32_t* faces, int64_t n_faces, int64_t min_len, unsigned long long* keys,
                                     int32_t* owner, uint8_t* shared, int64_t slots, uint32_t* edge_slot, int32_t* parent,
                                     uint8_t* has_nb, int32_t* size, uint8_t* keep, void* stream) {
  if (n_faces <= 0) return SURF_E_ARG;
  const int64_t want = surf_clean_components_slots(n_faces);
  if (want < 0) return (int)want;
  if (!faces || !keys || !owner || !shared || !edge_slot || !parent || !has_nb || !size || !keep || slots != want) return SURF_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if ((e = hipMemsetAsync(keys, 0xff, (size_t)slots * 8, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(shared, 0, (size_t)slots, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(has_nb, 0, (size_t)n_faces, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(size, 0, (size_t)n_faces * 4, s)) != hipSuccess) return (int)e;
  // owner = INT32_MAX: 0x7f7f7f7f would do for the minimum, but "none yet" is compared for equality
  if ((e = hipMemsetD32Async((hipDeviceptr_t)owner, kNoOwner, (size_t)slots, s)) != hipSuccess) return (int)e;
  CcArgs a{faces, n_faces, keys, owner, shared, (uint32_t)(slots - 1), edge_slot, parent, has_nb, size, min_len, keep};
  hipLaunchKernelGGL(cc_insert_kernel, dim3(blocks(n_faces)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cc_union_kernel, dim3(blocks(n_faces * 3)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks(n_faces)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cc_keep_kernel, dim3(blocks(n_faces)), dim3(256), 0, s, a);
  return surf_check_launch();
}

extern "C" int surf_clean_mark_used(const int32_t* faces, const uint8_t* keep, int64_t n_faces, int64_t n_vertices, uint8_t* used,
                                    void* stream) {
  if (n_faces >= ((int64_t)1 << 31) || n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!faces || !keep || !used || n_faces <= 0 || n_vertices <= 0) return SURF_E_ARG;
  hipLaunchKernelGGL(mark_used_kernel, dim3(blocks(n_faces)), dim3(256), 0, (hipStream_t)stream, faces, keep, n_faces, n_vertices,
                     used);
  return surf_check_launch();
}

extern "C" int surf_clean_compact_faces(const int32_t* faces, const uint8_t* keep, const int64_t* face_scan,
                                        const int64_t* vertex_scan, int64_t n_faces, int64_t n_vertices, int32_t* out,
                                        void* stream) {
  if (n_faces >= ((int64_t)1 << 31) || n_vertices >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!faces || !keep || !face_scan || !out || n_faces <= 0 || n_vertices <= 0) return SURF_E_ARG;
  hipLaunchKernelGGL(compact_faces_kernel, dim3(blocks(n_faces)), dim3(256), 0, (hipStream_t)stream, faces, keep, face_scan,
                     vertex_scan, n_faces, n_vertices, out);
  return surf_check_launch();
}

extern "C" int surf_clean_compact_rows(const void* src, int elem_bytes, const uint8_t* flags, const int64_t* scan, int64_t n,
                                       void* out, void* stream) {
  if (n >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  if (!src || !flags || !scan || !out || n <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return SURF_E_ARG;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(compact_rows_kernel<uint32_t>, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)src, flags,
                       scan, n, (uint32_t*)out);
  else
    hipLaunchKernelGGL(compact_rows_kernel<uint64_t>, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const uint64_t*)src, flags,
                       scan, n, (uint64_t*)out);
  return surf_check_launch();
}
