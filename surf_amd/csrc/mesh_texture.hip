// Textured meshes (surf_amd/mesh_texture.py, backend="device"): the source photographs baked into a per-triangle atlas.  THE RULE
// (rules 1-5) is written once, in include/surf_hip.h above the surf_texture_* entry points; this file and the numpy mirror in
// mesh_texture.py implement that text and give equal arrays.  fp32 throughout, one operation per operator (the library is compiled
// with -ffp-contract=off); fp32 division and sqrtf are correctly rounded on gfx950 as they are in numpy.
//
//  * texture_pack_kernel: one pixel per lane, (r, g, b) and the mesh depth into one 16-byte record, so that a bilinear tap of the
//    bake kernel is ONE load that carries colour and depth.
//  * texture_bake_kernel: one texel per lane; face and barycentrics come from the texel index by rule 1 (no lookup table), the
//    accumulators (16 B, plus 4 B with a count) are read and written once per launch and live in registers across the launch's
//    views (<= SURF_FUSE_MAX_VIEWS, in the kernel arguments: 16 x 80 B).  The depth, bounds and cosine tests come before any
//    gather: about half the views of a ring of cameras fail them.  No atomics: a texel has one owner.
//  * texture_finish_kernel: rule 5, one texel per lane, three bytes out.
// All three are bandwidth kernels: 256-thread blocks, no LDS.  Nothing here has been tuned.
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

struct TexView {
  const float* rec;      // (H, W, 4) fp32: r, g, b, D
  float P[12];
  float c[3];
  int H, W;
  int pad;
};
struct TexViews { TexView v[SURF_FUSE_MAX_VIEWS]; };

// Rule 1 and the barycentrics of rule 2: the face of texel t of the atlas (>= m: the texel belongs to no face).
struct Texel {
  int64_t face;
  float beta, gamma;
};
__device__ __forceinline__ Texel texel_of(uint32_t t, int T, int cols, uint32_t Wa) {
  const uint32_t Y = t / Wa, X = t - Y * Wa;
  const uint32_t cc = X / (uint32_t)(T + 1), i = X - cc * (uint32_t)(T + 1);
  const uint32_t r = Y / (uint32_t)T, j = Y - r * (uint32_t)T;
  const int64_t k = (int64_t)r * cols + cc;
  const bool B = i + j >= (uint32_t)T;
  const float den = (float)(T - 2);
  Texel o;
  o.face = 2 * k + (B ? 1 : 0);
  o.beta = (float)(B ? T - (int)i : (int)i) / den;
  o.gamma = (float)(B ? T - 1 - (int)j : (int)j) / den;
  return o;
}

__device__ __forceinline__ bool finite3(const float* p) {
  return fabsf(p[0]) <= FLT_MAX && fabsf(p[1]) <= FLT_MAX && fabsf(p[2]) <= FLT_MAX;      // a NaN fails the compare
}

__device__ __forceinline__ float lerp1(float a, float b, float s) { return (1.0f - s) * a + s * b; }

__global__ __launch_bounds__(256) void texture_pack_kernel(const float* __restrict__ image, const float* __restrict__ depth,
                                                           int64_t pixels, f32x4* __restrict__ record) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pixels) return;
  f32x4 r = {image[i * 3 + 0], image[i * 3 + 1], image[i * 3 + 2], depth[i]};
  record[i] = r;
}

__global__ __launch_bounds__(256) void texture_bake_kernel(const float* __restrict__ vertices, int64_t n,
                                                           const int32_t* __restrict__ faces, int64_t m, int T, int cols,
                                                           uint32_t Wa, uint32_t total, TexViews views, int n_views, float z_min,
                                                           float depth_tol, float min_cos, int power, int two_sided, int first,
                                                           f32x4* __restrict__ sums, int32_t* __restrict__ count) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  if (!first) {
    acc = sums[t];
    if (count) cnt = count[t];
  }
  const Texel tx = texel_of(t, T, cols, Wa);
  bool live = tx.face < m;
  float p[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, ln = 0.0f;
  if (live) {
    const int32_t ia = faces[tx.face * 3 + 0], ib = faces[tx.face * 3 + 1], ic = faces[tx.face * 3 + 2];
    live = ia >= 0 && ia < n && ib >= 0 && ib < n && ic >= 0 && ic < n;
    if (live) {
      float a[3], b[3], c[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        a[e] = vertices[(int64_t)ia * 3 + e];
        b[e] = vertices[(int64_t)ib * 3 + e];
        c[e] = vertices[(int64_t)ic * 3 + e];
      }
      live = finite3(a) && finite3(b) && finite3(c);
      float e1[3], e2[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        e1[e] = b[e] - a[e];
        e2[e] = c[e] - a[e];
        p[e] = (a[e] + tx.beta * e1[e]) + tx.gamma * e2[e];
      }
      nrm[0] = e1[1] * e2[2] - e1[2] * e2[1];
      nrm[1] = e1[2] * e2[0] - e1[0] * e2[2];
      nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
      const float nn = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2];
      live = live && nn > 0.0f && nn <= FLT_MAX;
      ln = sqrtf(nn);
    }
  }
  if (live) {
    for (int v = 0; v < n_views; ++v) {
      const TexView& V = views.v[v];
      const float cx = ((V.P[0] * p[0] + V.P[1] * p[1]) + V.P[2] * p[2]) + V.P[3];
      const float cy = ((V.P[4] * p[0] + V.P[5] * p[1]) + V.P[6] * p[2]) + V.P[7];
      const float z = ((V.P[8] * p[0] + V.P[9] * p[1]) + V.P[10] * p[2]) + V.P[11];
      if (!(z > z_min)) continue;
      const float x = cx / z, y = cy / z;
      if (!(x >= 0.0f && x <= (float)(V.W - 1) && y >= 0.0f && y <= (float)(V.H - 1))) continue;
      const float dx = V.c[0] - p[0], dy = V.c[1] - p[1], dz = V.c[2] - p[2];
      const float nd = (nrm[0] * dx + nrm[1] * dy) + nrm[2] * dz;
      const float dd = (dx * dx + dy * dy) + dz * dz;
      float cs = nd / (ln * sqrtf(dd));
      if (two_sided) cs = fabsf(cs);
      if (!(cs >= min_cos)) continue;
      const int x0 = min((int)floorf(x), V.W - 2), y0 = min((int)floorf(y), V.H - 2);     // inside [0, W-2] x [0, H-2]: the test above
      const float fu = x - (float)x0, fv = y - (float)y0;
      const f32x4* row0 = reinterpret_cast<const f32x4*>(V.rec) + ((int64_t)y0 * V.W + x0);
      const f32x4* row1 = row0 + V.W;
      const f32x4 c00 = row0[0], c01 = row0[1], c10 = row1[0], c11 = row1[1];
      const float zt = z + depth_tol;
      bool vis = true;
      for (const f32x4& c : {c00, c01, c10, c11}) vis = vis && c[3] > 0.0f && z <= c[3] + depth_tol && c[3] <= zt;
      if (!vis) continue;
      float w = cs;
      for (int k = 1; k < power; ++k) w = w * cs;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float col = lerp1(lerp1(c00[e], c01[e], fu), lerp1(c10[e], c11[e], fu), fv);
        acc[e] = acc[e] + w * col;
      }
      acc[3] = acc[3] + w;
      cnt = cnt + 1;
    }
  }
  sums[t] = acc;
  if (count) count[t] = cnt;
}

__global__ __launch_bounds__(256) void texture_finish_kernel(const f32x4* __restrict__ sums, int64_t n,
                                                             const int32_t* __restrict__ faces, int64_t m, int T, int cols,
                                                             uint32_t Wa, uint32_t total, const uint8_t* __restrict__ vertex_colors,
                                                             float fill, uint8_t* __restrict__ atlas) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const Texel tx = texel_of(t, T, cols, Wa);
  float val[3] = {fill, fill, fill};
  if (tx.face < m) {
    const f32x4 s = sums[t];
    if (s[3] > 0.0f) {
#pragma unroll
      for (int e = 0; e < 3; ++e) val[e] = s[e] / s[3];
    } else if (vertex_colors) {
      const int32_t ia = faces[tx.face * 3 + 0], ib = faces[tx.face * 3 + 1], ic = faces[tx.face * 3 + 2];
      if (ia >= 0 && ia < n && ib >= 0 && ib < n && ic >= 0 && ic < n) {
        float beta = tx.beta, gamma = tx.gamma;
        const float sum = beta + gamma;
        if (sum > 1.0f) {
          beta = beta / sum;
          gamma = gamma / sum;
        }
        const float alpha = (1.0f - beta) - gamma;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const float ca = (float)vertex_colors[(int64_t)ia * 3 + e] / 255.0f, cb = (float)vertex_colors[(int64_t)ib * 3 + e] / 255.0f,
                      cc = (float)vertex_colors[(int64_t)ic * 3 + e] / 255.0f;
          val[e] = (alpha * ca + beta * cb) + gamma * cc;
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    float q = val[e] * 256.0f;
    q = fminf(fmaxf(q, 0.0f), 255.0f);
    atlas[(int64_t)t * 3 + e] = (uint8_t)q;
  }
}

// The layout arguments of surf_texture_bake and surf_texture_finish: 0, SURF_E_ARG or SURF_E_LIMIT, and the atlas size.
inline int check_layout(int64_t n, int64_t m, int T, int cols, int rows, uint32_t* Wa, uint32_t* total) {
  if (n < 0 || m < 1 || T < 4 || T > 64 || cols < 1 || rows < 1) return SURF_E_ARG;
  if (n > 0x7fffffffLL || m > 0x7fffffffLL) return SURF_E_LIMIT;
  if ((int64_t)rows * cols < (m + 1) / 2) return SURF_E_ARG;
  const int64_t Ha = (int64_t)rows * T, W = (int64_t)cols * (T + 1);
  if (Ha >= ((int64_t)1 << 31) || W >= ((int64_t)1 << 31) || Ha * W >= ((int64_t)1 << 31)) return SURF_E_LIMIT;
  *Wa = (uint32_t)W;
  *total = (uint32_t)(Ha * W);
  return 0;
}

}  // namespace

extern "C" int surf_texture_pack_view(const float* image, const float* depth, int H, int W, float* record, void* stream) {
  if (!image || !depth || !record || H < 2 || W < 2) return SURF_E_ARG;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= ((int64_t)1 << 31) / 4) return SURF_E_LIMIT;
  hipLaunchKernelGGL(texture_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, depth,
                     pixels, reinterpret_cast<f32x4*>(record));
  return surf_check_launch();
}

extern "C" int surf_texture_bake(const float* vertices, int64_t n, const int32_t* faces, int64_t m, int T, int cols, int rows,
                                 const float* h_P, const float* h_centre, const float* const* h_records, const int* h_hw,
                                 int n_views, float z_min, float depth_tol, float min_cos, int power, int two_sided, int first,
                                 float* sums, int32_t* count, void* stream) {
  if (!vertices || !faces || !sums || n_views < 0) return SURF_E_ARG;
  if (n_views > 0 && (!h_P || !h_centre || !h_records || !h_hw)) return SURF_E_ARG;
  if (power < 1 || power > 16 || z_min != z_min || depth_tol != depth_tol || min_cos != min_cos) return SURF_E_ARG;
  uint32_t Wa, total;
  if (int e = check_layout(n, m, T, cols, rows, &Wa, &total)) return e;
  if (n_views > SURF_FUSE_MAX_VIEWS) return SURF_E_LIMIT;
  TexViews views;
  for (int v = 0; v < SURF_FUSE_MAX_VIEWS; ++v) views.v[v] = TexView{};
  for (int v = 0; v < n_views; ++v) {
    TexView& V = views.v[v];
    const int H = h_hw[2 * v], W = h_hw[2 * v + 1];
    if (!h_records[v] || H < 2 || W < 2) return SURF_E_ARG;
    if ((int64_t)H * W >= ((int64_t)1 << 31) / 4) return SURF_E_LIMIT;
    V.rec = h_records[v];
    for (int e = 0; e < 12; ++e) V.P[e] = h_P[12 * v + e];
    for (int e = 0; e < 3; ++e) V.c[e] = h_centre[3 * v + e];
    V.H = H;
    V.W = W;
  }
  hipLaunchKernelGGL(texture_bake_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, vertices, n, faces, m, T,
                     cols, Wa, total, views, n_views, z_min, depth_tol, min_cos, power, two_sided, first,
                     reinterpret_cast<f32x4*>(sums), count);
  return surf_check_launch();
}

extern "C" int surf_texture_finish(const float* sums, int64_t n, const int32_t* faces, int64_t m, int T, int cols, int rows,
                                   const uint8_t* vertex_colors, float fill, uint8_t* atlas, void* stream) {
  if (!sums || !faces || !atlas) return SURF_E_ARG;
  uint32_t Wa, total;
  if (int e = check_layout(n, m, T, cols, rows, &Wa, &total)) return e;
  hipLaunchKernelGGL(texture_finish_kernel, dim3((total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(sums), n, faces, m, T, cols, Wa, total, vertex_colors, fill, atlas);
  return surf_check_launch();
}
