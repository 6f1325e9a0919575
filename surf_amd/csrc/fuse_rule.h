// The per-point rules of depth-map fusion, ONE copy for fuse.hip (dense lattice) and fuse_sparse.hip (brick-major state): the view
// table of a launch with its host-side filler, the integration of all views into one lattice point, and the colour of a mesh
// vertex.  The operations and their order are written out in fuse.hip's header comment; the library is compiled with
// -ffp-contract=off, so every operator below is one fp32 operation.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"

struct FuseView {
  float P[12];
  const float* depth;
  const float* image;
  int H, W;
  float dscale;
  int pad;
};
struct FuseViews { FuseView v[SURF_FUSE_MAX_VIEWS]; };

// The host side of a launch's view table (surf_fuse_integrate's h_P / h_depths / h_images / h_hw / h_dscale): 0, SURF_E_ARG or
// SURF_E_LIMIT.  color: are colours fused (then every view needs an image).
inline int surf_fill_fuse_views(FuseViews& views, bool color, const float* h_P, const float* const* h_depths,
                                const float* const* h_images, const int* h_hw, const float* h_dscale, int n_views) {
  for (int v = 0; v < n_views; ++v) {
    FuseView& V = views.v[v];
    const int H = h_hw[2 * v], W = h_hw[2 * v + 1];
    if (!h_depths[v] || H < 1 || W < 1 || (color && !h_images[v])) return SURF_E_ARG;
    if ((int64_t)H * W >= ((int64_t)1 << 31) / 3) return SURF_E_LIMIT;
    for (int e = 0; e < 12; ++e) V.P[e] = h_P[12 * v + e];
    V.depth = h_depths[v];
    V.image = color ? h_images[v] : nullptr;
    V.H = H;
    V.W = W;
    V.dscale = h_dscale[v];
    V.pad = 0;
  }
  for (int v = n_views; v < SURF_FUSE_MAX_VIEWS; ++v) views.v[v] = FuseView{};
  return 0;
}

// All views of a launch into the state of the lattice point (px, py, pz) at position i of the state arrays, in registers;
// written back only when some view observed the point.
template <bool COLOR>
__device__ __forceinline__ void surf_fuse_integrate_point(float* __restrict__ tsdf, float* __restrict__ weight,
                                                          float* __restrict__ color, int64_t i, float px, float py, float pz,
                                                          const FuseViews& views, int n_views, float trunc) {
  float ts = tsdf[i], w = weight[i];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  if (COLOR) { c0 = color[i * 3 + 0]; c1 = color[i * 3 + 1]; c2 = color[i * 3 + 2]; }
  const float w0 = w;
  for (int v = 0; v < n_views; ++v) {
    const FuseView& V = views.v[v];
    const float cx = ((V.P[0] * px + V.P[1] * py) + V.P[2] * pz) + V.P[3];
    const float cy = ((V.P[4] * px + V.P[5] * py) + V.P[6] * pz) + V.P[7];
    const float cz = ((V.P[8] * px + V.P[9] * py) + V.P[10] * pz) + V.P[11];
    if (!(cz > 0.0f)) continue;
    const float rx = rintf(cx / cz), ry = rintf(cy / cz);
    if (!(rx >= 0.0f && rx <= (float)(V.W - 1) && ry >= 0.0f && ry <= (float)(V.H - 1))) continue;
    const int64_t pix = (int64_t)(int)ry * V.W + (int)rx;
    const float d = V.depth[pix] * V.dscale;
    if (!(d > 0.0f && d <= FLT_MAX)) continue;
    const float diff = d - cz;
    if (!(diff >= -trunc)) continue;
    const float t = fminf(diff / trunc, 1.0f);
    const float wn = w + 1.0f;
    ts = (ts * w + t) / wn;
    if (COLOR) {
      c0 = (c0 * w + V.image[pix * 3 + 0]) / wn;
      c1 = (c1 * w + V.image[pix * 3 + 1]) / wn;
      c2 = (c2 * w + V.image[pix * 3 + 2]) / wn;
    }
    w = wn;
  }
  if (w == w0) return;                            // no view observed the point: its state is unchanged, nothing to write
  tsdf[i] = ts;
  weight[i] = w;
  if (COLOR) { color[i * 3 + 0] = c0; color[i * 3 + 1] = c1; color[i * 3 + 2] = c2; }
}

// The colour of mesh vertex t (lattice-index units, float64), which lies on one edge of the (nx, ny, nz) lattice: interpolated
// between the edge's two lattice points and quantised.  colors.locate(x, y, z) = where a lattice point's colour is kept,
// colors.read(where, c) = its channel c.
template <class Colors>
__device__ __forceinline__ void surf_fuse_vertex_color(const double* __restrict__ vertices, int64_t t, int nx, int ny, int nz,
                                                       const Colors& colors, uint8_t* __restrict__ out) {
  const int dims[3] = {nx, ny, nz};
  int lo[3], axis = 0;
  float f = 0.0f;
  bool found = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = vertices[t * 3 + a];
    const double fl = fmin(fmax(floor(v), 0.0), (double)(dims[a] - 1));    // a NaN coordinate lands on 0: every read stays inside
    lo[a] = (int)fl;
    const double fr = v - fl;
    if (!found && fr != 0.0) { found = true; axis = a; f = (float)fr; }
  }
  int hi[3] = {lo[0], lo[1], lo[2]};
  hi[axis] = min(lo[axis] + 1, dims[axis] - 1);
  const int64_t a_lo = colors.locate(lo[0], lo[1], lo[2]), a_hi = colors.locate(hi[0], hi[1], hi[2]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float cl = colors.read(a_lo, c), ch = colors.read(a_hi, c);
    float q = (cl + (ch - cl) * f) * 256.0f;
    q = fminf(fmaxf(q, 0.0f), 255.0f);
    out[t * 3 + c] = (uint8_t)q;
  }
}
