// The round-trip rule of multi-view geometric consistency, ONE copy for depth_filter.hip (which counts the agreeing sources of a
// pixel) and point_cloud.hip (which marks the source pixels an emitted point stands for).  The operations, their order and the
// thresholds are written out in depth_filter.hip's header comment; the library is compiled with -ffp-contract=off, so every
// operator below is one fp32 operation.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"

struct FilterSource {
  float A_rs[9], b_rs[3], A_sr[9], b_sr[3];
  const float* depth;
  int H, W;
  float dscale;
  int pad;
};
struct FilterSources { FilterSource s[SURF_FUSE_MAX_VIEWS]; };

__device__ __forceinline__ bool surf_measured(float d) { return d > 0.0f && d <= FLT_MAX; }

// Does source S agree with the reference pixel (xf, yf) of measured depth d (q = (xf d, yf d, d))?  On agreement *wz is the
// back-projected depth w.z and (*sx, *sy) the pixel's projection into the source, 0 <= sx <= Ws-1 and 0 <= sy <= Hs-1.
__device__ __forceinline__ bool surf_consistency_rule(const FilterSource& S, float xf, float yf, float d, float qx, float qy,
                                                      float qz, float px2, float rel_thresh, float* wz_out, float* sx_out,
                                                      float* sy_out) {
  const float ux = ((S.A_rs[0] * qx + S.A_rs[1] * qy) + S.A_rs[2] * qz) + S.b_rs[0];
  const float uy = ((S.A_rs[3] * qx + S.A_rs[4] * qy) + S.A_rs[5] * qz) + S.b_rs[1];
  const float uz = ((S.A_rs[6] * qx + S.A_rs[7] * qy) + S.A_rs[8] * qz) + S.b_rs[2];
  if (!(uz > 0.0f)) return false;
  const float sx = ux / uz, sy = uy / uz;
  if (!(sx >= 0.0f && sx <= (float)(S.W - 1) && sy >= 0.0f && sy <= (float)(S.H - 1))) return false;
  const float x0f = floorf(sx), y0f = floorf(sy);
  const float fx = sx - x0f, fy = sy - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;                     // 0 <= x0 <= Ws-1, 0 <= y0 <= Hs-1 by the test above
  const int x1 = min(x0 + 1, S.W - 1), y1 = min(y0 + 1, S.H - 1);
  const int64_t r0 = (int64_t)y0 * S.W, r1 = (int64_t)y1 * S.W;
  const float d00 = S.depth[r0 + x0] * S.dscale, d01 = S.depth[r0 + x1] * S.dscale;
  const float d10 = S.depth[r1 + x0] * S.dscale, d11 = S.depth[r1 + x1] * S.dscale;
  if (!(surf_measured(d00) && surf_measured(d01) && surf_measured(d10) && surf_measured(d11))) return false;
  const float top = d00 + (d01 - d00) * fx;
  const float bot = d10 + (d11 - d10) * fx;
  const float ds = top + (bot - top) * fy;
  const float vx = sx * ds, vy = sy * ds, vz = ds;
  const float wx = ((S.A_sr[0] * vx + S.A_sr[1] * vy) + S.A_sr[2] * vz) + S.b_sr[0];
  const float wy = ((S.A_sr[3] * vx + S.A_sr[4] * vy) + S.A_sr[5] * vz) + S.b_sr[1];
  const float wz = ((S.A_sr[6] * vx + S.A_sr[7] * vy) + S.A_sr[8] * vz) + S.b_sr[2];
  if (!(wz > 0.0f)) return false;
  const float ex = wx / wz - xf, ey = wy / wz - yf;
  const float e2 = ex * ex + ey * ey;
  const float rel = fabsf(wz - d) / d;
  if (!(e2 < px2 && rel < rel_thresh)) return false;
  *wz_out = wz;
  *sx_out = sx;
  *sy_out = sy;
  return true;
}

// The host side of a launch's source table (surf_depth_consistency's h_T / h_depths / h_hw / h_dscale): 0, SURF_E_ARG or SURF_E_LIMIT.
inline int surf_fill_filter_sources(FilterSources& sources, const float* h_T, const float* const* h_depths, const int* h_hw,
                                    const float* h_dscale, int n_sources) {
  const int side_max = 1 << 24;                                 // (float)(side - 1) is exact: the bounds test keeps every tap inside
  for (int s = 0; s < n_sources; ++s) {
    FilterSource& S = sources.s[s];
    const int Hs = h_hw[2 * s], Ws = h_hw[2 * s + 1];
    if (!h_depths[s] || Hs < 1 || Ws < 1) return SURF_E_ARG;
    if ((int64_t)Hs * Ws >= ((int64_t)1 << 31) || Hs > side_max || Ws > side_max) return SURF_E_LIMIT;
    const float* T = h_T + 24 * s;
    for (int e = 0; e < 9; ++e) { S.A_rs[e] = T[e]; S.A_sr[e] = T[12 + e]; }
    for (int e = 0; e < 3; ++e) { S.b_rs[e] = T[9 + e]; S.b_sr[e] = T[21 + e]; }
    S.depth = h_depths[s];
    S.H = Hs;
    S.W = Ws;
    S.dscale = h_dscale[s];
    S.pad = 0;
  }
  for (int s = n_sources; s < SURF_FUSE_MAX_VIEWS; ++s) sources.s[s] = FilterSource{};
  return 0;
}
