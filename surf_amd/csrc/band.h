// The brick layout of a band, ONE copy for mesh_band.hip, fuse_sparse.hip and ray_cast.hip: the lattice is cut into bricks of 8^3
// points, nbp bricks per axis; brick ids are linear, (bx nbp + by) nbp + bz (< 2^31, the entry points check it); the table maps an
// id to a slot or -1, and values are brick-major: slot * 512 + (lx << 6 | ly << 3 | lz).  Also the finiteness test and the
// observed-corner classification that mcubes.hip (dense lattice) and fuse_sparse.hip (band) share.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"

__device__ __forceinline__ bool surf_finite_f(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN and +-inf

// id of brick (bx, by, bz); band_brick_of: of the brick that holds lattice point (x, y, z).  I = the integer type the id is
// computed in: an id fits int32, so int is enough where the resolution is checked against SURF_BAND_MAX_RES (mesh_band.hip);
// int64_t costs a few instructions more and needs no such argument.
template <class I = int64_t>
__device__ __forceinline__ I band_brick_id(int nbp, int bx, int by, int bz) { return ((I)bx * nbp + by) * nbp + bz; }
template <class I = int64_t>
__device__ __forceinline__ I band_brick_of(int nbp, int x, int y, int z) { return band_brick_id<I>(nbp, x >> 3, y >> 3, z >> 3); }
__device__ __forceinline__ int band_local(int x, int y, int z) { return ((x & 7) << 6) | ((y & 7) << 3) | (z & 7); }
__device__ __forceinline__ void band_brick_xyz(int nbp, int id, int& bx, int& by, int& bz) {
  bz = id % nbp;
  by = (id / nbp) % nbp;
  bx = id / (nbp * nbp);
}
// lattice point of local index l (0 .. 511) of brick id
__device__ __forceinline__ void band_point_xyz(int nbp, int id, int l, int& x, int& y, int& z) {
  int bx, by, bz;
  band_brick_xyz(nbp, id, bx, by, bz);
  x = bx * 8 + (l >> 6);
  y = by * 8 + ((l >> 3) & 7);
  z = bz * 8 + (l & 7);
}

// band position of lattice point (x, y, z) (inside the lattice), or -1 when its brick is not in the table; D has a member nbp
// and a type id_t (the I above)
template <class D>
__device__ __forceinline__ int64_t band_pos(const D& d, const int32_t* __restrict__ table, int x, int y, int z) {
  const int32_t s = table[band_brick_of<typename D::id_t>(d.nbp, x, y, z)];
  return s < 0 ? (int64_t)-1 : (int64_t)s * 512 + band_local(x, y, z);
}
// (a missing brick reads NaN, which is never inside and never finite)
template <class D>
__device__ __forceinline__ float band_val(const D& d, const int32_t* __restrict__ table, const float* __restrict__ vals, int x, int y,
                                          int z) {
  const int64_t p = band_pos(d, table, x, y, z);
  return p < 0 ? __builtin_nanf("") : vals[p];
}

// The flag byte of marching cubes on a lattice with unobserved (non-finite) points, for the point (x, y, z) of value v0 of an
// (nx, ny, nz) lattice: bits 0-2 = sign change along x / y / z from this point, only where both end points are finite; bits 3-5 =
// ntri[case] of the cell whose origin it is, only where its eight corners are.  at(x, y, z) fetches a lattice value.
template <class Fetch>
__device__ __forceinline__ unsigned surf_classify_observed(int x, int y, int z, int nx, int ny, int nz, float v0, double iso,
                                                           Fetch at, const int8_t (&ntri)[256]) {
  const bool hx = x + 1 < nx, hy = y + 1 < ny, hz = z + 1 < nz;
  const float v1 = hx ? at(x + 1, y, z) : v0, v3 = hy ? at(x, y + 1, z) : v0, v4 = hz ? at(x, y, z + 1) : v0;
  const bool ok0 = surf_finite_f(v0), in0 = (double)v0 <= iso;
  unsigned f = 0;
  if (hx && ok0 && surf_finite_f(v1) && ((double)v1 <= iso) != in0) f |= 1u;
  if (hy && ok0 && surf_finite_f(v3) && ((double)v3 <= iso) != in0) f |= 2u;
  if (hz && ok0 && surf_finite_f(v4) && ((double)v4 <= iso) != in0) f |= 4u;
  if (hx && hy && hz && ok0) {
    float c[8];
    c[0] = v0; c[1] = v1; c[3] = v3; c[4] = v4;
    c[2] = at(x + 1, y + 1, z);
    c[5] = at(x + 1, y, z + 1);
    c[6] = at(x + 1, y + 1, z + 1);
    c[7] = at(x, y + 1, z + 1);
    unsigned cs = 0;
    bool all = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      all = all && surf_finite_f(c[k]);
      cs |= ((double)c[k] <= iso ? 1u : 0u) << k;
    }
    if (all) f |= (unsigned)ntri[cs] << 3;
  }
  return f;
}
