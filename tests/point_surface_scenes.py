"""Scenes and the float64 restatement shared by tests/test_point_surface_host.py and tests/test_point_surface_gpu.py.

The restatement knows nothing of bricks, keys or order: per lattice node, the points within R come from cKDTree.query_ball_point in
float64 and the sums are numpy's.  restate(..., dtype=np.float32) repeats it with the pair arithmetic in fp32 (its sums in the tree's
order, not the rule's): the largest difference between the two is E, the scale the tolerances on the mirror are multiples of
(the convention of tests/test_ray_composite_kernels.py)."""
import functools
from collections import namedtuple

import numpy as np

from surf_amd.fusion import lattice_axes

Lattice = namedtuple("Lattice", "axes lo voxel shape")
Restated = namedtuple("Restated", "count f sw color ambiguous")
Restated.__doc__ = """Dense (nx, ny, nz) arrays: count of admitted points, f = sum w g / sum w (0 where count == 0), sw, color
(nx, ny, nz, 3) or None, ambiguous: some float64 d2 lies within fp32 rounding of R2 (the admission may differ from fp32's)."""

WORLD_CENTRE = (300.0, -150.0, 600.0)
CENTRES = {"origin": (0.0, 0.0, 0.0), "world": WORLD_CENTRE}
SPHERE_R = 0.4
AMBIGUOUS_REL = 8.0 * 2.0 ** -24     # d2 in fp32: a difference and three products / sums, each good to 2^-24 relative


def lattice(lo, hi, voxel):
    lo = np.asarray(lo, np.float64)
    axes = lattice_axes(lo, hi, voxel)
    return Lattice(axes, lo, float(voxel), tuple(len(a) for a in axes))


def fibonacci_sphere(n, r=SPHERE_R, centre=(0.0, 0.0, 0.0)):
    """(points, unit normals) fp32 of n Fibonacci samples of a sphere; built in float64 and rounded once."""
    i = np.arange(n) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / n)
    th = np.pi * (1.0 + 5.0 ** 0.5) * i
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)
    return (np.asarray(centre, np.float64) + r * d).astype(np.float32), d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_scene(where="origin", side=23):
    """The 1000-point sphere of radius 0.4 on a side^3 lattice over [-0.78, 0.78]^3 about the centre: voxel 1.56 / 22 = 0.0709,
    about the sample spacing."""
    c = np.asarray(CENTRES[where], np.float64)
    P, N = fibonacci_sphere(1000, SPHERE_R, c)
    return P, N, lattice(c - 0.78, c + 0.78, 1.56 / (side - 1))


@functools.lru_cache(maxsize=None)
def plane_scene():
    """3000 points on z = 0.125 over [0, 1]^2 with normals (0, 0, 1); voxel 1 / 32 (the plane is a lattice plane)."""
    g = np.random.default_rng(5)
    P = np.concatenate([g.uniform(0.0, 1.0, (3000, 2)), np.full((3000, 1), 0.125)], axis=1).astype(np.float32)
    N = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (3000, 1))
    return P, N, lattice((0.0, 0.0, -0.125), (1.0, 1.0, 0.375), 1.0 / 32)


def restate(points, normals, colors, lat, radius, dtype=np.float64):
    """The rule's node sums without bricks or order (module docstring).  Points take part by rule 1."""
    from scipy.spatial import cKDTree
    P, N = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    part = np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & (N != 0).any(axis=1)
    # rule 2's far points are dropped too: they are admitted nowhere, but overflow the tree's arithmetic
    part &= (np.abs(np.where(np.isfinite(P), P, 0)) < 1e6).all(axis=1)
    P, N = P[part], N[part]
    C = None if colors is None else (np.asarray(colors)[part].astype(np.float64) + 0.5) / 256.0
    shape = lat.shape
    X = np.stack(np.meshgrid(*lat.axes, indexing="ij"), axis=-1).reshape(-1, 3)          # fp32 node coordinates
    R32 = np.float32(radius)
    R2 = float(R32 * R32)
    count, f, sw = np.zeros(len(X), np.int64), np.zeros(len(X)), np.zeros(len(X))
    col = None if C is None else np.zeros((len(X), 3))
    amb = np.zeros(len(X), bool)
    if len(P):
        balls = cKDTree(P.astype(np.float64)).query_ball_point(X.astype(np.float64), float(R32) * (1.0 + 1e-4))
        lens = np.fromiter((len(b) for b in balls), np.int64, len(X))
        row = np.repeat(np.arange(len(X)), lens)
        colj = np.fromiter((j for b in balls for j in b), np.int64, int(lens.sum()))
        d = X[row].astype(dtype) - P[colj].astype(dtype)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        adm = d2 < dtype(R2)
        d64 = X[row].astype(np.float64) - P[colj].astype(np.float64)
        near = np.abs((d64 ** 2).sum(axis=1) - R2) <= AMBIGUOUS_REL * R2
        t = dtype(1.0) - d2 * (dtype(1.0) / dtype(R2))
        w = np.where(adm, (t * t) * (t * t), dtype(0.0))
        n = N[colj].astype(dtype)
        g = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        count = np.bincount(row[adm], minlength=len(X))
        acc = (lambda v: np.bincount(row, weights=v, minlength=len(X))) if dtype is np.float64 else (lambda v: _add_at(row, v, len(X)))
        sw = acc(w).astype(np.float64)
        sf = acc(np.where(adm, w * g, dtype(0.0))).astype(np.float64)
        f = np.where(sw > 0, sf / np.where(sw > 0, sw, 1.0), 0.0)
        if C is not None:
            col = np.stack([acc(w * C[colj, ch].astype(dtype)).astype(np.float64) / np.where(sw > 0, sw, 1.0) for ch in range(3)], axis=1)
        amb = np.bincount(row[near], minlength=len(X)) > 0
    return Restated(count.reshape(shape), f.reshape(shape), sw.reshape(shape), None if col is None else col.reshape(shape + (3,)),
                    amb.reshape(shape))


def _add_at(row, v, n):
    out = np.zeros(n, v.dtype)
    np.add.at(out, row, v)                                  # sequential in pair order, in v's own precision
    return out


def dense(state, shape):
    """Brick-major state (bricks, table, tsdf, weight, color) -> dense (tsdf, weight, color or None, allocated) arrays of the
    lattice `shape`; an unallocated node reads 0 and allocated == False."""
    bricks, table, tsdf, weight, color = (None if x is None else np.asarray(x) for x in state)
    nbp = (max(shape) + 7) // 8
    I, J, K = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    slot = table[((I >> 3) * nbp + (J >> 3)) * nbp + (K >> 3)].astype(np.int64)
    have = slot >= 0
    pos = np.where(have, slot * 512 + (((I & 7) << 6) | ((J & 7) << 3) | (K & 7)), 0)
    pick = lambda a: np.where(have if a.ndim == 1 else have[..., None], a[pos], 0) if len(a) else np.zeros(shape + a.shape[1:], a.dtype)
    return pick(tsdf), pick(weight), None if color is None else pick(color), have
