"""The cloud of tests/test_point_filter_host.py and tests/test_point_filter_gpu.py: 3649 fp32 points in six parts, each there for a
reason.  Built in float64, moved by `centre`, then rounded to fp32 once - so the lattice part stays exact at any centre whose
coordinates are multiples of 2^-7 of moderate size (at (300, -150, 600) fp32 spacing is 6e-5: a subtraction done in the wrong
order shows)."""
from collections import namedtuple

import numpy as np

Scene = namedtuple("Scene", "points parts centre")
Scene.__doc__ = """points (n, 3) fp32; parts: name -> slice of rows; centre (3,) float64 the cloud was moved by."""

LATTICE_STEP = 2.0 ** -7
SPHERE_CENTRE = np.array([0.25, 0.1875, 0.3125])         # multiples of 2^-7, like everything added to the lattice
SPHERE_RADIUS = 0.1
PAIR_GAP = 0.004
WORLD_CENTRE = (300.0, -150.0, 600.0)


def build(seed, centre=(0.0, 0.0, 0.0)):
    """plane: 48 x 40 points at 0.01 spacing, xy jitter +-0.002, z noise 2e-4 (a surface with sensor noise);
    sphere: 1500 points on a sphere of radius 0.1 (curvature; the normals' orientation);
    lattice: an EXACT 9 x 9 x 2 lattice at spacing 2^-7 (every value representable: equal d2 abound - the tie and stop rules);
    outliers: 60 uniform points in [-0.5, 1.5]^3;
    pair: two points 0.004 apart, far from everything (starved at k > 1);
    duplicates: 5 exact copies of plane points (distance 0 is an ordinary neighbour)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:40, :48].astype(np.float64)
    plane = np.stack([xx.reshape(-1) * 0.01, yy.reshape(-1) * 0.01, np.zeros(48 * 40)], axis=1)
    plane[:, :2] += g.uniform(-0.002, 0.002, (len(plane), 2))
    plane[:, 2] += g.normal(0.0, 2e-4, len(plane))
    d = g.normal(size=(1500, 3))
    sphere = SPHERE_CENTRE + SPHERE_RADIUS * d / np.linalg.norm(d, axis=1, keepdims=True)
    ix, iy, iz = np.mgrid[:9, :9, :2]
    lattice = np.array([0.75, 0.25, 0.5]) + LATTICE_STEP * np.stack([ix, iy, iz], axis=-1).reshape(-1, 3)
    outliers = g.uniform(-0.5, 1.5, (60, 3))
    pair = np.array([[2.0, 2.0, 2.0], [2.0 + PAIR_GAP, 2.0, 2.0]])
    dup = plane[g.choice(len(plane), 5, replace=False)]
    chunks = (("plane", plane), ("sphere", sphere), ("lattice", lattice), ("outliers", outliers), ("pair", pair), ("duplicates", dup))
    parts, at = {}, 0
    for name, c in chunks:
        parts[name] = slice(at, at + len(c))
        at += len(c)
    centre = np.asarray(centre, dtype=np.float64)
    points = (np.concatenate([c for _, c in chunks]) + centre).astype(np.float32)
    return Scene(points, parts, centre)


def with_bad_rows(scene):
    """(points with six rows of NaN / +inf / -inf put in at the front, in the middle and at the end, the indices of those rows)."""
    n = len(scene.points)
    at = np.array([0, 1000, 1000, 2500, n, n])
    bad = np.array([[np.nan, 0.1, 0.1], [0.2, np.inf, 0.0], [0.2, 0.2, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, 0.3],
                    [0.25, 0.19, np.nan]], dtype=np.float32)
    points = np.insert(scene.points, at, bad, axis=0)
    return points, np.flatnonzero(~np.isfinite(points).all(axis=1))
