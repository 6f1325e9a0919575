"""Scenes shared by tests/test_mesh_distance_host.py and tests/test_mesh_distance_gpu.py: meshes and query points that cross each
edge of the distance rule (include/surf_hip.h, surf_meshdist_*) and of the query kernel (one query per lane, 64 per wavefront, 256
per block).  The meshes of tests/mesh_smooth_scenes.py are used as they are."""
import numpy as np

from tests.mesh_smooth_scenes import MESHES, noisy_sphere

REGION_TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
# one query per region of the pair rule, in region order, and one far beyond REGION_MAX_DIST
REGION_QUERIES = np.array([[-1, -1, 0.5], [2, -0.5, 0.5], [0.5, -1, 0.5], [-0.5, 2, 0.5], [-1, 0.5, 0.5], [1, 1, 0.5],
                           [0.25, 0.25, 0.5], [40, -30, 25]], np.float32)
REGION_MAX_DIST = 8.0
QUERY_COUNTS = (1, 63, 64, 65, 257)


def spanning_scene():
    """One triangle that spans the whole box and 200 small ones inside it: the large face is listed in most cells of the table."""
    g = np.random.default_rng(5)
    centre = g.uniform(-0.9, 0.9, (200, 1, 3))
    small = (centre + g.uniform(-0.03, 0.03, (200, 3, 3))).reshape(-1, 3)
    v = np.concatenate([[[-1, -1, -1], [1, 1, -0.8], [-0.7, 1, 1]], small]).astype(np.float32)
    f = np.concatenate([[[0, 1, 2]], 3 + np.arange(600).reshape(200, 3)]).astype(np.int32)
    return v, f


def mixed_scene():
    """Ordinary faces among degenerate ones (a == b, b == c, a == c, a == b == c, collinear corners) and vertices no face names."""
    g = np.random.default_rng(6)
    v = g.uniform(-1, 1, (40, 3)).astype(np.float32)
    v[30], v[31], v[32] = [0, 0, 0], [0.25, 0.5, -0.25], [0.5, 1, -0.5]           # exactly collinear
    f = [[0, 1, 2], [3, 3, 4], [2, 1, 5], [6, 7, 7], [8, 9, 8], [10, 10, 10], [30, 31, 32], [30, 32, 31], [11, 12, 13], [13, 12, 14],
         [15, 16, 17], [5, 3, 18]]
    return v, np.array(f, np.int32)                                               # 19 .. 29 and 33 .. 39 are named by no face


def queries(v, f, count, seed=0, away_once=False):
    """`count` fp32 queries around the mesh (v, f): on vertices, on edge midpoints, on centroids, near the surface, anywhere in a
    box three times the mesh's, and far outside it - in that proportion, shuffled."""
    g = np.random.default_rng(seed)
    v64 = v.astype(np.float64)
    tri = v64[f[g.integers(0, len(f), count)]]
    lo, hi = v64.min(axis=0), v64.max(axis=0)
    size = max(float((hi - lo).max()), 1e-3)
    kinds = [v64[f.reshape(-1)[g.integers(0, 3 * len(f), count)]], (tri[:, 0] + tri[:, 1]) / 2, tri.mean(axis=1),
             tri.mean(axis=1) + g.normal(0, 0.02 * size, (count, 3)), g.uniform(lo - size, hi + size, (count, 3)),
             (lo + hi) / 2 + g.choice([-1.0, 1.0], (count, 3)) * g.uniform(4 * size, 9 * size, (count, 3))]
    # away_once: the two kinds away from the surface, whose walks are long, only once each (the large scene)
    pick = g.integers(0, 4 if away_once else len(kinds), count)
    pick[:min(count, len(kinds))] = np.arange(len(kinds))[:count]                 # every kind at least once where count allows
    out = np.stack(kinds)[pick, np.arange(count)]
    return out[g.permutation(count)].astype(np.float32)


def scenes():
    """name -> (vertices, faces) of the device == host comparison."""
    out = {"one_face": REGION_TRIANGLE}
    for name in ("two_triangles", "fan", "strip257", "grid", "noisy_sphere"):
        out[name] = MESHES[name]
    out["spanning"] = spanning_scene()
    out["mixed"] = mixed_scene()
    return out


def big_sphere():
    """About 115 k faces with radial noise and 20,000 queries on and near the surface (and one each far from it): 79 blocks of
    queries and cells of several records each, so that every loop of the query kernel makes second trips."""
    v, f = noisy_sphere(240, 240, 0.002, 2)
    return v, f, queries(v, f, 20000, 7, away_once=True)
