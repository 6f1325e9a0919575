"""The host path of the mesh deviation (surf_amd/mesh_distance.py): the pair rule of include/surf_hip.h against an independent
fp64 formulation, the cell-table walk against brute force over all faces to the bit, and the geometry of the result.  No GPU."""
import math
import os

import numpy as np
import pytest

from surf_amd import _lib
from surf_amd import mesh_distance as md
from surf_amd.mesh_smooth import smooth_mesh
from tests.mesh_distance_scenes import REGION_MAX_DIST, REGION_QUERIES, REGION_TRIANGLE, mixed_scene, queries
from tests.mesh_smooth_scenes import MESHES, noisy_sphere
from tests.test_mesh_simplify_host import uv_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["surf_meshdist_pairs_count", "surf_meshdist_pairs_emit", "surf_meshdist_query"]
INT32_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    for g, w, part in zip(got, want, ("distance", "face", "closest")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part)
        same = np.array_equal(bits(g), bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, (what, part, int((g != w).sum()))


# ---- the library ----------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    """Fails on the parent commit: the surf_meshdist_* group is new.  The ABI version stays 41 (entry points added, none changed)."""
    with open(os.path.join(ROOT, "include", "surf_hip.h")) as f:
        header = f.read()
    assert "#define SURF_ABI_VERSION 41" in header and _lib.ABI_VERSION == 41
    L = _lib.lib()
    assert L.surf_abi_version() == 41
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name


def test_limits_and_arguments_are_reported_before_any_launch():
    from surf_amd import ops
    L = _lib.lib()
    big = INT32_MAX + 1
    table = (0.0, 0.0, 0.0, 0.5, 4, 4, 4)
    assert (ops.MESHDIST_MAX_AXIS_CELLS, ops.MESHDIST_MAX_CELLS, ops.MESHDIST_PAIRS_PER_FACE) == (4096, 2 ** 26, 8)
    for call in (lambda: L.surf_meshdist_pairs_count(None, big, None, 10, *table, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, big, *table, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, 0.0, 0.0, 0.0, 0.5, 4097, 1, 1, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, 0.0, 0.0, 0.0, 0.5, 4096, 4096, 5, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, big, *table, None, 10, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, 10, *table, None, big, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, 10, 0.0, 0.0, 0.0, 0.5, 1, 4097, 1, None, 10, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, big, None, 10, None, *table, 1.0, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, big, None, *table, 1.0, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, 0.0, 0.0, 0.0, 0.5, 1, 1, 4097, 1.0, None, None, None,
                                               None)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            call()
    nan, inf = float("nan"), float("inf")
    for call in (lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, *table, None, None, None),              # null pointers
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, 0.0, 0.0, 0.0, 0.0, 4, 4, 4, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, 0.0, 0.0, 0.0, inf, 4, 4, 4, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, nan, 0.0, 0.0, 0.5, 4, 4, 4, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, 10, None, 10, 0.0, 0.0, 0.0, 0.5, 4, 0, 4, None, None, None),
                 lambda: L.surf_meshdist_pairs_count(None, -1, None, 10, *table, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, 10, *table, None, 10, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, 10, *table, None, -1, None, None, None),
                 lambda: L.surf_meshdist_pairs_emit(None, 10, 0.0, 0.0, 0.0, -0.5, 4, 4, 4, None, 10, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, *table, 1.0, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, *table, 0.0, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, *table, -1.0, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, *table, inf, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, *table, nan, None, None, None, None),
                 lambda: L.surf_meshdist_query(None, None, 10, None, 10, None, 0.0, 0.0, 0.0, nan, 4, 4, 4, 1.0, None, None, None,
                                               None)):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            call()
    assert L.surf_meshdist_pairs_count(None, 10, None, 0, *table, None, None, None) == 0                        # empty: at once
    assert L.surf_meshdist_pairs_emit(None, 0, *table, None, 0, None, None, None) == 0
    assert L.surf_meshdist_query(None, None, 0, None, 10, None, *table, 1.0, None, None, None, None) == 0
    for bad in (0.0, -1.0, inf, nan, "x"):
        with pytest.raises(ValueError, match="max_dist"):
            md.point_to_mesh(REGION_QUERIES, *REGION_TRIANGLE, max_dist=bad)


# ---- the pair rule --------------------------------------------------------------------------------------------------------------

def _segment_distance2(p, a, b):
    ab = b - a
    L2 = np.einsum("ij,ij->i", ab, ab)
    t = np.clip(np.einsum("ij,ij->i", p - a, ab) / np.where(L2 > 0, L2, 1.0), 0.0, 1.0)
    e = p - (a + ab * t[:, None])
    return np.einsum("ij,ij->i", e, e)


def independent_distance(p, a, b, c):
    """A second fp64 formulation that shares nothing with the region scheme: the distance to the plane where the projection falls
    inside the triangle (three signed areas of one sign), otherwise the least of the three clamped segment distances."""
    n = np.cross(b - a, c - a)
    nn = np.einsum("ij,ij->i", n, n)
    h = np.einsum("ij,ij->i", p - a, n) / np.where(nn > 0, nn, 1.0)
    q = p - n * h[:, None]                                                         # the projection onto the plane
    areas = [np.einsum("ij,ij->i", np.cross(u - q, w - q), n) for u, w in ((a, b), (b, c), (c, a))]
    inside = (nn > 0) & (areas[0] >= 0) & (areas[1] >= 0) & (areas[2] >= 0)
    edges = np.minimum(np.minimum(_segment_distance2(p, a, b), _segment_distance2(p, b, c)), _segment_distance2(p, c, a))
    return np.where(inside, np.abs(h) * np.sqrt(nn), np.sqrt(edges))


def _triangles(kind, count, g):
    if kind == "random":
        return g.uniform(-1, 1, (count, 3, 3))
    if kind == "small":                                                            # 2 % of the box
        return g.uniform(-0.98, 0.98, (count, 1, 3)) + g.uniform(-0.02, 0.02, (count, 3, 3))
    along = g.standard_normal((count, 3))                                          # needles of aspect 1e3
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    across = np.cross(along, g.standard_normal((count, 3)))
    across /= np.linalg.norm(across, axis=1, keepdims=True)
    a = g.uniform(-0.5, 0.5, (count, 3))
    L = g.uniform(0.1, 0.5, (count, 1))
    return np.stack([a, a + along * L, a + along * L * g.uniform(0.2, 0.8, (count, 1)) + across * L * 1e-3], axis=1)


@pytest.mark.parametrize("kind", ["random", "small", "needle"])
def test_pair_rule_against_an_independent_formulation(kind):
    """|distance difference| <= 1e-12 for coordinates in [-1, 1]; half of the queries lie within 1e-3 of their triangle."""
    g = np.random.default_rng({"random": 1, "small": 2, "needle": 3}[kind])
    count = 100000
    tri = _triangles(kind, count, g).astype(np.float32).astype(np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    w = g.dirichlet([1, 1, 1], count)
    w[::4] = g.dirichlet([0.3, 0.3, 0.3], count)[::4] * 1.5 - 0.25                 # some outside the triangle, near edges and corners
    on = a * w[:, :1] + b * w[:, 1:2] + c * w[:, 2:]
    p = np.where((np.arange(count) % 2 == 0)[:, None], on + g.uniform(-1e-3, 1e-3, (count, 3)) / math.sqrt(3.0),
                 g.uniform(-1, 1, (count, 3))).astype(np.float32).astype(np.float64)
    q, cs, region = md.pair_rule(p, a, b, c)
    assert not np.isnan(q).any() and np.isfinite(cs).all()
    assert sorted(np.unique(region).tolist()) == list(range(7)), np.bincount(region, minlength=7)
    diff = np.abs(np.sqrt(q) - independent_distance(p, a, b, c))
    print(kind, "largest difference", diff.max(), "regions", np.bincount(region, minlength=7).tolist())
    assert diff.max() <= 1e-12


def test_pair_rule_on_the_region_triangle_and_on_degenerate_faces():
    v, _ = REGION_TRIANGLE
    a, b, c = (np.repeat(v[i:i + 1].astype(np.float64), 7, axis=0) for i in range(3))
    q, cs, region = md.pair_rule(REGION_QUERIES[:7].astype(np.float64), a, b, c)
    assert region.tolist() == list(range(7))
    want_cs = [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]]
    assert np.array_equal(cs, np.array(want_cs, np.float64))
    assert q.tolist() == [2.25, 1.5, 1.25, 1.5, 1.25, 0.75, 0.25]
    # exact degenerate faces, hand-computed: a == b is the segment a-c, a == b == c a point, collinear corners the segment a-c
    o, x2, x1 = np.array([[0.0, 0, 0]]), np.array([[2.0, 0, 0]]), np.array([[1.0, 0, 0]])
    cases = [(o, o, x2, [1, 1, 0], 1.0, [1, 0, 0]), (o, o, x2, [-3, 0, 4], 25.0, [0, 0, 0]), (o, o, x2, [3, 0, 1], 2.0, [2, 0, 0]),
             (o, x2, x2, [1, 2, 0], 4.0, [1, 0, 0]), (o, x2, o, [0.5, 0, 2], 4.0, [0.5, 0, 0]), (o, x2, x2, [4, 0, 0], 4.0, [2, 0, 0]),
             (x1, x1, x1, [1, 2, 2], 8.0, [1, 0, 0]), (o, x1, x2, [1.5, 1, 0], 1.0, [1.5, 0, 0]), (o, x2, x1, [1.5, 0, 2], 4.0, [1.5, 0, 0]),
             (o, x1, x2, [-1, 0, 0], 1.0, [0, 0, 0]), (x1, o, x2, [2.5, 0, 1], 1.25, [2, 0, 0]), (x1, o, x2, [0.25, 3, 0], 9.0, [0.25, 0, 0])]
    for a, b, c, p, want_q, want_c in cases:
        q, cs, _ = md.pair_rule(np.array([p], np.float64), a, b, c)
        assert q[0] == want_q and cs[0].tolist() == want_c, (a, b, c, p, q, cs)


# ---- the table walk against brute force -------------------------------------------------------------------------------------------

def _walk_queries(v, f, g):
    v64 = v.astype(np.float64)
    size = float(np.ptp(v64, axis=0).max()) or 1.0
    mid = (v64.min(axis=0) + v64.max(axis=0)) / 2
    some = f[g.integers(0, len(f), 40)]
    parts = [v[np.unique(f)[:80]], (v64[some[:, 0]] + v64[some[:, 1]]) / 2, v64[some].mean(axis=1), queries(v, f, 150, 3),
             mid + 0.3 * size * g.standard_normal((40, 3)), mid + g.choice([-1.0, 1.0], (12, 3)) * g.uniform(20, 60, (12, 3)) * size]
    return np.concatenate(parts).astype(np.float32)


def test_table_walk_equals_all_faces_on_the_noisy_sphere():
    """Distance bits, face index and closest-point bits, for three cell sizes a factor 8 apart end to end and the default one,
    with max_dist large and with max_dist equal to one query's own distance, which is below the sphere's radius."""
    v, f = noisy_sphere(24, 32)
    g = np.random.default_rng(0)
    q = _walk_queries(v, f, g)
    want = md.point_to_mesh_all_faces(q, v, f, 10.0)
    inner = np.flatnonzero((want[0] > 0.25) & (want[0] < 0.5))[0]
    cap = float(want[0][inner])                                                    # that query is at exactly max_dist: +inf
    want_cap = md.point_to_mesh_all_faces(q, v, f, cap)
    assert np.isinf(want_cap[0][inner]) and want_cap[1][inner] == -1 and np.isinf(want_cap[2][inner]).all()
    assert 0 < np.isinf(want_cap[0]).sum() < len(q) and np.isfinite(want[0][:160]).all() and np.isinf(want[0][-12:]).all()
    assert np.array_equal(np.isinf(want_cap[0]), ~(want[0] < cap))
    for cell in (None, 0.05, 0.13, 0.4):
        stats = {}
        assert_same(md.point_to_mesh_host(q, v, f, 10.0, _cell=cell, stats=stats), want, ("large", cell))
        assert cell is None or stats["cell"] == cell
        assert_same(md.point_to_mesh_host(q, v, f, cap, _cell=cell), want_cap, ("capped", cell))
    # exact ties between faces go to the smaller index: the queries on vertices are at distance 0 from every face around them
    a, b, c = md._corners(v, f)
    ties = 0
    for i in range(80):
        pair_q = md.pair_rule(np.repeat(q[i:i + 1].astype(np.float64), len(f), axis=0), a, b, c)[0]
        at = np.flatnonzero(pair_q == pair_q.min())
        ties += len(at) > 1
        assert want[1][i] == at[0] and want[0][i] == math.sqrt(pair_q.min())
    assert ties >= 40


@pytest.mark.parametrize("name", [n for n in MESHES if len(MESHES[n][1]) <= 6000])
def test_table_walk_equals_all_faces_on_the_small_meshes(name):
    v, f = MESHES[name]
    q = _walk_queries(v, f, np.random.default_rng(len(name)))
    want = md.point_to_mesh_all_faces(q, v, f)
    assert_same(md.point_to_mesh_host(q, v, f), want, name)
    size = float(np.ptp(v.astype(np.float64), axis=0).max())
    assert_same(md.point_to_mesh_host(q, v, f, 0.2 * size), md.point_to_mesh_all_faces(q, v, f, 0.2 * size), (name, "capped"))
    near = np.flatnonzero(want[0] < 0.5 * size)[:150]                              # far queries walk hundreds of shells of small cells
    for share in (0.05, 0.14, 0.4):                                                # three cells a factor 8 apart end to end
        got = md.point_to_mesh_host(q[near], v, f, md.joint_diagonal(q, v), _cell=share * size)
        assert_same(got, tuple(w[near] for w in want), (name, "cell", share))
    assert_same(md.point_to_mesh_host(q, v, f, _cell=0.31 * size), want, (name, "coarse"))


def test_mixed_scene_with_degenerate_faces():
    v, f = mixed_scene()
    q = _walk_queries(v, f, np.random.default_rng(4))
    want = md.point_to_mesh_all_faces(q, v, f)
    assert_same(md.point_to_mesh_host(q, v, f), want, "mixed")
    a, b, c = md._corners(v, f)
    every = md.pair_rule(np.repeat(q.astype(np.float64), len(f), axis=0), np.tile(a, (len(q), 1)), np.tile(b, (len(q), 1)),
                         np.tile(c, (len(q), 1)))[0]
    assert not np.isnan(every).any()
    assert set(want[1].tolist()) & {1, 3, 4, 5, 6}                                 # degenerate faces do answer queries


# ---- geometry -----------------------------------------------------------------------------------------------------------------------

def test_height_above_a_face_is_the_distance():
    v, f = REGION_TRIANGLE
    for h in (0.5, 3.0, 1e-3, 0.1):
        h32 = float(np.float32(h))
        d, face, cs = md.point_to_mesh(np.array([[0.25, 0.25, h], [0.25, 0.5, -h]], np.float32), v, f)
        assert d.tolist() == [h32, h32] and face.tolist() == [0, 0] and cs.tolist() == [[0.25, 0.25, 0], [0.25, 0.5, 0]]
    d, face, cs = md.point_to_mesh(REGION_QUERIES, v, f, REGION_MAX_DIST)
    assert d[:7].tolist() == [1.5, math.sqrt(1.5), math.sqrt(1.25), math.sqrt(1.5), math.sqrt(1.25), math.sqrt(0.75), 0.5]
    assert d[7] == np.inf and face.tolist() == [0] * 7 + [-1] and np.isinf(cs[7]).all()


def test_points_against_a_fine_sphere():
    """Within the chord sagitta of ||p| - R|: the mesh is inscribed, and no point of a face is further inside than
    R - sqrt(R^2 - (L/2)^2 * 4/3) for the longest edge L (the circumradius of a face is at most L / sqrt(3))."""
    R = 1.0
    v, f = uv_sphere(96, 128)
    v64 = v.astype(np.float64)
    assert np.allclose(np.linalg.norm(v64, axis=1), R, atol=1e-6)
    L = max(np.linalg.norm(v64[f[:, i]] - v64[f[:, (i + 1) % 3]], axis=1).max() for i in range(3))
    sagitta = R - math.sqrt(R * R - L * L / 3.0)
    g = np.random.default_rng(8)
    d = g.standard_normal((2000, 3))
    p = (d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.5, 2.0, (2000, 1))).astype(np.float32)
    dist = md.point_to_mesh(p, v, f)[0]
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    excess = dist - np.abs(r - R)
    print("sagitta", sagitta, "excess", excess.min(), excess.max())
    assert 0 < sagitta < 1e-3 and (np.abs(excess) <= sagitta + 1e-6).all()          # 1e-6: the vertices are fp32
    assert (excess[r >= R] >= -1e-6).all() and excess.max() > 0.1 * sagitta         # the mesh is inside the sphere, and not on it


def test_deviation_of_a_mesh_against_itself_is_zero():
    v, f = noisy_sphere(24, 32)
    rec = md.mesh_deviation(v, f, v, f)
    zero = {"count": len(v), "beyond": 0, "max": 0.0, "mean": 0.0, "rms": 0.0}
    assert rec == {"forward": zero, "backward": zero, "hausdorff": 0.0}


def test_deviation_is_consistent_with_the_smoothing_movement():
    """B = smooth_mesh(A): every vertex of B started on A, so B's vertices lie within moved_max of A."""
    v, f = noisy_sphere(24, 32)
    b, _, info = smooth_mesh(v, f, iterations=5, pin_boundary=False)
    rec = md.mesh_deviation(v, f, b, f)
    assert 0 < rec["backward"]["max"] <= info["moved_max"] and rec["backward"]["mean"] <= rec["backward"]["rms"] <= rec["backward"]["max"]
    assert rec["forward"]["max"] > 0 and rec["hausdorff"] == max(rec["forward"]["max"], rec["backward"]["max"])
    assert rec["forward"]["beyond"] == rec["backward"]["beyond"] == 0
    step = md.deviation_step(v, f, b, f)
    assert {k: step[k] for k in rec} == rec and set(step) == set(rec) | {"max_dist", "ms"}
    assert step["max_dist"] == md.joint_diagonal(v, b)
    capped = md.mesh_deviation(v, f, b, f, max_dist=0.5 * rec["backward"]["max"])
    assert 0 < capped["backward"]["beyond"] < capped["backward"]["count"] and capped["backward"]["max"] < 0.5 * rec["backward"]["max"]


def test_unreferenced_vertices_are_not_queried_and_an_empty_face_list_finds_nothing():
    v, f = MESHES["unreferenced"]                                                  # vertices 3 and 4 are named by no face
    far = v.copy()
    far[3] = far[4] = [50, 50, 50]
    rec = md.mesh_deviation(far, f, v, f)
    assert rec["forward"] == {"count": 4, "beyond": 0, "max": 0.0, "mean": 0.0, "rms": 0.0} and rec["hausdorff"] == 0.0
    empty = md.mesh_deviation(v, f, v, f[:0])
    none = {"max": None, "mean": None, "rms": None}
    assert empty["forward"] == {"count": 4, "beyond": 4, **none} and empty["backward"] == {"count": 0, "beyond": 0, **none}
    assert empty["hausdorff"] is None
    d, face, cs = md.point_to_mesh(v, v, f[:0])
    assert np.isinf(d).all() and (face == -1).all() and np.isinf(cs).all()


def test_inputs_are_checked_like_the_smoothing_inputs():
    v, f = MESHES["two_triangles"]
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="vertex 2 is not finite"):
            md.point_to_mesh(v, bad, f)
        with pytest.raises(ValueError, match="point 2 is not finite"):
            md.point_to_mesh(bad, v, f)
        with pytest.raises(ValueError, match="vertex 2 is not finite"):
            md.mesh_deviation(v, f, bad, f)
    with pytest.raises(ValueError, match=r"face indices span \[0, 4\]"):
        md.point_to_mesh(v, v, np.array([[0, 1, 4]], np.int32))
    with pytest.raises(ValueError, match=r"face indices span \[-1, 2\]"):
        md.mesh_deviation(v, np.array([[0, -1, 2]], np.int32), v, f)
    with pytest.raises(RuntimeError, match="no host fall-back"):
        md.point_to_mesh(v, v, f, backend="device", device="cpu")
    with pytest.raises(ValueError, match="backend"):
        md.point_to_mesh(v, v, f, backend="gpu")
