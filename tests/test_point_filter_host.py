"""surf_amd/point_filter.py, backend="host": the numpy mirror of the rule written in include/surf_hip.h above surf_points_knn*,
against float64 brute force over all pairs, an fp32 brute force with np.lexsort (the exact (d2, j) order), float64 cKDTree
statistics and np.linalg.eigh.  No GPU.  The cloud is tests/point_filter_scenes.py's (3649 points), at the origin and in a world
frame near (300, -150, 600)."""
import functools

import numpy as np
import pytest
from scipy.spatial import cKDTree

from surf_amd import mesh_io, point_filter as PF
from surf_amd.fusion import DepthView, PointCloud
from tests import point_filter_scenes as S

CASES = ((1, 0.05), (8, 0.05), (16, 0.08))               # (k, max_dist): the issue's cases
CENTRES = {"origin": (0.0, 0.0, 0.0), "world": S.WORLD_CENTRE}


@functools.lru_cache(maxsize=None)
def scene(seed=0, where="origin"):
    return S.build(seed, CENTRES[where])


@functools.lru_cache(maxsize=None)
def host_knn(seed, where, k, md):
    return PF.knn_host(scene(seed, where).points, k, md)


@functools.lru_cache(maxsize=None)
def brute64(seed, where):
    """All pairs in float64: (distance (n, n) sorted along rows with the point itself taken out BY INDEX, the indices in that order)."""
    P = scene(seed, where).points.astype(np.float64)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    d[np.arange(len(P)), np.arange(len(P))] = np.inf
    order = np.argsort(d, axis=1, kind="stable")
    return np.take_along_axis(d, order, axis=1), order


def brute32(P, k, md):
    """Rule 1 by brute force in fp32: every pair's d2 in the rule's operation order, np.lexsort by (d2, j)."""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P)
    md2 = np.float32(md) * np.float32(md)
    index, d2, count = np.full((n, k), -1, np.int32), np.full((n, k), np.inf, np.float32), np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            dx, dy, dz = P[:, 0] - P[i, 0], P[:, 1] - P[i, 1], P[:, 2] - P[i, 2]
            dd = (dx * dx + dy * dy) + dz * dz
            ok = dd <= md2
            ok[i] = False
            j = np.flatnonzero(ok)
            j = j[np.lexsort((j, dd[j]))][:k]
            index[i, :len(j)], d2[i, :len(j)], count[i] = j, dd[j], len(j)
    return index, d2, count


@pytest.mark.parametrize("where", list(CENTRES))
@pytest.mark.parametrize("k,md", CASES)
def test_knn_against_float64_brute_force(where, k, md):
    """Counts, sorted distances (1e-6 relative) at every point; the index SETS wherever float64 separates the k-th from the
    (k+1)-th neighbour by more than 1e-6 relative.  Rows with a pair within 1e-6 relative of max_dist itself (fp32 may admit what
    float64 does not) are left out of the comparison; they must be rare."""
    index, d2, count = host_knn(0, where, k, md)
    d64, order = brute64(0, where)
    n = len(d64)
    within = d64 <= md
    ambiguous = (np.abs(d64 - md) <= 1e-6 * md).any(axis=1)
    # a condition on the inputs, not on the code: ~3e5 pairs lie within 0.05, evenly spread, so about one pair (two rows) is expected
    # inside a band of 2e-6 * 0.05
    assert ambiguous.mean() < 1e-2
    want = np.minimum(within.sum(axis=1), k)
    ok = ~ambiguous
    assert np.array_equal(count[ok], want[ok])
    cols = np.arange(k)[None, :] < count[:, None]
    assert np.array_equal(index >= 0, cols) and np.array_equal(np.isfinite(d2), cols)
    got = np.sqrt(d2.astype(np.float64))
    ref = d64[:, :k]
    sel = cols & ok[:, None]
    assert np.allclose(got[sel], ref[sel], rtol=1e-6, atol=0.0)
    nxt = np.where(within[:, k], d64[:, k], np.inf) if d64.shape[1] > k else np.full(n, np.inf)
    separated = ok & ((count < k) | (nxt - d64[:, k - 1] > 1e-6 * d64[:, k - 1]))
    assert separated.mean() > 0.9
    for i in np.flatnonzero(separated):
        assert set(index[i, :count[i]]) == set(order[i, :count[i]]), i
    assert not (index == np.arange(n)[:, None]).any()                     # nobody is their own neighbour


@pytest.mark.parametrize("where", list(CENTRES))
def test_exact_order_on_the_lattice(where):
    """The exact (d2, j) order, ties to the smaller index: against the fp32 brute force, array for array, on the whole cloud - and
    the lattice part does hold ties (a lattice point has equal d2 among its first 8 neighbours)."""
    sc = scene(0, where)
    for k, md in ((8, 0.05), (32, 0.08)):
        index, d2, count = PF.knn_host(sc.points, k, md)
        bi, bd, bc = brute32(sc.points, k, md)
        assert np.array_equal(count, bc) and np.array_equal(index, bi) and np.array_equal(d2, bd)
    lat = d2[sc.parts["lattice"]]
    assert (lat[:, 1:] == lat[:, :-1]).any(axis=1).all()
    assert np.array_equal(lat[:, 0], np.full(len(lat), np.float32(S.LATTICE_STEP) ** 2))


def test_starved_pair_and_duplicates():
    sc = scene()
    index, d2, count = host_knn(0, "origin", 8, 0.05)
    a, b = sc.parts["pair"].start, sc.parts["pair"].start + 1
    assert count[a] == 1 and count[b] == 1 and index[a, 0] == b and index[b, 0] == a
    assert np.all(index[a, 1:] == -1) and np.all(np.isinf(d2[a, 1:]))
    stat = PF.stat_host(d2, count)
    assert np.isposinf(stat[a]) and np.isposinf(stat[b])
    assert np.isfinite(stat[sc.parts["plane"]]).all()
    # a duplicate is an ordinary neighbour at distance 0, and the nearest of its original
    for i in range(sc.parts["duplicates"].start, sc.parts["duplicates"].stop):
        assert d2[i, 0] == 0.0 and np.array_equal(sc.points[index[i, 0]], sc.points[i]) and index[i, 0] != i
        assert d2[index[i, 0], 0] == 0.0 and index[index[i, 0], 0] == i
    # k = 1: the statistic is the nearest distance itself
    _, d1, c1 = host_knn(0, "origin", 1, 0.05)
    assert np.array_equal(PF.stat_host(d1, c1)[c1 == 1], np.sqrt(d1[c1 == 1, 0]))


def test_non_finite_rows():
    sc = scene()
    points, bad = S.with_bad_rows(sc)
    index, d2, count = PF.knn_host(points, 8, 0.05)
    assert len(bad) == 6 and np.all(count[bad] == 0) and np.all(index[bad] == -1)
    assert not np.isin(index, bad).any()
    good = np.setdiff1d(np.arange(len(points)), bad)
    ri, rd, rc = host_knn(0, "origin", 8, 0.05)
    assert np.array_equal(count[good], rc) and np.array_equal(d2[good], rd)
    assert np.array_equal(np.where(index[good] >= 0, np.searchsorted(good, index[good]), -1), ri)
    for method in ("statistical", "radius"):
        _, kept = PF.remove_outliers(PointCloud(points, None, None), k=8, max_dist=0.05, method=method, backend="host")
        assert not np.isin(bad, kept).any()
    nrm = PF.estimate_normals(points, k=8, max_dist=0.05, backend="host")
    assert np.all(nrm[bad] == 0) and np.isfinite(nrm).all()


@pytest.mark.parametrize("n", [0, 1, 2, 8, 9])
def test_edge_sizes(n):
    k, md = 8, 0.2                                                        # the first points of the plane's first row: all within 0.2
    P = scene().points[:n]
    index, d2, count = PF.knn_host(P, k, md)
    bi, bd, bc = brute32(P, k, md)
    assert index.shape == (n, k) and d2.shape == (n, k) and count.shape == (n,)
    assert index.dtype == np.int32 and d2.dtype == np.float32 and count.dtype == np.int32
    assert np.array_equal(index, bi) and np.array_equal(d2, bd) and np.array_equal(count, bc)
    if n:
        assert count.max() == min(n - 1, k)
    cloud, kept = PF.remove_outliers(PointCloud(P, None, None), k=k, max_dist=md, backend="host")
    if n < k + 1:
        assert len(kept) == 0                                             # fewer than k others: everybody is starved
    else:
        stat = PF.stat_host(bd, bc).astype(np.float64)
        assert np.isfinite(stat).all()
        assert np.array_equal(kept, np.flatnonzero(stat <= stat.mean() + 2.0 * stat.std())) and len(kept) >= n - 1
    assert PF.estimate_normals(P, k=k, max_dist=md, backend="host").shape == (n, 3)


def test_bad_arguments():
    P = scene().points[:20]
    for k in (0, 33, -1, 2.5):
        with pytest.raises(ValueError):
            PF.knn(P, k, 0.05, backend="host")
    for md in (0.0, float("nan"), float("inf"), -1.0, None, 1e30, 1e-30):
        with pytest.raises(ValueError):
            PF.knn(P, 8, md, backend="host")
        with pytest.raises(ValueError):
            PF.remove_outliers(PointCloud(P, None, None), k=8, max_dist=md, backend="host")
    with pytest.raises(ValueError):
        PF.knn(P, 8, 0.05, backend="eager")
    with pytest.raises(ValueError):
        PF.remove_outliers(PointCloud(P, None, None), max_dist=0.05, method="median", backend="host")
    with pytest.raises(ValueError):
        PF.knn(P[:, :2], 8, 0.05, backend="host")
    with pytest.raises(RuntimeError, match="GPU"):                         # no host fall-back behind the device backend
        PF.knn(P, 8, 0.05, backend="device", device="cpu")


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("k,md", CASES)
def test_statistical_mask_against_float64_kdtree(seed, k, md):
    """The mask from float64 cKDTree distances.  Precondition (a condition on the INPUTS): every finite float64 statistic is at
    least 1e-5 relative away from the threshold - fp32 against fp64 rounding is about 1e-7.  Then the masks are equal, and all 60
    outliers go."""
    sc = scene(seed)
    P = sc.points.astype(np.float64)
    d = cKDTree(P).query(P, k=k + 1, distance_upper_bound=md)[0][:, 1:].reshape(len(P), k)
    stat = np.where(np.isfinite(d).all(axis=1), d.sum(axis=1) / k, np.inf)
    fin = stat[np.isfinite(stat)]
    thr = fin.mean() + 2.0 * fin.std()
    assert np.abs(fin - thr).min() >= 1e-5 * thr
    st = {}
    cloud, kept = PF.remove_outliers(PointCloud(sc.points, None, None), k=k, std_ratio=2.0, max_dist=md, backend="host", stats=st)
    mask = np.zeros(len(P), bool)
    mask[kept] = True
    assert np.array_equal(mask, stat <= thr)
    assert not mask[sc.parts["outliers"]].any()
    assert mask[sc.parts["plane"]].mean() > 0.9 and mask[sc.parts["lattice"]].all()
    assert st["points_in"] == len(P) and st["points_out"] == len(kept) and st["starved"] == int(np.isinf(stat).sum())
    assert st["threshold"] == pytest.approx(thr, rel=1e-6) and st["mu"] == pytest.approx(fin.mean(), rel=1e-6)
    assert st["sd"] == pytest.approx(fin.std(), rel=1e-5)
    assert np.array_equal(cloud.points, sc.points[kept])
    s2, c2 = PF.outlier_stats(sc.points, k, md, backend="host")
    assert np.allclose(s2[np.isfinite(s2)], fin, rtol=1e-6) and np.array_equal(np.isfinite(s2), np.isfinite(stat))


@pytest.mark.parametrize("k,radius", [(4, 0.013), (8, 0.02)])
def test_radius_rule_against_kdtree_ball_count(k, radius):
    sc = scene()
    P = sc.points.astype(np.float64)
    tree = cKDTree(P)
    balls = tree.query_ball_point(P, radius)
    n_in = np.array([len(b) - 1 for b in balls])
    # a pair within 1e-6 relative of the radius may fall either way in fp32: none here (the precondition)
    assert all(len(a) == len(b) for a, b in zip(tree.query_ball_point(P, radius * (1 - 1e-6)), tree.query_ball_point(P, radius * (1 + 1e-6))))
    st = {}
    _, kept = PF.remove_outliers(PointCloud(sc.points, None, None), k=k, max_dist=radius, method="radius", backend="host", stats=st)
    assert np.array_equal(kept, np.flatnonzero(n_in >= k))
    assert st["threshold"] is None and st["starved"] == len(P) - len(kept)
    assert not np.isin(np.arange(sc.parts["outliers"].start, sc.parts["outliers"].stop), kept).any()


def _cov_rows(P, index, rows):
    """The float64 covariance of a point and its neighbours, from the rule's fp32 differences."""
    E = (P[index[rows]] - P[rows][:, None, :]).astype(np.float64)
    m = index.shape[1] + 1
    M = E.sum(axis=1) / m
    return np.einsum("nka,nkb->nab", E, E) / m - M[:, :, None] * M[:, None, :]


def _angle(a, b):
    return np.arcsin(np.minimum(np.linalg.norm(np.cross(a, b), axis=-1), 1.0))


@pytest.mark.parametrize("where", list(CENTRES))
def test_normals_against_eigh(where):
    """At points with count == k and a separated smallest eigenvalue ((l1 - l0) >= 1e-3 l2; at most 1 % may fail that): within
    1e-6 rad of np.linalg.eigh's eigenvector of the same float64 covariance.  Converged fp64 Jacobi is good to ~1e-13; the one
    rounding to fp32 costs ~4e-8."""
    k, md = 16, 0.08
    sc = scene(0, where)
    index, _, count = host_knn(0, where, k, md)
    nrm = PF.normals_host(sc.points, index, count)
    assert nrm.dtype == np.float32 and nrm.shape == (len(sc.points), 3)
    full = count == k
    w, v = np.linalg.eigh(_cov_rows(sc.points, index, full))
    ok = (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]
    assert ok.mean() >= 0.99
    n = nrm[full].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    assert _angle(n[ok], v[ok, :, 0]).max() <= 1e-6
    # without centres: the component of largest magnitude is positive
    big = np.take_along_axis(n, np.abs(n).argmax(axis=1)[:, None], axis=1)
    assert (big > 0).all()
    # the plane's normals are +-z within 0.1 rad
    plane = np.zeros(len(full), bool)
    plane[sc.parts["plane"]] = True
    assert _angle(nrm[plane & full].astype(np.float64), np.array([0.0, 0.0, 1.0])).max() <= 0.1
    # count < 2: (0, 0, 0)
    assert np.all(nrm[count < 2] == 0) and (count < 2).sum() >= 2 and np.all(nrm[sc.parts["pair"]] == 0)
    assert np.all(np.linalg.norm(nrm[count >= 2], axis=1) > 0.99)


@pytest.mark.parametrize("where", list(CENTRES))
def test_normals_turn_to_the_camera(where):
    """On the sphere every oriented normal satisfies n . (c - p) >= 0.  A camera at the sphere's centre turns every normal inwards.
    A camera far away on +z turns them outwards on the half of the sphere that faces it (on the far half, which such a camera
    could not have seen, 'towards the camera' IS inwards: those points are left out of the outward claim, not of the first one)."""
    k, md = 16, 0.08
    sc = scene(0, where)
    n_pts = len(sc.points)
    sphere = np.zeros(n_pts, bool)
    sphere[sc.parts["sphere"]] = True
    mid = S.SPHERE_CENTRE + sc.centre
    far = mid + np.array([0.0, 0.0, 1000.0])
    origin = np.stack([np.arange(n_pts) % 2, np.arange(n_pts)], axis=1).astype(np.int32)      # two views, interleaved
    cloud = PointCloud(sc.points, None, origin)
    P = sc.points.astype(np.float64)
    radial = P - mid
    for centres, name in ((np.stack([mid, mid]), "inside"), (np.stack([far, far]), "far"), (np.stack([mid, far]), "mixed")):
        nrm = PF.estimate_normals(cloud, centres, k=k, max_dist=md, backend="host").astype(np.float64)
        c = centres[origin[:, 0]]
        assert ((nrm * (c - P)).sum(axis=1) >= 0)[sphere].all(), name
        out = (nrm * radial).sum(axis=1)
        if name == "inside":
            assert (out[sphere] < 0).all()                                # a camera at the sphere's centre: every normal points inwards
        elif name == "far":
            facing = sphere & (radial[:, 2] > 0.2 * S.SPHERE_RADIUS)      # the side that camera sees: outwards
            assert (out[facing] > 0).all() and facing.sum() > 400
        else:
            assert (out[sphere & (origin[:, 0] == 0)] < 0).all()
    with pytest.raises(ValueError):                                       # a view index the centres do not have
        PF.estimate_normals(cloud, np.zeros((1, 3)), k=k, max_dist=md, backend="host")
    with pytest.raises(ValueError):
        PF.estimate_normals(sc.points, np.zeros((2, 3)), k=k, max_dist=md, backend="host")


def test_camera_centres():
    g = np.random.default_rng(3)
    views, want = [], []
    for _ in range(3):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        K = np.array([[500.0, 0, 320], [0, 510.0, 240], [0, 0, 1]])
        c = g.normal(size=3) * 100 + np.array(S.WORLD_CENTRE)
        views.append(DepthView(np.concatenate([K @ q, (-(K @ q) @ c)[:, None]], axis=1), np.zeros((2, 2), np.float32), 1.0))
        want.append(c)
    got = PF.camera_centres(views)
    assert got.dtype == np.float64 and np.allclose(got, np.array(want), rtol=0, atol=1e-8)


def test_remove_outliers_filters_every_field():
    sc = scene()
    n = len(sc.points)
    g = np.random.default_rng(5)
    colors = g.integers(0, 256, (n, 3)).astype(np.uint8)
    origin = np.stack([np.arange(n) // 1000, g.integers(0, 5000, n)], axis=1).astype(np.int32)
    cloud, kept = PF.remove_outliers(PointCloud(sc.points, colors, origin), k=8, max_dist=0.05, backend="host")
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0) and 0 < len(kept) < n
    assert isinstance(cloud, PointCloud)
    assert np.array_equal(cloud.points, sc.points[kept]) and np.array_equal(cloud.colors, colors[kept])
    assert np.array_equal(cloud.origin, origin[kept])
    cloud2, kept2 = PF.remove_outliers((sc.points, None, origin), k=8, max_dist=0.05, backend="host")
    assert cloud2.colors is None and np.array_equal(kept2, kept)
    # the scripts' step: outliers first, normals on what is left
    views = [DepthView(np.concatenate([np.eye(3), -np.array([[0.2], [0.2], [5.0 + v]])], axis=1), np.zeros((2, 2), np.float32), 1.0)
             for v in range(4)]
    c3, nrm, rec = PF.clean_step(PointCloud(sc.points, colors, origin), views, outliers=(8, 2.0), normals_k=8, max_dist=0.05, backend="host")
    assert np.array_equal(c3.points, cloud.points) and nrm.shape == c3.points.shape
    assert rec["cloud_filter"]["points_out"] == len(kept) and rec["cloud_filter"]["method"] == "statistical"
    assert set(rec["cloud_filter"]) == {"method", "k", "std_ratio", "max_dist", "points_in", "points_out", "starved", "threshold", "ms"}
    assert set(rec["cloud_normals"]) == {"k", "zero", "ms"} and rec["cloud_normals"]["zero"] == int((~nrm.any(axis=1)).sum())
    assert np.array_equal(nrm, PF.estimate_normals(c3, PF.camera_centres(views), k=8, max_dist=0.05, backend="host"))


def test_write_ply_points_with_normals(tmp_path):
    from surf_amd.datasets import mvs_io
    sc = scene()
    P = sc.points[:500]
    g = np.random.default_rng(9)
    colors = g.integers(0, 256, (len(P), 3)).astype(np.uint8)
    normals = g.normal(size=(len(P), 3)).astype(np.float32)
    path = str(tmp_path / "cloud.ply")
    for col in (None, colors):
        mesh_io.write_ply_points(path, P, col, normals=normals)
        assert np.array_equal(mvs_io.read_ply_points(path), P.astype(np.float64))
        v, t, attrs = mesh_io.read_ply(path, attributes=True)
        assert np.array_equal(v, P) and len(t) == 0 and np.array_equal(attrs["normals"], normals)
        assert (col is None and "colors" not in attrs) or np.array_equal(attrs["colors"], col)
        with open(path, "rb") as f:
            assert b"property float nx\nproperty float ny\nproperty float nz\n" in f.read(400)
        # without normals the file is today's, byte for byte: write_ply called as write_ply_points has called it so far
        mesh_io.write_ply_points(path, P, col)
        mesh_io.write_ply(str(tmp_path / "ref.ply"), P, np.zeros((0, 3), dtype=np.int32), colors=col)
        with open(path, "rb") as a, open(str(tmp_path / "ref.ply"), "rb") as b:
            assert a.read() == b.read()


def test_points_knn_exports():
    """Header, binding table and library agree on the new entry points; the status codes arrive as ValueError before the call."""
    from surf_amd import _lib, ops
    L = _lib.lib()
    with open(_lib.HEADER_PATH) as f:
        hdr = f.read()
    for name in ("surf_points_knn_keys", "surf_points_knn", "surf_points_knn_reduce", "surf_points_stat_sums"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
    assert ops.POINTS_KNN_MAX_K == PF.KNN_MAX_K == 32 and "#define SURF_POINTS_KNN_MAX_K 32" in hdr
    assert f"#define SURF_POINTS_NORMAL_SWEEPS {PF.NORMAL_SWEEPS}" in hdr
    assert f"#define SURF_POINTS_STAT_SLOTS {ops.POINTS_STAT_SLOTS}" in hdr
    assert ops.POINTS_KNN_MAX_CELLS == 1 << 26 and "#define SURF_POINTS_KNN_MAX_CELLS (1 << 26)" in hdr
    # argument validation happens before any HIP call: no GPU needed
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_points_knn(None, None, None, 5, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, 33, 0.1, None, None, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_points_knn(None, None, None, 5, 0.0, 0.0, 0.0, 1.0, 1, 1, 1, 8, 0.0, None, None, None, None)
    for k, md in ((0, 0.1), (33, 0.1), (8, 0.0), (8, float("nan"))):
        with pytest.raises(ValueError):
            ops._chk_knn(k, md, "test")
