"""CPU: fused point clouds - fusion.fuse_points(backend="host"), the numpy-fp32 mirror of the merge rule written out in
csrc/point_cloud.hip's header comment, on analytic sphere scenes; the point-cloud writer; the evaluator's point-cloud mode against
chamfer_dtu and against the numbers the reference's evaluator printed; the new entry points of the library.
tests/test_points_gpu.py compares the device path with this one."""
import json
import os

import numpy as np
import pytest

from surf_amd import fusion, mesh_io
from surf_amd.datasets import mvs_io
from surf_amd.evaluation import dtu_eval as E
from tests import points_scenes as S

F32_MAX = float(np.finfo(np.float32).max)


def others(n):
    return [[s for s in range(n) if s != r] for r in range(n)]


def replay(views, cloud, min_consistent, sources):
    """Walks the views in order with consistency_host and the cloud's origin, keeping the used maps as the rule states them:
    yields per view (the view with its used pixels zeroed, count, zsum, keep, the flat indices the cloud emitted for it), having
    asserted that no emitted pixel had been marked by an earlier view and that the emitted pixels are the accepted ones."""
    used = [np.zeros(np.asarray(v.depth).shape, bool) for v in views]
    assert np.array_equal(cloud.origin, cloud.origin[np.lexsort((cloud.origin[:, 1], cloud.origin[:, 0]))])
    for r, view in enumerate(views):
        emitted = cloud.origin[cloud.origin[:, 0] == r, 1]
        assert not used[r].reshape(-1)[emitted].any(), r
        cand = view._replace(depth=np.where(used[r], np.float32(0), view.depth))
        matches = []
        count, zsum = fusion.consistency_host(list(views[:r]) + [cand] + list(views[r + 1:]), r, sources[r], matches=matches)
        keep = fusion.finish_host(cand, count, zsum, min_consistent)[1]
        assert np.array_equal(np.flatnonzero(keep), emitted), r
        for s, agree, sx, sy in matches:
            hit = keep & agree
            used[s][np.rint(sy[hit]).astype(int), np.rint(sx[hit]).astype(int)] = True
        yield cand, count, zsum, keep, emitted
    replay.used = used


def test_lift_returns_to_the_pixel_within_the_rounding_bound():
    """float64 P_r [X; 1] = (x z, y z, z) within the rounding of the lift.  With u = 2^-24 (fp32 unit roundoff), per coordinate
    X_k = fl(fl(fl(a0 qx + a1 qy) + a2 z) + c_k): the terms a0 qx and a1 qy each carry the rounding of a_j (Minv, rounded once), of
    q_j = fl(x z), of the product and of the three additions they pass through = 6 roundings; a2 z carries 4 (z is exact), c_k 2
    (its own and the last addition).  So |X_k - exact| <= k u (sum_j |Minv_kj q_j| + |c_k|) with k = 6 (gamma_6 = 6u / (1 - 6u), the
    factor 1 / (1 - 6u) is the 1 + 2^-20 below); through P_r that is |M_r| times this vector.  The float64 inverse the exact value is
    stated with has its own error, cond(M) 2^-53 relative; 2^-40 of the same magnitudes covers it for these cameras (cond < 10^3)."""
    views = S.mixed_views()
    cloud = fusion.fuse_points(views, 0, sources=[[]] * len(views), average=False, backend="host")     # every measured pixel
    assert len(cloud.points) > 800 and cloud.points.dtype == np.float32
    k, u = 6, 2.0 ** -24
    worst = 0.0
    for r, v in enumerate(views):
        sel = cloud.origin[:, 0] == r
        assert sel.sum() > 50
        P = np.asarray(v.P, np.float64)
        M, t = P[:, :3], P[:, 3]
        assert np.linalg.cond(M) < 1e3
        Minv = np.linalg.inv(M)
        c = -Minv @ t
        W = v.depth.shape[1]
        y, x = np.divmod(cloud.origin[sel, 1].astype(np.int64), W)
        z = (v.depth[y, x] * np.float32(v.dscale)).astype(np.float64)            # average off: the emitted depth is d, fp32
        q = np.stack([x * z, y * z, z], axis=-1)
        got = cloud.points[sel].astype(np.float64) @ M.T + t
        mag = np.abs(q) @ np.abs(Minv).T + np.abs(c)                             # (n, 3): sum_j |Minv_kj q_j| + |c_k|
        bound = (k * u * (1 + 2.0 ** -20) + 2.0 ** -40) * (mag @ np.abs(M).T)
        err = np.abs(got - q)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (r, float((err / bound).max()))
    print(f"lift: largest error / bound {worst:.3f}")


def test_no_sources_emits_every_measured_pixel_in_order():
    views = S.mixed_views()
    n = len(views)
    stats = {}
    cloud = fusion.fuse_points(views, 0, sources=[[]] * n, backend="host", stats=stats)
    want_origin, want_points, want_colors = [], [], []
    for r, v in enumerate(views):
        with np.errstate(all="ignore"):
            d = v.depth * np.float32(v.dscale)
            flat = np.flatnonzero((d > 0) & (d <= F32_MAX))
        y, x = np.divmod(flat, v.depth.shape[1])
        want_origin.append(np.stack([np.full(len(flat), r), flat], axis=-1))
        want_points.append(fusion.lift_host(fusion.lift_transform(v), x, y, d[y, x]))
        want_colors.append(fusion.quantise_colors_host(v.image[y, x]))
        assert 0 < len(flat) < d.size
    assert cloud.origin.dtype == np.int32 and np.array_equal(cloud.origin, np.concatenate(want_origin))
    assert np.array_equal(cloud.points, np.concatenate(want_points))
    assert cloud.colors.dtype == np.uint8 and np.array_equal(cloud.colors, np.concatenate(want_colors))
    assert (cloud.colors == 0).any() and (cloud.colors == 255).any()             # both clamps were at work
    assert stats["marked"] == [0] * n and not any(u.any() for u in stats["used"])
    assert stats["candidates"] == stats["emitted"] == [len(o) for o in want_origin]
    # min_consistent = 0 with sources still merges: fewer points, the same first view
    merged = fusion.fuse_points(views, 0, backend="host")
    assert len(merged.points) < len(cloud.points)
    assert np.array_equal(merged.origin[merged.origin[:, 0] == 0], want_origin[0])


@pytest.mark.parametrize("min_consistent", [1, 2])
def test_views_of_one_surface_are_merged_not_repeated(min_consistent):
    views = S.ring_views()
    n = len(views)
    stats, fstats = {}, {}
    cloud = fusion.fuse_points(views, min_consistent, backend="host", stats=stats)
    fusion.filter_views(views, min_consistent, average=True, backend="host", stats=fstats)
    print(f"min_consistent {min_consistent}: {len(cloud.points)} points, filter_views keeps {sum(fstats['kept'])}; "
          f"per view {stats['emitted']}, marked {stats['marked']}")
    assert 0 < len(cloud.points) < sum(fstats["kept"])
    assert stats["emitted"][0] == fstats["kept"][0]                              # nothing is used when the first view is visited
    assert all(e <= k for e, k in zip(stats["emitted"], fstats["kept"])) and stats["emitted"][-1] < fstats["kept"][-1]
    assert sum(stats["emitted"]) == len(cloud.points) and all(e <= c for e, c in zip(stats["emitted"], stats["candidates"]))
    steps = list(replay(views, cloud, min_consistent, others(n)))
    assert len(steps) == n
    assert all(np.array_equal(u, s != 0) for u, s in zip(replay.used, stats["used"]))
    assert sum(stats["marked"]) == sum(int(u.sum()) for u in stats["used"]) > 0
    # the points lie on the sphere the depth maps were rendered from: an averaged depth is within rel_thresh = 1 % of the pixel's
    # own (every agreeing w.z is), a point therefore within 1 % of its distance to the camera (< 2.5 + 0.5) of the surface
    assert np.abs(np.linalg.norm(cloud.points.astype(np.float64), axis=1) - 0.5).max() < 0.01 * 3.0


def test_order_and_determinism():
    views = S.mixed_views()
    a = fusion.fuse_points(views, 1, backend="host")
    b = fusion.fuse_points(views, 1, backend="host")
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    key = a.origin[:, 0].astype(np.int64) * (1 << 32) + a.origin[:, 1]
    assert (np.diff(key) > 0).all() and len(np.unique(a.origin[:, 0])) == len(views)
    assert a.points.shape == (len(key), 3) and a.colors.shape == (len(key), 3) and a.origin.shape == (len(key), 2)
    # an explicit source list: nearest_sources' lists go through unchanged
    near = fusion.nearest_sources(views, 2)
    c = fusion.fuse_points(views, 1, sources=near, backend="host")
    list(replay(views, c, 1, near))


@pytest.mark.parametrize("average", [True, False])
def test_emitted_depth_is_finish_hosts(average):
    views = S.ring_views()                                                       # dscale 1: finish_host's division by it is exact
    n = len(views)
    cloud = fusion.fuse_points(views, 2, average=average, backend="host")
    moved = 0
    for r, (cand, count, zsum, keep, emitted) in enumerate(replay(views, cloud, 2, others(n))):
        depth = fusion.finish_host(cand, count, zsum, 2, average)[0]
        y, x = np.divmod(emitted, depth.shape[1])
        want = fusion.lift_host(fusion.lift_transform(views[r]), x, y, depth[y, x])
        assert np.array_equal(cloud.points[cloud.origin[:, 0] == r], want), r
        moved += int((depth[y, x] != views[r].depth[y, x]).sum())
    assert (moved > 0) == average


def test_holes_are_never_emitted_nor_marked_and_a_tap_across_a_hole_does_not_agree():
    views = S.mixed_views()
    for mc in (0, 1):
        stats = {}
        cloud = fusion.fuse_points(views, mc, backend="host", stats=stats)
        assert np.isfinite(cloud.points).all()
        for r, v in enumerate(views):
            with np.errstate(all="ignore"):
                hole = ~((v.depth > 0) & (v.depth <= F32_MAX))
            assert hole.sum() > 10
            assert not hole.reshape(-1)[cloud.origin[cloud.origin[:, 0] == r, 1]].any()
            assert not stats["used"][r][hole].any()
    # one source, one hole in it: the reference pixels whose four taps touch the hole are emitted without it and not with it
    ring = S.ring_views(5)[:3]
    only = [[1], [], []]
    matches = []
    fusion.consistency_host(ring, 0, [1], matches=matches)
    _, agree, sx, sy = matches[0]
    clean = fusion.fuse_points(ring, 1, sources=only, backend="host")
    mid = np.flatnonzero(agree)[agree.sum() // 2]                                 # the hole goes where a pair in the middle agreed
    hy, hx = int(np.floor(sy.reshape(-1)[mid])), int(np.floor(sx.reshape(-1)[mid]))
    for h in S.HOLES:
        depth = ring[1].depth.copy()
        assert depth[hy, hx] > 0
        depth[hy, hx] = h
        holed = [ring[0], ring[1]._replace(depth=depth), ring[2]]
        with np.errstate(invalid="ignore"):
            touches = agree & (np.floor(sx) >= hx - 1) & (np.floor(sx) <= hx) & (np.floor(sy) >= hy - 1) & (np.floor(sy) <= hy)
        assert touches.sum() >= 3
        got = fusion.fuse_points(holed, 1, sources=only, backend="host")
        flat = np.flatnonzero(touches)
        mine = got.origin[got.origin[:, 0] == 0, 1]
        assert np.isin(flat, clean.origin[clean.origin[:, 0] == 0, 1]).all() and not np.isin(flat, mine).any()
        assert len(mine) == (clean.origin[:, 0] == 0).sum() - len(flat)


def test_arguments_are_checked_like_filter_views():
    views = S.ring_views(3)
    with pytest.raises(ValueError, match="backend"):
        fusion.fuse_points(views, 1, backend="numpy")
    with pytest.raises(ValueError, match="min_consistent"):
        fusion.fuse_points(views, -1, backend="host")
    with pytest.raises(ValueError, match="sources"):
        fusion.fuse_points(views, 1, sources=[[0], [0], [0]], backend="host")                    # a view lists itself
    with pytest.raises(ValueError, match="sources"):
        fusion.fuse_points(views, 1, sources=[[1]], backend="host")
    some = [views[0]._replace(image=np.zeros(views[0].depth.shape + (3,), np.float32))] + views[1:]
    with pytest.raises(ValueError, match="image"):
        fusion.fuse_points(some, 1, backend="host")
    empty = fusion.fuse_points([], 1, backend="host")
    assert empty.points.shape == (0, 3) and empty.points.dtype == np.float32 and empty.colors is None
    assert empty.origin.shape == (0, 2) and empty.origin.dtype == np.int32
    assert fusion.fuse_points(views, 1, backend="host").colors is None


def test_a_cloud_reads_back_from_its_ply(tmp_path):
    cloud = fusion.fuse_points(S.SCENES["ring_colors"](), 1, backend="host")
    assert len(cloud.points) > 300
    for name, colors in (("plain.ply", None), ("colors.ply", cloud.colors)):
        path = str(tmp_path / "sub" / name)
        mesh_io.write_ply_points(path, cloud.points, colors)
        back = mvs_io.read_ply_points(path)
        assert back.dtype == np.float64 and np.array_equal(back, cloud.points.astype(np.float64))
        v, t, attrs = mesh_io.read_ply(path, attributes=True)
        assert np.array_equal(v, cloud.points) and t.shape == (0, 3)
        assert ("colors" in attrs) == (colors is not None) and (colors is None or np.array_equal(attrs["colors"], colors))
    mesh_io.write_ply_points(str(tmp_path / "none.ply"), np.zeros((0, 3), np.float32))
    assert mvs_io.read_ply_points(str(tmp_path / "none.ply")).shape == (0, 3)


def test_dtu_eval_pcd_mode_equals_chamfer_and_the_reference_evaluator(tmp_path):
    """tests/golden/dtu_eval_pcd_results.json is the results.json the reference's evaluation/dtu_eval.py wrote with `--mode pcd` for
    the clouds of tests/golden/eval_clouds.py on the fifteen synthetic scans of tests/golden/eval_scene.py (run as the script it is
    by tests/golden/make_golden_eval_pcd.py).  The tolerance is test_dtu_eval_equals_the_reference_evaluator's."""
    from scipy.io import loadmat
    from tests.golden import eval_clouds, eval_scene
    with open(os.path.join(os.path.dirname(__file__), "golden", "dtu_eval_pcd_results.json")) as f:
        gold = json.load(f)
    out_dir, data_dir = str(tmp_path / "exp"), str(tmp_path / "eval")
    eval_scene.write_eval_scene(out_dir, data_dir)
    eval_clouds.write_eval_clouds(out_dir)
    rows = []
    for scan in eval_scene.SCANS:
        path = os.path.join(out_dir, eval_clouds.PCD_NAME.format(scan=scan))
        d2s, s2d, overall = E.evaluate_scan(path, data_dir, scan, mode="pcd", rng=np.random.default_rng(eval_scene.SHUFFLE_SEED),
                                            **eval_scene.ARGS)
        ref = gold[str(scan)]
        assert abs(d2s - ref["d2s"]) < 1e-9 * ref["d2s"] + 1e-12, (scan, d2s, ref["d2s"])
        assert abs(s2d - ref["s2d"]) < 1e-9 * ref["s2d"] + 1e-12, (scan, s2d, ref["s2d"])
        assert abs(overall - ref["all"]) < 1e-9 * ref["all"] + 1e-12
        rows.append((d2s, s2d, overall))
    m = np.mean(np.array(rows), axis=0)
    for got, key in zip(m, ("d2s", "s2d", "all")):
        assert abs(got - gold["mean"][key]) < 1e-9 * gold["mean"][key]
    # chamfer_dtu on the same points and generator: the very same numbers
    scan = eval_scene.SCANS[3]
    mat = loadmat(f"{data_dir}/ObsMask/ObsMask{scan}_10.mat")
    direct = E.chamfer_dtu(eval_clouds.cloud_points(scan).astype(np.float64), mvs_io.read_ply_points(f"{data_dir}/Points/stl/stl{scan:03}_total.ply"),
                           mat["ObsMask"], mat["BB"], mat["Res"], loadmat(f"{data_dir}/ObsMask/Plane{scan}.mat")["P"],
                           rng=np.random.default_rng(eval_scene.SHUFFLE_SEED), **eval_scene.ARGS)
    assert direct == rows[3]
    # the mesh of the same scan in mesh mode is another number, and an unknown mode is an error
    mesh = os.path.join(out_dir, "meshes", "final", f"scan{scan}.ply")
    assert E.evaluate_scan(mesh, data_dir, scan, rng=np.random.default_rng(eval_scene.SHUFFLE_SEED), **eval_scene.ARGS) != rows[3]
    with pytest.raises(ValueError, match="mode"):
        E.evaluate_scan(mesh, data_dir, scan, mode="points")
    # the command-line entry reads <out_dir>/mvsnet{scan:03}_l3.ply by default and writes the same file
    E.main(["--out_dir", out_dir, "--dataset_dir", data_dir, "--downsample_density", str(eval_scene.ARGS["downsample_density"]),
            "--shuffle_seed", str(eval_scene.SHUFFLE_SEED), "--mode", "pcd"])
    with open(os.path.join(out_dir, "results.json")) as f:
        mine = json.load(f)
    assert set(mine) == set(gold) and abs(mine["mean"]["all"] - gold["mean"]["all"]) < 1e-9 * gold["mean"]["all"]


def test_points_entry_points_are_declared_bound_and_exported():
    from surf_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "surf_hip.h")).read()
    L = _lib.lib()
    for name in ("surf_points_candidates", "surf_points_mark", "surf_points_lift"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).errcheck is not None
    assert _lib.ABI_VERSION == 41 and L.surf_abi_version() == 41
    assert callable(ops.points_candidates) and callable(ops.points_mark) and callable(ops.points_lift)
    c = _lib.ctypes
    sig = _lib.SIGNATURES["surf_points_mark"][1]
    assert len(sig) == 14 and sig[3] is c.c_float and sig[11:13] == [c.c_float] * 2 and sig[10] is c.c_int
    sig = _lib.SIGNATURES["surf_points_lift"][1]
    assert len(sig) == 16 and sig[8] is c.c_int64 and sig[11] is c.c_int
    # empty work returns at once, whatever the pointers; a negative size is an invalid argument
    assert L.surf_points_candidates(None, None, 0, None, None) == 0
    assert L.surf_points_mark(None, 0, 0, 1.0, None, None, None, None, None, None, 0, 1.0, 0.01, None) == 0
    assert L.surf_points_lift(None, 4, 4, 1.0, None, None, 1, None, 0, None, None, 0, None, None, None, None) == 0
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_points_candidates(None, None, 5, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_points_lift(None, 4, 4, 1.0, None, None, 1, None, 3, None, None, 0, None, None, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_points_mark(None, 4, 4, 1.0, None, None, None, None, None, None, 2, 1.0, 0.01, None)
