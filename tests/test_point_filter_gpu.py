"""csrc/point_knn.hip through surf_amd/point_filter.py, backend="device", against the numpy mirror (backend="host", itself pinned by
tests/test_point_filter_host.py): EQUAL arrays - neighbour lists, statistics, masks, normals - on tests/point_filter_scenes.py's
cloud at the origin and in a world frame near (300, -150, 600), under forced cell sizes, at the edge sizes, with non-finite rows,
and once behind fusion.fuse_points."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import fusion, ops, point_filter as PF
from surf_amd.fusion import PointCloud
from tests import point_filter_scenes as S
from tests import points_scenes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CENTRES = {"origin": (0.0, 0.0, 0.0), "world": S.WORLD_CENTRE}
CASES = ((1, 0.05), (8, 0.05), (16, 0.08), (32, 0.08))


@functools.lru_cache(maxsize=None)
def scene(where="origin"):
    return S.build(0, CENTRES[where])


@functools.lru_cache(maxsize=None)
def host_knn(where, k, md):
    return PF.knn_host(scene(where).points, k, md)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("where", list(CENTRES))
@pytest.mark.parametrize("k,md", CASES)
def test_knn_device_equals_host(where, k, md):
    sc = scene(where)
    got = PF.knn(sc.points, k, md, backend="device", device=DEV)
    _same(got, host_knn(where, k, md))
    # the fused entry point (no lists) gives the statistic and the count derived from the lists
    stat, count = PF.outlier_stats(sc.points, k, md, backend="device", device=DEV)
    assert stat.dtype == np.float32 and np.array_equal(stat, PF.stat_host(got[1], got[2])) and np.array_equal(count, got[2])


@pytest.mark.parametrize("where", list(CENTRES))
@pytest.mark.parametrize("k,md", [(8, 0.05), (32, 0.08)])
def test_result_does_not_depend_on_the_cell(where, k, md):
    """The default cell, a quarter of it (a walk over many shells) and four times it (many points per cell)."""
    sc = scene(where)
    pts = torch.from_numpy(sc.points).to(DEV)
    cell = ops.PointKnnTable(pts, md).cell
    want = host_knn(where, k, md)
    for c in (cell, cell / 4, cell * 4):
        table = ops.PointKnnTable(pts, md, cell=c)
        assert table.cell == c
        _same([t.cpu().numpy() for t in ops.points_knn(table, k, md)], want)
        stat, count, nrm = ops.points_knn_reduce(table, k, md, normals=True)
        assert np.array_equal(count.cpu().numpy(), want[2])
        assert np.array_equal(stat.cpu().numpy(), PF.stat_host(want[1], want[2]))
        assert np.array_equal(nrm.cpu().numpy(), PF.normals_host(sc.points, want[0], want[2]))


@pytest.mark.parametrize("where", list(CENTRES))
@pytest.mark.parametrize("method,k,md", [("statistical", 1, 0.05), ("statistical", 8, 0.05), ("statistical", 16, 0.08), ("radius", 8, 0.02)])
def test_masks_device_equal_host(where, method, k, md):
    sc = scene(where)
    n = len(sc.points)
    g = np.random.default_rng(11)
    cloud = PointCloud(sc.points, g.integers(0, 256, (n, 3)).astype(np.uint8), np.stack([np.arange(n) % 3, np.arange(n)], 1).astype(np.int32))
    sd, sh = {}, {}
    dev_cloud, dev_kept = PF.remove_outliers(cloud, k=k, std_ratio=2.0, max_dist=md, method=method, backend="device", device=DEV, stats=sd)
    host_cloud, host_kept = PF.remove_outliers(cloud, k=k, std_ratio=2.0, max_dist=md, method=method, backend="host", stats=sh)
    assert np.array_equal(dev_kept, host_kept) and dev_kept.dtype == np.int64 and 0 < len(dev_kept) < n
    _same(dev_cloud, host_cloud)
    assert not np.isin(np.arange(sc.parts["outliers"].start, sc.parts["outliers"].stop), dev_kept).any()
    for key in ("points_in", "points_out", "starved"):
        assert sd[key] == sh[key]
    if method == "statistical":
        for key in ("mu", "sd", "threshold"):                       # the same numbers added in another order: the last bits may differ
            assert sd[key] == pytest.approx(sh[key], rel=1e-12)
    else:
        assert sd["threshold"] is None


@pytest.mark.parametrize("where", list(CENTRES))
def test_normals_device_equal_host(where):
    k, md = 16, 0.08
    sc = scene(where)
    n = len(sc.points)
    cloud = PointCloud(sc.points, None, np.stack([np.arange(n) % 3, np.arange(n)], 1).astype(np.int32))
    mid = S.SPHERE_CENTRE + sc.centre
    centres = np.stack([mid, mid + np.array([0.0, 0.0, 1000.0]), mid + np.array([3.0, -2.0, 0.5])])
    for c in (None, centres):
        got = PF.estimate_normals(cloud, c, k=k, max_dist=md, backend="device", device=DEV)
        want = PF.estimate_normals(cloud, c, k=k, max_dist=md, backend="host")
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert (np.linalg.norm(want, axis=1) > 0.99).mean() > 0.97 and np.all(want[sc.parts["pair"]] == 0)


def test_two_runs_are_bit_equal():
    sc = scene("world")
    cloud = PointCloud(sc.points, None, np.zeros((len(sc.points), 2), np.int32))
    runs = []
    for _ in range(2):
        st = {}
        _, kept = PF.remove_outliers(cloud, k=16, max_dist=0.08, backend="device", device=DEV, stats=st)
        nrm = PF.estimate_normals(cloud, np.array([[0.0, 0.0, 0.0]]), k=16, max_dist=0.08, backend="device", device=DEV)
        runs.append((kept, nrm, np.array([st["mu"], st["sd"], st["threshold"]])))
    _same(runs[0], runs[1])


def test_stat_sums_are_reproducible_and_right():
    """More values than slots x 256 (a thread adds several), with +inf and NaN among them: number, sum and sum of squares of the
    finite ones against numpy's float64 (pairwise) sums, and the same bits twice."""
    g = np.random.default_rng(13)
    x = g.uniform(0.0, 0.1, 300001).astype(np.float32)
    x[g.choice(len(x), 999, replace=False)] = np.inf
    x[5], x[70000] = np.nan, -np.inf
    for n in (300001, 3649, 1):
        t = torch.from_numpy(x[:n]).to(DEV)
        a, b = ops.points_stat_sums(t).cpu().numpy(), ops.points_stat_sums(t).cpu().numpy()
        fin = x[:n][np.isfinite(x[:n])].astype(np.float64)
        assert np.array_equal(a, b) and a[0] == len(fin)
        assert a[1] == pytest.approx(fin.sum(), rel=1e-12) and a[2] == pytest.approx((fin * fin).sum(), rel=1e-12)


@pytest.mark.parametrize("n", [0, 1, 2, 8, 9])
def test_edge_sizes(n):
    k, md = 8, 0.2
    P = scene().points[:n]
    _same(PF.knn(P, k, md, backend="device", device=DEV), PF.knn_host(P, k, md))
    cloud = PointCloud(P, None, np.zeros((n, 2), np.int32))
    _same(PF.remove_outliers(cloud, k=k, max_dist=md, backend="device", device=DEV)[1:], PF.remove_outliers(cloud, k=k, max_dist=md, backend="host")[1:])
    got = PF.estimate_normals(cloud, np.zeros((1, 3)), k=k, max_dist=md, backend="device", device=DEV)
    assert np.array_equal(got, PF.estimate_normals(cloud, np.zeros((1, 3)), k=k, max_dist=md, backend="host")) and got.shape == (n, 3)


def test_non_finite_rows():
    points, bad = S.with_bad_rows(scene())
    k, md = 8, 0.05
    got = PF.knn(points, k, md, backend="device", device=DEV)
    _same(got, PF.knn_host(points, k, md))
    assert np.all(got[2][bad] == 0) and not np.isin(got[0], bad).any()
    cloud = PointCloud(points, None, np.zeros((len(points), 2), np.int32))
    for method in ("statistical", "radius"):
        kept = PF.remove_outliers(cloud, k=k, max_dist=md, method=method, backend="device", device=DEV)[1]
        assert np.array_equal(kept, PF.remove_outliers(cloud, k=k, max_dist=md, method=method, backend="host")[1])
        assert not np.isin(bad, kept).any()
    nrm = PF.estimate_normals(cloud, None, k=k, max_dist=md, backend="device", device=DEV)
    assert np.array_equal(nrm, PF.estimate_normals(cloud, None, k=k, max_dist=md, backend="host")) and np.all(nrm[bad] == 0)
    # nothing but non-finite rows
    got = PF.knn(points[bad], k, md, backend="device", device=DEV)
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isinf(got[1]))


def test_three_points_all_apart():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.5]], np.float32)
    for k in (1, 2):
        index, d2, count = PF.knn(P, k, 0.5, backend="device", device=DEV)
        assert np.all(count == 0) and np.all(index == -1) and np.all(np.isinf(d2))
        stat, _ = PF.outlier_stats(P, k, 0.5, backend="device", device=DEV)
        assert np.all(np.isposinf(stat))
        for method in ("statistical", "radius"):
            st = {}
            cloud, kept = PF.remove_outliers(PointCloud(P, None, None), k=k, max_dist=0.5, method=method, backend="device", device=DEV, stats=st)
            assert len(kept) == 0 and len(cloud.points) == 0 and st["starved"] == 3 and st["points_out"] == 0
    assert np.all(PF.estimate_normals(P, k=2, max_dist=0.5, backend="device", device=DEV) == 0)
    # exactly AT max_dist is within it: d2 <= md2
    index, d2, count = PF.knn(P, 1, 1.0, backend="device", device=DEV)
    assert count.tolist() == [1, 1, 0] and index[:, 0].tolist() == [1, 0, -1] and d2[0, 0] == 1.0


def test_bad_arguments_reach_no_kernel():
    pts = torch.from_numpy(scene().points[:50]).to(DEV)
    for k, md in ((0, 0.1), (33, 0.1), (8, 0.0), (8, float("nan")), (8, float("inf"))):
        with pytest.raises(ValueError):
            ops.points_knn(pts, k, md)
        with pytest.raises(ValueError):
            ops.points_knn_reduce(pts, k, md)
        with pytest.raises(ValueError):
            PF.knn(pts, k, md, backend="device", device=DEV)


def test_behind_fuse_points():
    """fuse_points -> remove_outliers -> estimate_normals on a ring of views of a sphere, host against device."""
    views = points_scenes.SCENES["ring_colors"]()
    cloud = fusion.fuse_points(views, 1, backend="device", device=DEV)
    assert len(cloud.points) > 500
    centres = PF.camera_centres(views)
    out = {}
    for backend in ("device", "host"):
        st = {}
        kept_cloud, kept = PF.remove_outliers(cloud, k=8, std_ratio=2.0, max_dist=0.1, backend=backend, device=DEV if backend == "device" else None,
                                              stats=st)
        nrm = PF.estimate_normals(kept_cloud, centres, k=8, max_dist=0.1, backend=backend, device=DEV if backend == "device" else None)
        out[backend] = (kept, kept_cloud.points, kept_cloud.colors, kept_cloud.origin, nrm)
        assert 0 < len(kept) <= len(cloud.points)
    _same(out["device"], out["host"])
    kept, pts, _, origin, nrm = out["device"]
    seen = np.linalg.norm(nrm, axis=1) > 0
    assert seen.mean() > 0.9
    # every normal looks at the camera that saw its point, and on this sphere (centred at the origin) that is outwards
    assert (((centres[origin[:, 0]] - pts) * nrm).sum(axis=1)[seen] >= 0).all()
    assert ((pts * nrm).sum(axis=1)[seen] > 0).mean() > 0.95


def test_fuse_scene_cloud_flags(tmp_path):
    """scripts/fuse_scene.py --point_cloud --cloud_outliers 16 2.0 --cloud_normals 16 on the synthetic DTU-format scene: the filtered
    cloud with nx ny nz in <scan>_points.ply and the two record entries; without the flags the cloud and the record are what they
    were."""
    from bench import surf_conf
    from surf_amd import mesh_io
    from surf_amd.datasets import mvs_io
    from tests.test_end_to_end_dtu import _write_scene
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import fuse_scene
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "3", "--resolution", "64", "--logit_override", "sphere",
              "--min_consistent", "1", "--colors", "--point_cloud"]
    s0, s1 = {}, {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), s0)
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--cloud_outliers", "16", "2.0", "--cloud_normals", "16", "--out_dir",
                                                         str(tmp_path / "out")]), s1)
    assert set(rec) == set(plain) | {"cloud_filter", "cloud_normals"}
    cf, cn = rec["cloud_filter"], rec["cloud_normals"]
    assert cf["method"] == "statistical" and cf["k"] == 16 and cf["std_ratio"] == 2.0 and cf["max_dist"] == pytest.approx(10 * rec["voxel"])
    assert cf["points_in"] == plain["points"] and cf["points_out"] == rec["points"] and 0 < rec["points"] <= plain["points"]
    assert cn["k"] == 16 and cf["ms"] > 0 and cn["ms"] > 0
    # the unfiltered cloud is what it is without the flags; the filtered one is a subset of it, written with its normals
    raw = mvs_io.read_ply_points(plain["points_file"])
    assert np.array_equal(raw, s0["cloud"].points.astype(np.float64))
    want_cloud, kept = PF.remove_outliers(s0["cloud"], k=16, std_ratio=2.0, max_dist=cf["max_dist"], backend="host")
    v, t, attrs = mesh_io.read_ply(rec["points_file"], attributes=True)
    assert len(t) == 0 and np.array_equal(v, want_cloud.points) and np.array_equal(attrs["colors"], want_cloud.colors)
    assert np.array_equal(v, s1["cloud"].points) and attrs["normals"].shape == v.shape
    assert cn["zero"] == int((~attrs["normals"].any(axis=1)).sum())
    assert np.allclose(np.linalg.norm(attrs["normals"], axis=1)[attrs["normals"].any(axis=1)], 1.0, atol=1e-6)
    with open(plain["points_file"], "rb") as f:
        assert b"property float nx" not in f.read(400)
    with pytest.raises(SystemExit):
        fuse_scene.run(fuse_scene.parse_args(common[:-1] + ["--cloud_normals", "16", "--out_dir", str(tmp_path / "bad")]))
    print(f"fuse_scene cloud steps: {cf['points_in']} -> {cf['points_out']} points ({cf['starved']} starved) in {cf['ms']:.1f} ms, "
          f"normals in {cn['ms']:.1f} ms ({cn['zero']} zero)")
