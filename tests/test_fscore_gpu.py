"""GPU: csrc/fscore.hip against the host path of surf_amd.evaluation.fscore, stage by stage - equal arrays for the transform, the
crop, the voxel mean and the nearest distance / index; the ICP against the true motion; the protocol's tallies against the host's;
scripts/fuse_scene.py --scene / --tnt_dir on the synthetic Tanks and Temples scene."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import mesh_io, ops
from surf_amd.evaluation import fscore as F
from tests import test_fscore_host as H

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 257, 5000]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def cloud(n, seed=0):
    p = np.random.default_rng(100 * seed + n).uniform(-1, 1, (n, 3)) * np.array([2.0, 1.0, 0.5]) + np.array([10.0, -3.0, 0.25])
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("n", SIZES)
def test_transform_equals_host(n):
    T = np.eye(4)
    T[:3, :3] = H.rotation((0.2, -1.0, 0.4), 33.0)
    T[:3, 3] = [0.3, -20.0, 7.5]
    got = F.transform_points(cloud(n), T, device="gpu")
    assert isinstance(got, np.ndarray) and np.array_equal(bits(got), bits(F.transform_points(cloud(n), T)))


@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
@pytest.mark.parametrize("n", SIZES)
def test_crop_equals_host(n, axis):
    crop = H.l_crop(axis)
    p = np.random.default_rng(n).uniform(-1, 5, (n, 3))
    p[:, "XYZ".index(axis)] = np.random.default_rng(n + 1).uniform(-1, 1.25, n)
    p[::7, "XYZ".index(axis)] = crop.axis_max                                    # on the closed end of the range
    want = F.crop_points(p, crop)
    got = F.crop_points(p, crop, device="gpu")
    assert got.dtype == bool and np.array_equal(got, want)
    if n == 5000:
        assert 0.05 * n < want.sum() < 0.5 * n
        lattice, keep = H.l_lattice(axis)                                        # the host test's case, against its own truth
        assert np.array_equal(F.crop_points(lattice, crop, device="gpu"), keep)


@pytest.mark.parametrize("n", SIZES)
def test_voxel_mean_equals_host(n):
    p = cloud(n)
    want = F.voxel_mean(p, 0.3)
    got = F.voxel_mean(p, 0.3, device="gpu")
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert n < 64 or len(want) < n                                               # voxels with several members


@pytest.mark.parametrize("case", ["mixed", "big_voxel", "one_voxel", "far_origin"])
def test_voxel_mean_segments(case):
    g = np.random.default_rng(9)

    def big_voxel():
        """3,000 normal points and 1,500 in the middle of one voxel of the grid Open3D's rule lays over them."""
        p = g.standard_normal((3000, 3))
        origin = p.min(axis=0) - 0.125
        return np.concatenate([p, origin + 0.25 * (np.floor((7.3 - origin) / 0.25) + 0.5) + g.uniform(-0.05, 0.05, (1500, 3))])
    p = {"mixed": H.voxel_cloud,                                                                 # 400 members in one voxel
         "big_voxel": big_voxel,
         "one_voxel": lambda: g.uniform(0, 0.12, (2049, 3)),
         "far_origin": lambda: g.standard_normal((4000, 3)) * 3 + np.array([1e5, -2e5, 3e4])}[case]()
    want = F.voxel_mean(p, 0.25)
    got = F.voxel_mean(p, 0.25, device="gpu")
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    if case == "one_voxel":
        assert len(got) == 1
    if case == "big_voxel":                                                      # a segment longer than a workgroup, several times
        origin = p.min(axis=0) - 0.125
        cells = np.floor((p - origin) / 0.25).astype(np.int64)
        assert np.unique(cells, axis=0, return_counts=True)[1].max() > 1024


def test_voxel_mean_refuses_more_than_2_21_cells_per_axis():
    from surf_amd._lib import SurfHipError
    with pytest.raises(SurfHipError, match="limit"):
        F.voxel_mean(np.array([[0.0, 0, 0], [3e6, 0, 0]]), 1.0, device="gpu")


@pytest.mark.parametrize("r", [1, 1300])
@pytest.mark.parametrize("n", SIZES)
def test_nearest_equals_host(n, r):
    ref = cloud(r, seed=1)
    q = cloud(n, seed=2).copy()
    q[0] = ref.max(axis=0) + [0.9, 0.0, 0.0]                                     # outside the reference's box by more than max_dist
    max_dist = 0.6
    _, _, d2 = H.brute_nearest(q, ref)
    assert r == 1 or H.no_ties(d2)
    want_d, want_i = F.nearest(q, ref, max_dist)
    got_d, got_i = F.nearest(q, ref, max_dist, device="gpu")
    assert got_i.dtype == np.int64 and np.array_equal(bits(got_d), bits(want_d)) and np.array_equal(got_i, want_i)
    assert np.isposinf(got_d[0]) and got_i[0] == -1
    assert n < 64 or r == 1 or (np.isfinite(got_d).sum() > n // 2 and np.isposinf(got_d).sum() > 0)


def test_nearest_empty_and_ties():
    q = cloud(65)
    d, i = F.nearest(q, np.zeros((0, 3)), 1.0, device="gpu")
    assert np.isposinf(d).all() and (i == -1).all() and d.shape == i.shape == (65,)
    d, i = F.nearest(np.zeros((0, 3)), q, 1.0, device="gpu")
    assert d.shape == i.shape == (0,)
    ref = np.concatenate([q[::-1], q, q])                                        # every point three times: the smallest index wins
    d, i = F.nearest(q, ref, 1.0, device="gpu")
    assert (d == 0).all() and np.array_equal(i, np.minimum(64 - np.arange(65), 65 + np.arange(65)))


@pytest.mark.parametrize("r", [1, 7, 300])
def test_nearest_distance_and_index_walks_agree(r):
    """The two instances of the one shell walk: nearest_dist_capped's distances equal nearest_capped_index's bit for bit, and the
    index attains that distance and is the smallest that does.  All coordinates lie on a 0.125 lattice, so squared distances are
    exact and tie exactly.  257 queries (one past a block): copies of reference points, the midpoint of two reference points that
    no other one is nearer to, two far outside the grid, one NaN, the rest scattered over the box and around it."""
    rng = np.random.default_rng(r)
    ref = rng.integers(-8, 9, (r, 3)) * 0.25
    if r >= 2:
        ref[0], ref[1] = (10.0, 10.0, 10.0), (10.5, 10.0, 10.0)
    q = rng.integers(-24, 25, (257, 3)) * 0.125
    q[:64] = ref[np.arange(64) % r]
    q[64] = (10.25, 10.0, 10.0)
    q[65], q[66] = (1.0e6, 0.0, 0.0), (0.25, -1.0e12, 3.0e9)
    q[67] = (np.nan, 0.0, 0.0)
    d = q[:, None, :] - ref[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[67] = np.inf                                                              # a NaN query has no neighbour
    best = d2.min(axis=1)
    assert r == 1 or ((d2 == best[:, None]).sum(axis=1)[64] == 2 and (d2[68:] == best[68:, None]).sum(axis=1).max() >= 2)
    tq, tref = torch.from_numpy(q).cuda(), torch.from_numpy(ref).cuda()

    def check(tq, d2, max_dist):
        best = d2.min(axis=1)
        dist = ops.nearest_dist_capped(tq, tref, max_dist)
        dist_i, index = ops.nearest_capped_index(tq, tref, max_dist)
        assert dist.dtype == torch.float64 and torch.equal(dist, dist_i)
        got_d, got_i = dist_i.cpu().numpy(), index.cpu().numpy()
        near = np.sqrt(best) < max_dist
        assert np.array_equal(np.isfinite(got_d), near) and np.isposinf(got_d[~near]).all() and (got_i[~near] == -1).all()
        assert np.array_equal(bits(got_d[near]), bits(np.sqrt(best[near])))
        assert np.array_equal(got_i[near], np.argmin(d2[near], axis=1))         # argmin: the first, i.e. smallest, index
        return near

    near = check(tq, d2, 0.75)
    assert near[:64].all() and near[64] == (r > 1) and not near[65:68].any() and 0 < near[68:].sum() < 189
    apart = best > 0                                                             # below the smallest distance: nothing is near
    assert not check(tq[torch.from_numpy(apart).cuda()].contiguous(), d2[apart], 0.5 * np.sqrt(best[apart].min())).any()
    near = check(tq, d2, 0.0625)                                                 # with them, only the copies (distance 0) are
    assert near[:64].all() and not near[64:].any()


@pytest.mark.parametrize("offset", H.ICP_OFFSETS)
def test_icp_recovers_the_motion(offset):
    """The host test's two cases against the same truth and the same bound (not against the host's transform)."""
    src, tgt = H.icp_pair(offset)
    T, fitness, rmse, iterations = F.icp(src, tgt, np.eye(4), 0.2, device="gpu")
    err = np.abs(F.transform_points(src, T) - tgt).max()
    print(f"icp (gpu) offset {offset}: {iterations} iterations, fitness {fitness}, rmse {rmse:.3e}, max error {err:.3e}")
    assert fitness == 1.0 and 0 < iterations <= 20
    assert err < 1e-9


@pytest.mark.parametrize("n", [1, 257, 5000, 300000])
def test_icp_reductions_repeat_bit_for_bit_and_match_float64(n):
    """300,000 pairs take more workgroups than there are slots (a grid-stride pass)."""
    g = np.random.default_rng(n)
    src = g.standard_normal((n, 3)) + [100.0, -50.0, 25.0]
    tgt = g.standard_normal((max(n // 2, 1), 3)) + [100.0, -50.0, 25.0]
    index = g.integers(-1, len(tgt), n)
    index[0] = 0
    dist = g.uniform(0, 1, n)
    S, Tg, I, D = (torch.from_numpy(a).to("cuda") for a in (src, tgt, index, dist))
    assert n <= 256 * ops.FSCORE_ICP_SLOTS or n == 300000
    sums = [ops.fscore_icp_sums(S, Tg, I, D).cpu().numpy() for _ in range(2)]
    assert np.array_equal(bits(sums[0]), bits(sums[1]))
    pair = index >= 0
    want = np.concatenate([[pair.sum()], src[pair].sum(0), tgt[index[pair]].sum(0), [(dist[pair] ** 2).sum()]])
    # float64 sums of n terms in another order: n eps relative to the sum of magnitudes
    scale = np.concatenate([[1.0], np.abs(src[pair]).sum(0), np.abs(tgt[index[pair]]).sum(0), [(dist[pair] ** 2).sum()]])
    assert sums[0][0] == want[0] and (np.abs(sums[0] - want) <= n * 2.3e-16 * scale).all()
    cs, ct = want[1:4] / want[0], want[4:7] / want[0]
    cov = [ops.fscore_icp_cov(S, Tg, I, cs, ct).cpu().numpy() for _ in range(2)]
    assert cov[0].shape == (3, 3) and np.array_equal(bits(cov[0]), bits(cov[1]))
    a, b = src[pair] - cs, tgt[index[pair]] - ct
    assert (np.abs(cov[0] - a.T @ b) <= n * 2.3e-16 * (np.abs(a).T @ np.abs(b)) + 1e-300).all()


def test_protocol_equals_host():
    pred, gt = H.protocol_case()
    host = H.protocol_host()
    dev = F.evaluate_points(pred, gt, H.PROTOCOL_TAU, taus=H.PROTOCOL_TAUS, device="gpu")
    for key in ("precision", "recall", "fscore", "taus", "curve_precision", "curve_recall", "counts"):
        assert dev[key] == host[key], key
    assert np.abs(np.array(dev["transform"]) - np.array(host["transform"])).max() < 1e-9
    assert np.abs(np.array(dev["transform"]) - H.true_transform()).max() < 1e-9
    assert [r["iterations"] for r in dev["icp"]] == [r["iterations"] for r in host["icp"]]
    fixed = F.evaluate_points(pred, gt, H.PROTOCOL_TAU, transform=H.true_transform(), refine=False, taus=H.PROTOCOL_TAUS, device="gpu")
    want = H.protocol_host(refine=False)
    for key in ("precision", "recall", "fscore", "taus", "curve_precision", "curve_recall", "counts"):
        assert fixed[key] == want[key], key
    crop = F.CropVolume("Y", -0.3, 0.35, np.array([[-0.9, 0, -1], [0.7, 0, -1], [0.9, 0, 1], [-0.2, 0, 0.1], [-0.9, 0, 1]]))
    a = F.evaluate_points(pred, gt, H.PROTOCOL_TAU, transform=H.true_transform(), refine=False, crop=crop, device="gpu")
    b = F.evaluate_points(pred, gt, H.PROTOCOL_TAU, transform=H.true_transform(), refine=False, crop=crop)
    assert a["counts"] == b["counts"] and 0 < a["counts"]["gt_cropped"] < len(gt)
    assert (a["precision"], a["recall"], a["curve_recall"]) == (b["precision"], b["recall"], b["curve_recall"])


def _scripts():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import fuse_scene
    return fuse_scene


def test_fuse_scene_script_scene(tmp_path):
    """scripts/fuse_scene.py --scene Family on the synthetic Tanks and Temples scene, the U-Nets' logits replaced by the sphere
    field, scored against points sampled from that sphere (radius 0.5 in the first group's normalised frame)."""
    from bench import surf_conf
    from surf_amd import conf as C
    from surf_amd.datasets import get_loader
    from tests.golden.dtu_scene import TANKS_CONF, ring_cams, write_cam, write_tanks_scene
    root = tmp_path / "tnt"
    write_tanks_scene(str(root), hw=(96, 128), with_masks=())
    # that fixture serves the reader's tests: its ring climbs 20 units per view at a radius of 4, so its views share no surface.
    # The cameras are written again as the synthetic DTU scene's rig (ring of 600, 425 + 192 x 2.5 deep, same field of view), 1 : 150
    K = np.array([[2892.33 * 1920 / 1600, 0, 960.0], [0, 2883.18 * 1080 / 1200, 540.0], [0, 0, 1.0]])
    for v, w2c in enumerate(ring_cams(4)):
        c2w = np.linalg.inv(w2c)
        c2w[:3, 3] /= 150.0
        write_cam(str(root / "Family" / "cams" / f"{v:08d}_cam.txt"), np.linalg.inv(c2w), K, 425.0 / 150, 2.5 / 150)
    dconf = dict(TANKS_CONF, data_dir=str(root), ref_view=[1], img_hw=[96, 128])
    conf_path = tmp_path / "tanks.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    scale_mat = get_loader(C.from_dict(dconf), "val", False, num_workers=0)[2][0]["scale_mat"].numpy().astype(np.float64)
    g = np.random.default_rng(0)
    d = g.standard_normal((20000, 3))
    scale = np.linalg.norm(scale_mat[:3, 0])                                     # scale_mat = the reference camera's pose x the fit
    sphere = scale_mat[:3, 3] + 0.5 * scale * d / np.linalg.norm(d, axis=1, keepdims=True)
    half = 2.0 * scale
    c = scale_mat[:3, 3]
    box = F.CropVolume("Z", c[2] - half, c[2] + half, np.array([[c[0] - half, c[1] - half, 0], [c[0] + half, c[1] - half, 0],
                                                               [c[0] + half, c[1] + half, 0], [c[0] - half, c[1] + half, 0]]))
    H.write_tnt_ground_truth(tmp_path / "gt", "Family", sphere, np.eye(4), box)
    fuse_scene = _scripts()
    tau = 0.05 * scale
    rec = fuse_scene.run(fuse_scene.parse_args(["--conf", str(conf_path), "--scene", "Family", "--ref_views", "1", "2", "--resolution", "64",
                                                "--logit_override", "sphere", "--point_cloud", "--tnt_dir", str(tmp_path / "gt"),
                                                "--tau", str(tau), "--eval_device", "gpu", "--out_dir", str(tmp_path / "out")]))
    assert rec["scene"] == "Family" and "scan" not in rec
    for key in ("precision", "recall", "fscore", "pcd_precision", "pcd_recall", "pcd_fscore"):
        assert 0.0 <= rec[key] <= 1.0, key
    print(f"fuse_scene --scene Family: mesh P/R/F {rec['precision']:.3f} {rec['recall']:.3f} {rec['fscore']:.3f}, cloud "
          f"{rec['pcd_precision']:.3f} {rec['pcd_recall']:.3f} {rec['pcd_fscore']:.3f} in {rec['ms']['evaluate_fscore']:.0f} ms")
    assert rec["ms"]["evaluate_fscore"] > 0.0
    fused = tmp_path / "out" / "meshes" / "fused"
    assert rec["mesh"] == str(fused / "Family.ply") and rec["points_file"] == str(fused / "Family_points.ply")
    assert os.path.exists(rec["mesh"]) and os.path.exists(rec["points_file"])
    assert json.load(open(tmp_path / "out" / "fused_Family.json"))["fscore"] == rec["fscore"]
    with pytest.raises(SystemExit, match="--scan"):
        fuse_scene.run(fuse_scene.parse_args(["--conf", str(conf_path), "--scene", "Family", "--eval_dir", str(tmp_path)]))
    with pytest.raises(SystemExit):
        fuse_scene.parse_args(["--conf", str(conf_path), "--scene", "Family", "--scan", "37"])


def test_fuse_scene_script_scan_is_unchanged(tmp_path):
    """A --scan run keeps the parent commit's record keys and file names, also when the Namespace is built by hand without the
    new attributes."""
    from bench import surf_conf
    from tests.test_end_to_end_dtu import _write_scene
    Hh, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, Hh, W)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [Hh, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    fuse_scene = _scripts()
    args = fuse_scene.parse_args(["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--resolution", "64",
                                  "--logit_override", "sphere", "--point_cloud", "--out_dir", str(tmp_path / "out")])
    for new in ("scene", "tnt_dir", "tau", "no_refine"):
        delattr(args, new)
    rec = fuse_scene.run(args)
    assert set(rec) == {"scan", "views_fused", "lattice", "voxel", "trunc", "observed_share", "vertices", "triangles", "depth", "colors",
                        "cleaned", "mesh", "ms", "points", "points_file"}
    assert set(rec["ms"]) == {"load", "lattice", "forward", "integrate", "points", "extract", "write"}
    assert rec["scan"] == 24
    fused = tmp_path / "out" / "meshes" / "fused"
    assert rec["mesh"] == str(fused / "scan24.ply") and rec["points_file"] == str(fused / "scan24_points.ply")
    assert sorted(os.listdir(fused)) == ["scan24.ply", "scan24_points.ply"] and os.path.exists(tmp_path / "out" / "fused_scan24.json")
    assert len(mesh_io.read_ply(rec["mesh"])[0]) == rec["vertices"] > 100
