"""CPU: the host path of surf_amd.evaluation.fscore (Tanks and Temples crop / voxel mean / nearest / ICP / F-score) against
independent brute force - Python loops and the full O(nm) float64 distance table - never against the device path; the CLI on a
scene written in the benchmark's layout.  The inputs below are shared with tests/test_fscore_gpu.py."""
import functools
import json

import numpy as np
import pytest

from surf_amd import mesh_io
from surf_amd.evaluation import fscore as F

L_POLYGON = [(0, 0), (4, 0), (4, 1), (1, 1), (1, 3), (0, 3)]


def l_crop(axis, axis_min=-0.5, axis_max=0.75):
    """The six-vertex L polygon in the plane orthogonal to `axis` ("X", "Y" or "Z"), its vertices as 3-D points."""
    a = "XYZ".index(axis)
    u, v = [k for k in range(3) if k != a]
    poly = np.zeros((len(L_POLYGON), 3))
    poly[:, u] = [p[0] for p in L_POLYGON]
    poly[:, v] = [p[1] for p in L_POLYGON]
    return F.CropVolume(axis, axis_min, axis_max, poly)


def l_lattice(axis):
    """Quarter-step lattice offset by one eighth over [-1, 5]^2 (no point on an edge of the L), at five heights along `axis`
    that include axis_min and axis_max themselves.  Returns (points, expected keep)."""
    a = "XYZ".index(axis)
    ua, va = [k for k in range(3) if k != a]
    s = np.arange(-1 + 0.125, 5, 0.25)
    h = np.array([-0.75, -0.5, 0.0, 0.75, 1.0])
    u, v, w = (t.reshape(-1) for t in np.meshgrid(s, s, h, indexing="ij"))
    p = np.zeros((len(u), 3))
    p[:, ua], p[:, va], p[:, a] = u, v, w
    in_l = ((0 < u) & (u < 4) & (0 < v) & (v < 1)) | ((0 < u) & (u < 1) & (0 < v) & (v < 3))     # the union of two rectangles
    return p, in_l & (-0.5 <= w) & (w <= 0.75)


def rotation(axis, degrees):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(degrees)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def surface(x, y):
    return 0.3 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * x * y + 0.1 * x * x


ICP_OFFSETS = [(0.0, 0.0, 0.0), (1000.0, -500.0, 250.0)]


@functools.lru_cache(maxsize=None)
def icp_pair(offset=(0.0, 0.0, 0.0)):
    """(source, target): 3,000 points of the bumpy surface at uniformly random (x, y) in [-1,1] x [-0.7,0.7] (a regular lattice
    would give ICP a local minimum one lattice step off), and the same points under a 2 degree rotation about (0.3, 1, 0.2) plus
    the translation (0.02, -0.015, 0.01); then both clouds shifted by `offset`."""
    g = np.random.default_rng(7)
    x, y = g.uniform(-1, 1, 3000), g.uniform(-0.7, 0.7, 3000)
    src = np.stack([x, y, surface(x, y)], axis=1)
    tgt = src @ rotation((0.3, 1.0, 0.2), 2.0).T + np.array([0.02, -0.015, 0.01])
    off = np.asarray(offset, dtype=np.float64)
    src, tgt = src + off, tgt + off
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt


def true_transform():
    T = np.eye(4)
    T[:3, :3] = rotation((0.3, 1.0, 0.2), 2.0)
    T[:3, 3] = [0.02, -0.015, 0.01]
    return T


PROTOCOL_TAU = 0.004
PROTOCOL_TAUS = (0.002, 0.008, 0.016)
# 3 tau, plus half a bin of the cumulative curves: at 3 tau exactly the displaced points' distances sit ON the curves' edge 300,
# where the last bit of the transform (which the two paths do not share) decides the bin
PROTOCOL_SHIFT = 3 * PROTOCOL_TAU + PROTOCOL_TAU / 200


@functools.lru_cache(maxsize=None)
def protocol_case():
    """(pred, gt): the ICP pair with the strip x > 0.8 (10 % of the target's area) missing from the prediction and 5 % of the
    prediction displaced by 3 tau (PROTOCOL_SHIFT) along z.  The displaced points are drawn from those with no other point
    within 6 tau, so that none of them lands within 2 tau of another surface point: the last ICP round (max_dist 2 tau) then
    sees inliers only and its fixed point is the true motion."""
    src, tgt = icp_pair()
    g = np.random.default_rng(11)
    pred = src[src[:, 0] <= 0.8].copy()
    d2 = brute_nearest(src[src[:, 0] <= 0.8], src)[2]
    alone = np.nonzero(np.sqrt(np.partition(d2, 1, axis=1)[:, 1]) > 6 * PROTOCOL_TAU)[0]
    moved = g.permutation(alone)[:len(pred) // 20]
    assert len(moved) == len(pred) // 20
    pred[moved, 2] += PROTOCOL_SHIFT
    pred.setflags(write=False)
    return pred, tgt


def brute_nearest(q, ref):
    """(distance, index, table) from the full float64 table of (dx*dx + dy*dy) + dz*dz."""
    d = q[:, None, :] - ref[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(d2.min(axis=1)), d2.argmin(axis=1), d2


def no_ties(d2):
    two = np.partition(d2, 1, axis=1)[:, :2]
    return bool((two[:, 0] < two[:, 1]).all())


@functools.lru_cache(maxsize=None)
def protocol_host(refine=True):
    pred, gt = protocol_case()
    return F.evaluate_points(pred, gt, PROTOCOL_TAU, transform=None if refine else true_transform(), refine=refine, taus=PROTOCOL_TAUS)


def voxel_cloud():
    """20,000 normal points, 400 packed into one voxel of 0.25, one isolated point."""
    g = np.random.default_rng(3)
    return np.concatenate([g.standard_normal((20000, 3)), np.array([5.3, 5.3, 5.3]) + g.uniform(0, 0.01, (400, 3)),
                           [[40.0, -37.0, 11.0]]])


def voxel_mean_loop(p, voxel):
    """Open3D's rule with a per-point Python loop: sums grow in input order, cells come out in ascending key order."""
    origin = p.min(axis=0) - voxel / 2
    sums, counts = {}, {}
    for row in p:
        c = np.floor((row - origin) / voxel).astype(np.int64)
        key = (int(c[0]) << 42) | (int(c[1]) << 21) | int(c[2])
        if key not in sums:
            sums[key], counts[key] = np.zeros(3), 0
        sums[key] = sums[key] + row
        counts[key] += 1
    return np.array([sums[k] / counts[k] for k in sorted(sums)])


# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", ["X", "Y", "Z"])
def test_crop_l_polygon(axis):
    p, want = l_lattice(axis)
    keep = F.crop_points(p, l_crop(axis))
    assert keep.dtype == bool and keep.shape == (len(p),)
    assert 0 < want.sum() < len(p) and np.array_equal(keep, want)
    a = "XYZ".index(axis)
    assert keep[(p[:, a] == -0.5) & want].any() and keep[(p[:, a] == 0.75) & want].any()      # the axis range is closed


def test_read_crop_volume(tmp_path):
    crop = l_crop("Y")
    path = tmp_path / "crop.json"
    path.write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "Y", "axis_min": crop.axis_min,
                                "axis_max": crop.axis_max, "bounding_polygon": crop.polygon.tolist(), "version_major": 1}))
    got = F.read_crop_volume(str(path))
    assert got.axis == "Y" and got.axis_min == crop.axis_min and got.axis_max == crop.axis_max
    assert np.array_equal(got.polygon, crop.polygon)


@pytest.mark.parametrize("case", ["mixed", "single", "one_voxel"])
def test_voxel_mean_equals_the_loop(case):
    p = {"mixed": voxel_cloud, "single": lambda: np.array([[0.3, -1.2, 7.0]]),
         "one_voxel": lambda: np.random.default_rng(4).uniform(0, 0.12, (500, 3))}[case]()   # < voxel / 2 wide
    got = F.voxel_mean(p, 0.25)
    want = voxel_mean_loop(p, 0.25)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if case != "mixed":
        assert len(got) == 1
    else:
        cells = np.floor((p - (p.min(axis=0) - 0.125)) / 0.25).astype(np.int64)
        counts = np.unique(cells, axis=0, return_counts=True)[1]
        assert counts.max() >= 400 and (counts == 1).sum() > 100 and len(counts) == len(got)


def test_voxel_mean_refuses_more_than_2_21_cells_per_axis():
    with pytest.raises(ValueError, match="2097152"):
        F.voxel_mean(np.array([[0.0, 0, 0], [3e6, 0, 0]]), 1.0)


def test_nearest_equals_the_table():
    g = np.random.default_rng(5)
    ref = g.uniform(-1, 1, (1300, 3))
    q = np.concatenate([g.uniform(-1.1, 1.1, (697, 3)), [[3.0, 0, 0], [0, -4.0, 0], [2.5, 2.5, 2.5]]])
    dist, index, d2 = brute_nearest(q, ref)
    assert no_ties(d2)
    max_dist = 0.5
    got_d, got_i = F.nearest(q, ref, max_dist)
    near = dist < max_dist
    assert got_d.dtype == np.float64 and got_i.dtype == np.int64 and near[:697].all() and not near[697:].any()
    assert np.array_equal(got_d[near].view(np.uint64), dist[near].view(np.uint64)) and np.array_equal(got_i[near], index[near])
    assert np.isposinf(got_d[~near]).all() and (got_i[~near] == -1).all()
    d, i = F.nearest(q, np.zeros((0, 3)), max_dist)
    assert np.isposinf(d).all() and (i == -1).all() and d.shape == i.shape == (len(q),)
    with pytest.raises(ValueError, match="device"):
        F.nearest(q, ref, max_dist, device="tpu")


def test_scores_pin_the_strict_comparison_and_the_denominators():
    tau = 0.01
    below = np.nextafter(tau, 0)
    d1 = np.array([tau, below, np.inf, 0.0, 2 * tau])              # 2 of 5 strictly below
    d2 = np.array([below, below, tau, np.inf])                     # 2 of 4
    p, r, f = F.fscore(d1, d2, tau)
    assert (p, r) == (2 / 5, 2 / 4) and f == 2 * p * r / (p + r)
    assert F.fscore(np.array([tau, np.inf]), np.array([tau]), tau) == (0.0, 0.0, 0.0)
    g = np.random.default_rng(6)
    d = np.concatenate([g.uniform(0, 6 * tau, 1000), [np.inf] * 7])
    hist, _ = np.histogram(d[np.isfinite(d)], np.arange(0, 5 * tau, tau / 100))
    assert np.array_equal(F.cumulative_curve(d, tau), np.cumsum(hist) / len(d))
    assert len(F.cumulative_curve(d, tau)) == len(np.arange(0, 5 * tau, tau / 100)) - 1


@pytest.mark.parametrize("offset", ICP_OFFSETS)
def test_icp_recovers_the_motion(offset):
    """Noise-free correspondences: the fixed point is exact, and what is left is float64 rounding of ~3e3 terms at coordinates
    <= 1e3, about 1e-12; 1e-9 leaves three orders of margin."""
    src, tgt = icp_pair(offset)
    T, fitness, rmse, iterations = F.icp(src, tgt, np.eye(4), 0.2)
    err = np.abs(F.transform_points(src, T) - tgt).max()
    print(f"icp offset {offset}: {iterations} iterations, fitness {fitness}, rmse {rmse:.3e}, max error {err:.3e}")
    assert fitness == 1.0 and 0 < iterations <= 20
    assert err < 1e-9


def brute_tallies(pred, gt, T, tau, taus):
    """The pipeline after the alignment with brute-force distances: transform, voxel mean at tau / 2, the full table."""
    pv, gv = F.voxel_mean(F.transform_points(pred, T), tau / 2), F.voxel_mean(gt, tau / 2)
    d1, _, _ = brute_nearest(pv, gv)
    d2, _, _ = brute_nearest(gv, pv)
    edges = np.concatenate([np.arange(0, 5 * tau, tau / 100), (tau,) + tuple(taus)])
    for d in (d1, d2):              # a last-bit difference in the transform cannot flip a tally, nor a bin of the curves
        assert (np.abs(d[d > 1e-6 * tau, None] - edges[None, :]) > 1e-6 * tau).all()
    return [(np.count_nonzero(d1 < t) / len(d1), np.count_nonzero(d2 < t) / len(d2)) for t in (tau,) + tuple(taus)], d1, d2


def test_protocol_equals_brute_force():
    pred, gt = protocol_case()
    out = protocol_host()
    tallies, d1, d2 = brute_tallies(pred, gt, np.array(out["transform"]), PROTOCOL_TAU, PROTOCOL_TAUS)
    assert (out["precision"], out["recall"]) == tallies[0]
    assert 0.9 < out["precision"] < 0.96 and 0.85 < out["recall"] < 0.93        # 5 % displaced; 10 % of the target not covered
    assert out["fscore"] == 2 * out["precision"] * out["recall"] / (out["precision"] + out["recall"])
    assert [(e["precision"], e["recall"]) for e in out["taus"]] == tallies[1:] and [e["tau"] for e in out["taus"]] == list(PROTOCOL_TAUS)
    cap = 5 * max(PROTOCOL_TAUS)                                                     # the distances are capped there
    for key, d in (("curve_precision", d1), ("curve_recall", d2)):
        hist, _ = np.histogram(d[d < cap], np.arange(0, 5 * PROTOCOL_TAU, PROTOCOL_TAU / 100))
        assert np.array_equal(np.array(out[key]), np.cumsum(hist) / len(d))
    assert np.abs(np.array(out["transform"]) - true_transform()).max() < 1e-9
    assert len(out["icp"]) == 3 and all(r["iterations"] <= 20 for r in out["icp"]) and out["icp"][2]["rmse"] < 1e-9
    assert out["counts"]["pred"] == len(pred) and len(gt) - 20 < out["counts"]["gt_voxel"] <= len(gt) and set(out["ms"]) >= {"icp", "nearest"}
    fixed = protocol_host(refine=False)
    assert (fixed["precision"], fixed["recall"]) == tallies[0] and fixed["icp"] == []
    assert [(e["precision"], e["recall"]) for e in fixed["taus"]] == tallies[1:]


def test_empty_crop_names_the_stage():
    pred, gt = protocol_case()
    with pytest.raises(ValueError, match="ground truth"):
        F.evaluate_points(pred, gt, PROTOCOL_TAU, crop=l_crop("Z", 50.0, 60.0))
    with pytest.raises(ValueError, match="device"):
        F.evaluate_points(pred, gt, PROTOCOL_TAU, device="cuda")


def write_tnt_ground_truth(gt_dir, scene, gt, T, crop):
    """<gt_dir>/<scene>/<scene>.ply, .json, _trans.txt in the benchmark's layout."""
    d = gt_dir / scene
    d.mkdir(parents=True)
    mesh_io.write_ply_points(str(d / f"{scene}.ply"), gt)
    (d / f"{scene}.json").write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": crop.axis,
                                                 "axis_min": crop.axis_min, "axis_max": crop.axis_max,
                                                 "bounding_polygon": crop.polygon.tolist(), "version_major": 1, "version_minor": 0}))
    np.savetxt(str(d / f"{scene}_trans.txt"), T)


def test_cli_prints_one_json_line(tmp_path, capsys):
    pred, gt = protocol_case()
    box = F.CropVolume("Z", -1.0, 1.0, np.array([[-2.0, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]]))
    write_tnt_ground_truth(tmp_path / "gt", "Barn", gt, true_transform(), box)
    mesh_io.write_ply_points(str(tmp_path / "pred.ply"), pred)
    F.main(["--pred", str(tmp_path / "pred.ply"), "--gt_dir", str(tmp_path / "gt"), "--scene", "Barn", "--no_refine", "--taus", "0.02"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["scene"] == "Barn" and rec["tau"] == F.SCENE_TAU["Barn"] == 0.01 and rec["mode"] == "pcd" and rec["icp"] == []
    assert {"precision", "recall", "fscore", "taus", "curve_precision", "curve_recall", "transform", "counts", "ms"} <= set(rec)
    assert 0.9 < rec["precision"] <= 1.0 and 0.85 < rec["recall"] <= 1.0 and rec["taus"][0]["tau"] == 0.02
    assert F.SCENE_TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003,
                           "Meetingroom": 0.01, "Truck": 0.005}
    with pytest.raises(ValueError, match="tau"):
        F.evaluate_scene(str(tmp_path / "pred.ply"), str(tmp_path / "gt"), "Family")
