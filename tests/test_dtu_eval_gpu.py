"""The device path of the DTU Chamfer evaluation (surf_amd/csrc/dtu_eval.hip, dtu_eval.py device="gpu").

CPU tests: the C ABI exports the new entry points, and the two facts the device path relies on are pinned (rng.permutation
is the order rng.shuffle applies; scikit-learn's radius_neighbors includes a point at exactly the radius).
GPU tests: the golden numbers of the reference evaluator, bit-identity with the numpy / scikit-learn pieces (samples, kept set
and its order, nearest-neighbour distances) and the --eval_device switch of scripts/dtu_chamfer.py."""
import json
import os
import re

import numpy as np
import pytest
import sklearn.neighbors as skln

from surf_amd.evaluation import dtu_eval as E

DTU_SYMBOLS = ["surf_dtu_sample_count", "surf_dtu_sample_write", "surf_dtu_cell_keys", "surf_dtu_thin_round", "surf_dtu_nearest"]


def test_library_exports_the_dtu_eval_entry_points():
    from surf_amd import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "surf_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(surf_\w+)\s*\(", hdr, flags=re.M))
    L = _lib.lib()
    for name in DTU_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(L, name)
    assert L.surf_abi_version() == _lib.ABI_VERSION == 41


@pytest.mark.parametrize("n", [0, 1, 2, 7, 1000, 65537])
def test_permutation_is_the_order_shuffle_applies(n):
    """rng.permutation(n) == the row order rng.shuffle(points, axis=0) leaves, and both consume the generator alike."""
    for seed in (0, 123, 2 ** 40 + 5):
        pts = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
        g1, g2 = np.random.default_rng(seed), np.random.default_rng(seed)
        shuffled = pts.copy()
        g1.shuffle(shuffled, axis=0)
        perm = g2.permutation(n)
        assert np.array_equal(shuffled, pts[perm])
        assert g1.integers(1 << 62) == g2.integers(1 << 62)


def test_radius_neighbors_includes_points_at_exactly_the_radius():
    """scikit-learn's kd-tree radius test is <= : the device thinning compares (dx*dx + dy*dy) + dz*dz <= thresh*thresh."""
    line = np.array([[0.0, 0, 0], [0.5, 0, 0], [1.0, 0, 0]])
    nn = skln.NearestNeighbors(radius=1.0, algorithm="kd_tree").fit(line)
    assert all(sorted(r.tolist()) == [0, 1, 2] for r in nn.radius_neighbors(line, return_distance=False))
    lattice = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    nn = skln.NearestNeighbors(radius=1.0, algorithm="kd_tree").fit(lattice)
    got = nn.radius_neighbors(lattice, return_distance=False)
    for i, p in enumerate(lattice):
        want = np.nonzero(((lattice - p) ** 2).sum(-1) <= 1.0)[0]
        assert sorted(got[i].tolist()) == want.tolist()
        assert len(want) == 1 + sum(1 for a in range(3) for s in (-1, 1) if 0 <= p[a] + s <= 3)


# ---------------------------------------------------------------------------------------------------------------- GPU --

def _meshes():
    from tests.golden import eval_scene
    from tests.test_evaluation import _sphere_mesh
    out = []
    for k in (0, 7, 14):                                    # the synthetic ellipsoids (degenerate triangles at the poles)
        v, t = eval_scene._mesh(40.0 + 3.0 * k, np.array([5.0 * k, -3.0 * k, 10.0 + k]), 0.8 + 0.02 * k)
        out.append((v, t, 2.5))
    v, t = _sphere_mesh(50.0, 36)                           # the marching-cubes sphere
    out.append((v.astype(np.float32), t, 0.5))
    return out


@pytest.mark.gpu
def test_sampling_and_thinning_equal_the_cpu_pieces():
    cases = _meshes()
    from tests.test_evaluation import _sphere_mesh
    v, t = _sphere_mesh(100.0, 96)                          # >= 1 M samples
    cases.append((v.astype(np.float32), t, 0.25))
    big = 0
    for v, t, thresh in cases:
        ref = E.sample_mesh_points(v, t, thresh)
        got = E.sample_mesh_points_gpu(v, t, thresh).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, ref), (len(got), len(ref))
        big = max(big, len(ref))
        want = E.downsample_points(ref, thresh, np.random.default_rng(5))
        down = E.downsample_points_gpu(got, thresh, np.random.default_rng(5)).cpu().numpy()
        assert np.array_equal(down, want), (len(down), len(want))
    assert big >= 1_000_000


@pytest.mark.gpu
def test_thinning_on_ties_equals_the_cpu_greedy_pass():
    """Points of an integer lattice, some moved by a little jitter and some duplicated: many pairs at exactly thresh = 1."""
    g = np.random.default_rng(3)
    pts = np.stack(np.meshgrid(*[np.arange(20.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    jit = g.random(len(pts)) < 0.3
    pts[jit] += g.normal(0, 0.05, (int(jit.sum()), 3))
    pts = np.concatenate([pts, pts[g.integers(0, len(pts), 500)]])
    for seed in (0, 1, 2):
        want = E.downsample_points(pts, 1.0, np.random.default_rng(seed))
        got = E.downsample_points_gpu(pts, 1.0, np.random.default_rng(seed)).cpu().numpy()
        assert np.array_equal(got, want), (len(got), len(want))


def _sk_dist(ref, q):
    return skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(ref).kneighbors(q, n_neighbors=1)[0][:, 0]


@pytest.mark.gpu
def test_capped_nearest_neighbour_equals_kneighbors():
    import torch
    from surf_amd import ops
    g = np.random.default_rng(0)
    d = g.standard_normal((40000, 3))
    ref = (d / np.linalg.norm(d, axis=1, keepdims=True) * 50.0 + g.normal(0, 0.3, (40000, 3))).astype(np.float32).astype(np.float64)
    q = np.concatenate([g.standard_normal((30000, 3)) * 40.0,            # inside and around the cloud
                        g.uniform(-500, 500, (3000, 3)),                  # far outside its box
                        ref[:2000] + g.normal(0, 1e-3, (2000, 3)),        # next to reference points
                        ref[2000:2100]])                                  # on them (distance 0)
    for max_dist in (20.0, 3.0, 0.5):
        want = _sk_dist(ref, q)
        got = ops.nearest_dist_capped(torch.from_numpy(q).cuda(), torch.from_numpy(ref).cuda(), max_dist).cpu().numpy()
        near = want < max_dist
        assert 0 < near.sum() < len(q)
        assert np.all(np.abs(got[near] - want[near]) <= 1e-15 * want[near])
        assert np.all(np.isinf(got[~near]))
    # a reference cloud of one point
    one = np.array([[1.0, -2.0, 3.0]])
    want = _sk_dist(one, q[:5000])
    got = ops.nearest_dist_capped(torch.from_numpy(q[:5000]).cuda(), torch.from_numpy(one).cuda(), 60.0).cpu().numpy()
    near = want < 60.0
    assert 0 < near.sum() < 5000 and np.array_equal(got[near], want[near]) and np.all(np.isinf(got[~near]))


@pytest.mark.gpu
def test_empty_selection_is_nan_as_on_the_cpu():
    """Nothing within max_dist: the CPU path's mean of an empty selection is nan, and so is the device path's."""
    g = np.random.default_rng(1)
    v, t = _meshes()[0][:2]
    stl = g.normal(0, 1.0, (500, 3)) + np.array([1000.0, 0, 0])           # far from the mesh
    obs = np.ones((8, 8, 8), np.uint8)
    BB = np.array([[-100.0, -100, -100], [100, 100, 100]], np.float32)
    plane = np.array([[0.0, 0.0, 0.0, 1.0]])                               # every point "above"
    kw = dict(patch_size=60, max_dist=20, downsample_density=2.5)
    with pytest.warns(RuntimeWarning):
        cpu = E.chamfer_dtu(E.sample_mesh_points(v, t, 2.5), stl, obs, BB, np.float32(25.0), plane, rng=np.random.default_rng(0), **kw)
    gpu = E.chamfer_dtu(E.sample_mesh_points_gpu(v, t, 2.5), stl, obs, BB, np.float32(25.0), plane, rng=np.random.default_rng(0),
                        device="gpu", **kw)
    assert all(np.isnan(x) for x in cpu) and all(np.isnan(x) for x in gpu)


@pytest.mark.gpu
def test_gpu_evaluator_equals_the_reference_evaluator(tmp_path):
    """tests/golden/dtu_eval_results.json (the reference's own results.json for the fifteen synthetic scans) with device="gpu",
    to the tolerance the CPU path is held to; the command line with --device gpu writes the same file."""
    from tests.golden import eval_scene
    with open(os.path.join(os.path.dirname(__file__), "golden", "dtu_eval_results.json")) as f:
        gold = json.load(f)
    out_dir, data_dir = str(tmp_path / "exp"), str(tmp_path / "eval")
    eval_scene.write_eval_scene(out_dir, data_dir)
    rows = []
    for scan in eval_scene.SCANS:
        d2s, s2d, overall = E.evaluate_scan(os.path.join(out_dir, "meshes", "final", f"scan{scan}.ply"), data_dir, scan, device="gpu",
                                            rng=np.random.default_rng(eval_scene.SHUFFLE_SEED), **eval_scene.ARGS)
        ref = gold[str(scan)]
        for got, key in ((d2s, "d2s"), (s2d, "s2d"), (overall, "all")):
            assert abs(got - ref[key]) < 1e-9 * ref[key] + 1e-12, (scan, key, got, ref[key])
        rows.append((d2s, s2d, overall))
    m = np.mean(np.array(rows), axis=0)
    for got, key in zip(m, ("d2s", "s2d", "all")):
        assert abs(got - gold["mean"][key]) < 1e-9 * gold["mean"][key]
    E.main(["--out_dir", out_dir, "--dataset_dir", data_dir, "--downsample_density", str(eval_scene.ARGS["downsample_density"]),
            "--shuffle_seed", str(eval_scene.SHUFFLE_SEED), "--device", "gpu"])
    with open(os.path.join(out_dir, "results.json")) as f:
        mine = json.load(f)
    assert set(mine) == set(gold)
    for scan, row in gold.items():
        for key, val in row.items():
            assert abs(mine[scan][key] - val) < 1e-9 * val, (scan, key)


@pytest.mark.gpu
def test_dtu_chamfer_eval_device_gpu_equals_cpu(tmp_path):
    """scripts/dtu_chamfer.py --eval_device gpu on the synthetic DTU scene of tests/test_end_to_end_dtu.py: the same d2s, s2d
    and chamfer as --eval_device cpu."""
    import sys

    import torch
    from scipy.io import savemat
    from bench import surf_conf
    from surf_amd import conf, mesh_io, synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.surf import SuRF
    from tests.test_end_to_end_dtu import _write_scene
    dev = torch.device("cuda:0")
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = conf.from_dict({"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
                            "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192,
                            "img_hw": [H, W], "total_views": 4})
    loader, _, _ = get_loader(dconf, "val", False, num_workers=0)
    np.random.seed(0)
    item = next(iter(loader))
    inputs = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in item.items()}
    inputs["mesh_resolution"] = 128
    torch.manual_seed(0)
    mcfg = surf_conf(base_dim=16)
    model = SuRF(conf.from_dict(mcfg)).to(dev).eval()
    model.logit_override = synthetic.sphere_logit
    with torch.no_grad():
        out = model("val", inputs, cos_anneal_ratio=1.0, step=0)
    vw = mesh_io.export_mesh(str(tmp_path / "mesh.ply"), out["vertices"], out["triangles"], item["scale_mat"])
    centre_w = item["scale_mat"].double().numpy()[:3, 3]
    r_world = float(np.linalg.norm(vw - centre_w[None], axis=1).mean())
    # the evaluation files: the scan is the mesh surface pushed outwards, as in tests/test_end_to_end_dtu.py
    density = r_world / 60.0
    ev = tmp_path / "dtu_eval"
    os.makedirs(ev / "ObsMask")
    os.makedirs(ev / "Points" / "stl")
    surf = E.sample_mesh_points(vw, out["triangles"], density)
    radial = (surf - centre_w[None]) / np.linalg.norm(surf - centre_w[None], axis=1, keepdims=True)
    stl = surf + 6.0 * radial
    with open(ev / "Points" / "stl" / "stl024_total.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n").encode())
        f.write(np.ascontiguousarray(stl, dtype="<f4").tobytes())
    lo, hi = centre_w - 2 * r_world, centre_w + 2 * r_world
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8), "BB": np.stack([lo, hi]).astype(np.float32),
                                                  "Res": np.float32(4.0 * r_world / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, -centre_w[2]]])})     # the upper half is "above"
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": mcfg, "val_dataset": {k: dconf[k] for k in dconf}}, indent=1))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import dtu_chamfer
    recs = {}
    for where in ("cpu", "gpu"):
        recs[where] = dtu_chamfer.run(dtu_chamfer.parse_args([
            "--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--out_dir", str(tmp_path / where),
            "--mesh_resolution", "128", "--downsample_density", str(density), "--logit_override", "sphere", "--eval_device", where]))
    for key in ("d2s", "s2d", "chamfer"):
        a, b = recs["cpu"][key], recs["gpu"][key]
        assert np.isfinite(a) and abs(a - b) <= 1e-9 * abs(a), (key, a, b)
