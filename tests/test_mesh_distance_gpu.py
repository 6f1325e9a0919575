"""The device path of the mesh deviation (csrc/mesh_distance.hip, surf_amd.mesh_distance backend="device") against the host path,
bit for bit (uint64 views of the fp64 arrays), on the scenes of tests/mesh_distance_scenes.py.  Both paths evaluate the one fp64
operation sequence of include/surf_hip.h; the value is a minimum over all faces, so the two cell tables need not agree.  Nothing
here compares the device path with itself, except one run-twice check that the bits repeat."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from surf_amd import mesh_distance as md
from tests.mesh_distance_scenes import QUERY_COUNTS, REGION_MAX_DIST, REGION_QUERIES, REGION_TRIANGLE, big_sphere, queries, scenes
from tests.mesh_smooth_scenes import MESHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SCENES = scenes()
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    for g, w, part in zip(got, want, ("distance", "face", "closest")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, part)
        same = np.array_equal(bits(g), bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, (what, part, int((g != w).sum()))


def device(points, v, f, max_dist, **kw):
    return md.point_to_mesh(points, v, f, max_dist, backend="device", device=DEV, **kw)


@pytest.mark.parametrize("name", list(SCENES))
def test_device_equals_host(name):
    """Uncapped (the joint box's diagonal) and capped at a distance that some queries exceed, for 1, 63, 64, 65 and 257 queries:
    a query's answer does not depend on the others, so the host path runs once per cap."""
    v, f = SCENES[name]
    q = queries(v, f, max(QUERY_COUNTS), seed=len(name))
    if name == "one_face":
        q[:8] = REGION_QUERIES
    if name == "fan":
        q[:70] = v[0]                                                              # at the hub: a tie across the whole fan
    diag = md.joint_diagonal(q, v)
    full = md.point_to_mesh(q, v, f, diag)
    cap = REGION_MAX_DIST if name == "one_face" else float(np.median(full[0]))
    for max_dist in (diag, cap):
        want = full if max_dist == diag else md.point_to_mesh(q, v, f, max_dist)
        beyond = int(np.isinf(want[0]).sum())
        assert (beyond == 0) if max_dist == diag else (0 < beyond < len(q)), (name, max_dist, beyond)
        for count in QUERY_COUNTS:
            got = device(q[:count], v, f, max_dist)
            assert_same(got, tuple(w[:count] for w in want), (name, max_dist, count))
    if name == "fan":
        assert (full[1][:70] == 0).all() and (full[0][:70] == 0).all()
    assert_same(device(q, v, f, None), md.point_to_mesh(q, v, f), (name, "default max_dist"))
    size = float(np.ptp(v.astype(np.float64), axis=0).max())
    assert_same(device(q, v, f, diag, _cell=0.37 * size), full, (name, "coarse cells"))


def test_big_sphere_and_the_bits_repeat():
    v, f, q = big_sphere()
    diag = md.joint_diagonal(q, v)
    want = md.point_to_mesh(q, v, f, diag)
    got = device(q, v, f, diag)
    assert_same(got, want, "big sphere")
    assert_same(device(q, v, f, diag), got, "second run")
    cap = float(np.median(want[0]))
    assert_same(device(q, v, f, cap), md.point_to_mesh(q, v, f, cap), "big sphere, capped")


def test_tensors_stay_on_the_device():
    """return_tensors=True: device tensors in, device tensors out, and exactly ops.MESHDIST_HOST_READS = 2 reads of the device on
    the way - [face index range, finite, boxes] and the number of pairs - on a mesh whose table needs no growth; the `spanning`
    scene, whose large face asks for growths, reads once more per growth.  The inputs are untouched."""
    from surf_amd import ops
    v, f = MESHES["noisy_sphere"]
    q = queries(v, f, 1000, 1)
    want = md.point_to_mesh(q, v, f)
    tq, tv, tf = torch.from_numpy(q).to(DEV), torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    device(tq, tv, tf, None, return_tensors=True)                                  # warm the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = device(tq, tv, tf, None, return_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchron" in str(w.message).lower()]
    for w in syncs:
        print(f"{os.path.relpath(w.filename, ROOT)}:{w.lineno}: {w.message}")
    assert ops.MESHDIST_HOST_READS == 2 and len(syncs) == ops.MESHDIST_HOST_READS
    assert all(torch.is_tensor(t) and t.is_cuda for t in got)
    assert_same(tuple(t.cpu().numpy() for t in got), want, "tensors")
    assert np.array_equal(tq.cpu().numpy().view(np.uint32), q.view(np.uint32))
    assert np.array_equal(tv.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(tf.cpu().numpy(), f)
    empty = device(tq, tv, tf[:0], None, return_tensors=True)
    assert torch.isinf(empty[0]).all() and (empty[1] == -1).all() and torch.isinf(empty[2]).all()


def test_device_refusals_raise_like_the_host_path():
    v, f = MESHES["two_triangles"]
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="vertex 2 is not finite"):
            device(v, bad, f, None)
        with pytest.raises(ValueError, match="point 2 is not finite"):
            device(bad, v, f, None)
    with pytest.raises(ValueError, match=r"face indices span \[0, 4\]"):
        device(v, v, np.array([[0, 1, 4]], np.int32), None)
    with pytest.raises(ValueError, match=r"face indices span \[-1, 2\]"):
        device(v, v, np.array([[0, -1, 2]], np.int32), None)
    with pytest.raises(ValueError, match="max_dist"):
        device(v, v, f, 0.0)


def test_deviation_on_the_device_equals_the_host_dict():
    from surf_amd.mesh_simplify import simplify_mesh
    from surf_amd.mesh_smooth import smooth_mesh
    v, f = MESHES["noisy_sphere"]
    b = smooth_mesh(v, f, iterations=5)[0]
    sv, sf = simplify_mesh(b, f, 0.2)[:2]
    for (va, fa, vb, fb), max_dist in (((v, f, b, f), None), ((v, f, sv, sf), None), ((v, f, sv, sf), 0.01), ((v, f, v, f[:0]), None)):
        want = md.mesh_deviation(va, fa, vb, fb, max_dist)
        assert md.mesh_deviation(va, fa, vb, fb, max_dist, backend="device", device=DEV) == want      # == on every float
    assert want["hausdorff"] is None and want["forward"]["beyond"] == want["forward"]["count"]


def test_fuse_scene_script_deviation(tmp_path):
    """scripts/fuse_scene.py --smooth_iters 5 --simplify_mm X --deviation on the synthetic DTU-format scene: the `deviation` block
    is mesh_deviation (host) of the mesh the run without the mesh steps wrote against the mesh this run wrote, and it is the
    record's only new key."""
    import sys
    from tests.test_mesh_smooth_gpu import _synthetic_conf
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuse_scene
    common = ["--conf", str(_synthetic_conf(tmp_path)), "--scan", "24", "--ref_views", "1", "2", "--colors", "--logit_override",
              "sphere", "--resolution", "64"]
    state = {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), state)
    v0, t0 = state["vertices"], state["triangles"]
    steps = ["--smooth_iters", "5", "--simplify_mm", repr(3.0 * plain["voxel"])]
    without = fuse_scene.run(fuse_scene.parse_args(common + steps + ["--out_dir", str(tmp_path / "steps")]))
    rec = fuse_scene.run(fuse_scene.parse_args(common + steps + ["--deviation", "--deviation_backend", "device", "--out_dir",
                                                                 str(tmp_path / "deviation")]), state)
    assert "deviation" not in plain and "deviation" not in without and set(rec) - set(without) == {"deviation"}
    want = md.mesh_deviation(v0, t0, state["vertices"], state["triangles"])
    block = rec["deviation"]
    assert set(block) == set(want) | {"max_dist", "ms"} and {k: block[k] for k in want} == want
    assert block["max_dist"] == md.joint_diagonal(np.asarray(v0, np.float32), np.asarray(state["vertices"], np.float32))
    assert block["hausdorff"] > 0 and plain["vertices"] >= block["forward"]["count"] > block["backward"]["count"] > 0
    assert block["forward"]["beyond"] == block["backward"]["beyond"] == 0
    assert json.load(open(tmp_path / "deviation" / "fused_scan24.json"))["deviation"]["hausdorff"] == want["hausdorff"]
    capped = fuse_scene.run(fuse_scene.parse_args(common + steps + ["--deviation", "--deviation_max_mm", repr(0.5 * want["hausdorff"]),
                                                                    "--out_dir", str(tmp_path / "capped")]))
    assert capped["deviation"]["max_dist"] == 0.5 * want["hausdorff"] and capped["deviation"]["forward"]["beyond"] + \
        capped["deviation"]["backward"]["beyond"] > 0
    with pytest.raises(SystemExit, match="--smooth_iters / --simplify_mm"):
        fuse_scene.run(fuse_scene.parse_args(common + ["--deviation", "--out_dir", str(tmp_path / "bad")]))


def test_fuse_scene_script_cloud_mesh_deviation(tmp_path):
    """--cloud_mesh with the mesh steps and --deviation: the `cloud_mesh` block gains `deviation`, mesh_deviation (host) of the
    cloud mesh the run without the steps returned against the one this run returned; nothing else is new."""
    import sys
    from tests.test_mesh_smooth_gpu import _synthetic_conf
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuse_scene
    common = ["--conf", str(_synthetic_conf(tmp_path)), "--scan", "24", "--ref_views", "1", "2", "3", "--resolution", "64",
              "--logit_override", "sphere", "--min_consistent", "1", "--colors", "--point_cloud", "--cloud_normals", "16", "--cloud_mesh"]
    s0, s1 = {}, {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), s0)
    steps = ["--smooth_iters", "3", "--simplify_mm", repr(2.0 * plain["voxel"])]
    without = fuse_scene.run(fuse_scene.parse_args(common + steps + ["--out_dir", str(tmp_path / "steps")]))
    rec = fuse_scene.run(fuse_scene.parse_args(common + steps + ["--deviation", "--deviation_backend", "device", "--out_dir",
                                                                 str(tmp_path / "deviation")]), s1)
    assert set(rec) - set(without) == {"deviation"} and set(rec["cloud_mesh"]) - set(without["cloud_mesh"]) == {"deviation"}
    assert "deviation" not in plain["cloud_mesh"] and len(s0["cloud_mesh"][1]) == len(s1["cloud_mesh_before"][1]) > len(s1["cloud_mesh"][1])
    (va, ta), (vb, tb) = s1["cloud_mesh_before"][:2], s1["cloud_mesh"][:2]                  # before and after the mesh steps
    want = md.mesh_deviation(va, ta, vb, tb)
    block = rec["cloud_mesh"]["deviation"]
    assert set(block) == set(want) | {"max_dist", "ms"} and {k: block[k] for k in want} == want and want["hausdorff"] > 0
    assert rec["deviation"]["hausdorff"] > 0 and rec["deviation"] != block


def test_chamfer_script_deviation(tmp_path):
    """scripts/dtu_chamfer.py --smooth_iters 5 --simplify_cell X --deviation on the synthetic scene (evaluation files as in
    tests/test_mesh_smooth_gpu.py::test_chamfer_script_smooth): `deviation` is mesh_deviation (host) of the mesh before the steps
    against the mesh after them, in the normalised frame, and the record's only new key."""
    import sys
    from scipy.io import savemat
    from tests.test_mesh_smooth_gpu import _synthetic_conf
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    ev = tmp_path / "dtu_eval"
    os.makedirs(ev / "ObsMask")
    os.makedirs(ev / "Points" / "stl")
    g = np.random.default_rng(0)
    d = g.standard_normal((60000, 3))
    stl = d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(80.0, 420.0, (60000, 1))
    with open(ev / "Points" / "stl" / "stl024_total.ply", "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\n"
                  "property float z\nend_header\n").encode())
        fh.write(np.ascontiguousarray(stl, dtype="<f4").tobytes())
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8),
                                                  "BB": np.stack([np.full(3, -800.0), np.full(3, 800.0)]).astype(np.float32),
                                                  "Res": np.float32(1600.0 / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, 801.0]])})
    base = ["--conf", str(_synthetic_conf(tmp_path)), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1",
            "--downsample_density", "4.0", "--logit_override", "sphere", "--mesh_resolution", "64"]
    state = {}
    dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "plain")]), state)
    v0, t0 = state["vertices"], state["triangles"]
    steps = ["--smooth_iters", "5", "--simplify_cell", "0.1"]
    without = dtu_chamfer.run(dtu_chamfer.parse_args(base + steps + ["--out_dir", str(tmp_path / "steps")]))
    rec = dtu_chamfer.run(dtu_chamfer.parse_args(base + steps + ["--deviation", "--deviation_backend", "device", "--out_dir",
                                                                 str(tmp_path / "deviation")]), state)
    assert set(rec) - set(without) == {"deviation"}
    want = md.mesh_deviation(v0, t0, state["vertices"], state["triangles"])
    block = rec["deviation"]
    assert set(block) == set(want) | {"max_dist", "ms"} and {k: block[k] for k in want} == want and want["hausdorff"] > 0
    assert rec["triangles"] < len(t0) and block["forward"]["beyond"] == block["backward"]["beyond"] == 0
    capped = dtu_chamfer.run(dtu_chamfer.parse_args(base + steps + ["--deviation", "--deviation_max_dist", repr(0.5 * want["hausdorff"]),
                                                                    "--out_dir", str(tmp_path / "capped")]))
    assert capped["deviation"]["max_dist"] == 0.5 * want["hausdorff"]
    assert capped["deviation"]["forward"]["beyond"] + capped["deviation"]["backward"]["beyond"] > 0
    with pytest.raises(SystemExit, match="--smooth_iters / --simplify_cell"):
        dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--deviation", "--out_dir", str(tmp_path / "bad")]))


def test_module_command_line(tmp_path, capsys):
    from surf_amd import mesh_io
    from surf_amd.mesh_smooth import smooth_mesh
    v, f = MESHES["noisy_sphere"]
    b = smooth_mesh(v, f, iterations=3)[0]
    mesh_io.write_ply(str(tmp_path / "a.ply"), v, f)
    mesh_io.write_ply(str(tmp_path / "b.ply"), b, f)
    rec = md.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--device", "gpu"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = md.mesh_deviation(v, f, b, f)
    assert {k: line[k] for k in want} == want and {k: rec[k] for k in want} == want
    assert line["max_dist"] == md.joint_diagonal(v, b) and line["vertices"] == [len(v), len(v)] and line["ms"] > 0
    capped = md.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--max_dist", "0.001"])
    assert capped["max_dist"] == 0.001 and capped["forward"]["beyond"] > 0
