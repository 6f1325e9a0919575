"""The device path of mesh simplification (csrc/mesh_simplify.hip, surf_amd.mesh_simplify backend="device") against the host
path, array for array, on the meshes of tests/test_mesh_simplify_host.py.  Integer arrays are equal and positions and normals are
BIT-equal: both paths evaluate the one fp64 operation sequence of include/surf_hip.h with sequential per-cell sums, and fp64
division and sqrt round correctly on the device as in numpy.  Nothing here compares the device path with itself, except one
run-twice check that the bits repeat."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from surf_amd import _lib
from surf_amd.mesh_simplify import simplify_mesh
from tests.test_mesh_simplify_host import CASES, attributes, uv_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW_SYMBOLS = ["surf_simplify_keys", "surf_simplify_segments", "surf_simplify_face_cells", "surf_simplify_faces",
               "surf_simplify_mark_used", "surf_simplify_cells", "surf_simplify_compact"]
NAMES = ("vertices", "faces", "normals", "colors", "vertex_map")


def crowded_cell():
    """A sphere of 10 272 vertices inside the cell [0, 1)^3 and two fans that tie it to vertices in eight other cells: one USED
    cell whose vertex segment has more than 10^4 members and whose corner segment has more than 6 10^4."""
    v, f = uv_sphere(80, 130, 0.4, (0.5, 0.5, 0.5))
    far = np.array([(x, y, z) for x in (-0.5, 1.5) for y in (-0.5, 1.5) for z in (-0.5, 1.5)], np.float32)
    n = len(v)
    ties = [(7 * k, n + k, n + (k + 1) % 8) for k in range(8)] + [(n + k, 11 * k + 1, n + (k + 3) % 8) for k in range(8)]
    return np.concatenate([v, far]), np.concatenate([f[:5000], np.asarray(ties, np.int32), f[5000:]]), 1.0


def big_sphere():
    """About 300 k faces: 1176 blocks of 256 faces, several rounds of workgroups on the device."""
    v, f = uv_sphere(388, 388)
    return v, f, 0.02


BIG = {"crowded": crowded_cell, "big_sphere": big_sphere}


def mesh(name):
    return CASES[name] if name in CASES else BIG[name]()


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype == np.float32:           # bit equality, not ==: -0 and +0 differ, a NaN equals itself
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (what, name, int((a != b).sum()))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    """Fails on the parent commit: the surf_simplify_* group is new.  The ABI version stays 41 (entry points added, none changed)."""
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
    L = _lib.lib()
    big = 1 << 31
    for call in (lambda: L.surf_simplify_keys(None, big, 1.0, None, None, None),
                 lambda: L.surf_simplify_segments(None, None, None, big, 1, None, None, None),
                 lambda: L.surf_simplify_face_cells(None, big, None, 10, None, None, None),
                 lambda: L.surf_simplify_faces(None, big, None, 1024, None, None, None),
                 lambda: L.surf_simplify_mark_used(None, None, big, 10, None, None),
                 lambda: L.surf_simplify_cells(None, None, None, big, None, 10, 1.0, None, None, None, None, None, 1, None, None, None,
                                               None, None, None),
                 lambda: L.surf_simplify_compact(None, None, None, big, None, 10, None, None, 1, None, None, None)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            call()
    for cell in (0.0, -1.0, float("nan"), 1e-200, 1e200):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            L.surf_simplify_keys(None, 10, cell, None, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid argument"):
        L.surf_simplify_faces(None, 1000, None, 1024, None, None, None)           # 2048 slots are wanted
    assert L.surf_simplify_keys(None, 0, 1.0, None, None, None) == 0               # empty launches return at once
    assert L.surf_simplify_faces(None, 0, None, 0, None, None, None) == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + list(BIG))
def test_device_equals_host(name):
    v, f, cell = mesh(name)
    nrm, col = attributes(v, len(name))
    want = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True)
    got = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True, backend="device", device=DEV)
    print(f"{name}: {len(f)} -> {len(want[1])} faces, {len(v)} -> {len(want[0])} vertices")
    assert_same(got, want, name)
    if name == "crowded":
        assert np.bincount(want[4][want[4] >= 0]).max() > 10 ** 4
    # without attributes (the kernel's other branches), and with each alone
    bare = simplify_mesh(v, f, cell, return_map=True, backend="device", device=DEV)
    assert_same(bare, (want[0], want[1], want[4]), name + " bare")
    only_n = simplify_mesh(v, f, cell, normals=nrm, backend="device", device=DEV)
    only_c = simplify_mesh(v, f, cell, colors=col, backend="device", device=DEV)
    assert_same(only_n, want[:3], name + " normals")
    assert_same(only_c, (want[0], want[1], want[3]), name + " colors")


@pytest.mark.gpu
def test_the_bits_repeat():
    v, f, cell = mesh("crowded")
    nrm, col = attributes(v, 1)
    a = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True, backend="device", device=DEV)
    b = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True, backend="device", device=DEV)
    assert_same(a, b, "second run")


@pytest.mark.gpu
def test_tensors_stay_on_the_device():
    """return_tensors=True: device tensors in, device tensors out, and exactly ops.SIMPLIFY_HOST_READS = 2 reads of the device on
    the way - [cells, limit flag, face index range] and [kept faces, used cells], the sizes the next allocations need."""
    from surf_amd import ops
    v, f, cell = CASES["sphere"]
    nrm, col = attributes(v, 2)
    want = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True)
    tv, tf, tn, tc = (torch.from_numpy(x).to(DEV) for x in (v, f, nrm, col))
    simplify_mesh(tv, tf, cell, normals=tn, colors=tc, backend="device", device=DEV, return_tensors=True)      # warm the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = simplify_mesh(tv, tf, cell, normals=tn, colors=tc, backend="device", device=DEV, return_tensors=True, return_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchron" in str(w.message).lower()]
    for w in syncs:
        print(f"{os.path.relpath(w.filename, ROOT)}:{w.lineno}: {w.message}")
    assert ops.SIMPLIFY_HOST_READS == 2 and len(syncs) == ops.SIMPLIFY_HOST_READS
    assert all(torch.is_tensor(t) and t.is_cuda for t in got)
    assert_same([t.cpu().numpy() for t in got], want, "tensors")
    # an empty face list reads nothing
    torch.cuda.set_sync_debug_mode("error")
    try:
        e = simplify_mesh(tv, tf[:0], cell, backend="device", device=DEV, return_tensors=True, return_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and bool((e[2] == -1).all())
    with pytest.raises(RuntimeError, match="no host fall-back"):
        simplify_mesh(v, f, cell, backend="device", device="cpu")


@pytest.mark.gpu
def test_device_limits_raise_like_the_host_path():
    v, f, cell = CASES["fine"]
    for bad_value in (np.nan, np.inf, 0.03 * 2 ** 20):
        bad = v.copy()
        bad[3, 1] = bad_value
        with pytest.raises(ValueError, match="not finite or lies outside"):
            simplify_mesh(bad, f, cell, backend="device", device=DEV)
    with pytest.raises(ValueError, match="face indices"):
        simplify_mesh(v, np.array([[0, 1, len(v)]], np.int32), cell, backend="device", device=DEV)
    with pytest.raises(ValueError, match="cell"):
        simplify_mesh(v, f, 0.0, backend="device", device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_extract_mesh_simplify_cell_device_backend(sparse):
    """A device-backend volume simplifies on the device and equals the host path applied to its own unsimplified mesh."""
    from surf_amd.fusion import FusionVolume
    from tests.test_fusion_sparse_host import sphere_scene
    axes, views, trunc = sphere_scene()
    vol = FusionVolume(axes, trunc=trunc, colors=True, backend="device", device=DEV, sparse=sparse)
    vol.integrate(views)
    v, t, c = vol.extract_mesh()
    cell = 3.0 / 128
    want = simplify_mesh(v, t, cell, colors=c)
    got = vol.extract_mesh(simplify_cell=cell)
    print(f"{len(t)} -> {len(got[1])} faces")
    assert 100 < len(got[1]) < len(t) // 3
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.uint8
    assert np.array_equal(got[0], want[0].astype(np.float64)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    bare = FusionVolume(axes, trunc=trunc, colors=False, backend="device", device=DEV, sparse=sparse)
    bare.integrate([x._replace(image=None) for x in views])
    got2 = bare.extract_mesh(simplify_cell=cell)
    assert len(got2) == 2 and np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])


@pytest.mark.gpu
def test_fuse_scene_script_simplify(tmp_path):
    """scripts/fuse_scene.py --simplify_mm on the synthetic DTU-format scene of tests/test_fusion_gpu.py::test_fuse_scene_script:
    a smaller PLY that holds the host path's simplification of the mesh the run without the flag wrote, and the `simplify` block
    as the record's only new key."""
    from bench import surf_conf
    from surf_amd import mesh_io
    from tests.test_end_to_end_dtu import _write_scene
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuse_scene
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--colors", "--logit_override", "sphere",
              "--resolution", "64"]
    state = {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), state)
    assert "simplify" not in plain and plain["triangles"] > 100
    cell = 3.0 * plain["voxel"]
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--simplify_mm", repr(cell), "--simplify_backend", "device",
                                                         "--out_dir", str(tmp_path / "simple")]))
    assert set(rec) - set(plain) == {"simplify"} and set(rec["ms"]) == set(plain["ms"])
    block = rec["simplify"]
    assert set(block) == {"cell", "vertices_in", "faces_in", "vertices_out", "faces_out", "ms"} and block["cell"] == cell
    assert (block["vertices_in"], block["faces_in"]) == (plain["vertices"], plain["triangles"])
    assert (block["vertices_out"], block["faces_out"]) == (rec["vertices"], rec["triangles"]) and 0 < rec["triangles"] < plain["triangles"] // 3
    assert os.path.getsize(rec["mesh"]) < os.path.getsize(plain["mesh"]) // 3
    assert json.load(open(tmp_path / "simple" / "fused_scan24.json"))["simplify"]["faces_out"] == block["faces_out"]
    want = simplify_mesh(state["vertices"], state["triangles"], cell, colors=state["colors"])
    v, t, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert np.array_equal(v.astype(np.float32), want[0]) and np.array_equal(t, want[1]) and np.array_equal(attrs["colors"], want[2])


@pytest.mark.gpu
def test_chamfer_script_simplify(tmp_path):
    """scripts/dtu_chamfer.py --simplify_cell on the synthetic DTU-format scene, evaluation files as in
    tests/test_clean_dtu_gpu.py::test_chamfer_script_with_the_protocol_cleaner: the evaluator scores the smaller mesh that was
    written, normals and colours follow the vertices, and `simplify` is the record's only new key."""
    from scipy.io import savemat
    from bench import surf_conf
    from surf_amd import mesh_io
    from tests.test_end_to_end_dtu import _write_scene
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
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
    base = ["--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--downsample_density", "4.0",
            "--logit_override", "sphere", "--mesh_resolution", "64", "--vertex_colors"]
    state = {}
    plain = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "plain")]), state)
    full_v, full_t = state["vertices"], state["triangles"]
    rec = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "simple"), "--simplify_cell", "0.1",
                                                         "--simplify_backend", "device"]), state)
    assert "simplify" not in plain and set(rec) - set(plain) == {"simplify"}
    block = rec["simplify"]
    assert (block["vertices_in"], block["faces_in"]) == (plain["vertices"], plain["triangles"]) == (len(full_v), len(full_t))
    assert (block["vertices_out"], block["faces_out"]) == (rec["vertices"], rec["triangles"]) and 0 < rec["triangles"] < plain["triangles"] // 2
    assert os.path.getsize(rec["mesh"]) < os.path.getsize(plain["mesh"]) // 2 and np.isfinite(rec["chamfer"])
    want_v, want_t = simplify_mesh(full_v, full_t, 0.1)
    assert np.array_equal(state["vertices"], want_v) and np.array_equal(state["triangles"], want_t)
    v, t, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert len(v) == rec["vertices"] and np.array_equal(t, want_t) and attrs["normals"].shape == v.shape and attrs["colors"].shape == v.shape
    assert np.allclose(np.linalg.norm(attrs["normals"].astype(np.float64), axis=1), 1.0, atol=1e-5)
