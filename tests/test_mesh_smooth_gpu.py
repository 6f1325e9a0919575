"""The device path of mesh smoothing (csrc/mesh_smooth.hip, surf_amd.mesh_smooth backend="device") against the host path, bit
for bit (uint32 views), on the meshes of tests/mesh_smooth_scenes.py: positions, normals, boundary flags and info, for both
schedules, pinned and free, with and without the cap.  Both paths evaluate the one fp64 operation sequence of include/surf_hip.h
with sequential per-vertex sums, and fp64 division and sqrt round correctly on the device as in numpy.  Nothing here compares the
device path with itself, except one run-twice check that the bits repeat."""
import os
import warnings

import numpy as np
import pytest
import torch

from surf_amd import _lib
from surf_amd.mesh_smooth import boundary_flags, smooth_mesh
from tests.mesh_smooth_scenes import MESHES, big_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW_SYMBOLS = ["surf_smooth_edge_keys", "surf_smooth_adjacency", "surf_smooth_step", "surf_smooth_cap", "surf_smooth_sum256",
               "surf_smooth_normals"]
SCHEDULES = {"laplacian": dict(lam=0.5, mu=None), "taubin": dict(lam=0.5, mu=-0.53)}
BIG = {"big_sphere": big_sphere}
_cache = {}


def mesh(name):
    if name not in _cache:
        _cache[name] = MESHES[name] if name in MESHES else BIG[name]()
    return _cache[name]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    (gv, gn, gi), (wv, wn, wi) = got, want
    assert gv.dtype == np.float32 and gv.shape == wv.shape, what
    assert np.array_equal(bits(gv), bits(wv)), (what, "vertices", int((bits(gv) != bits(wv)).any(axis=1).sum()))
    assert (gn is None) == (wn is None), what
    if wn is not None:
        assert gn.dtype == np.float32 and np.array_equal(bits(gn), bits(wn)), (what, "normals", int((bits(gn) != bits(wn)).any(axis=1).sum()))
    assert gi == wi, (what, gi, wi)                 # the floats of info compare with ==: the same bits


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    """Fails on the parent commit: the surf_smooth_* group is new.  The ABI version stays 41 (entry points added, none changed)."""
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
    big = ops.SMOOTH_MAX_ITEMS + 1
    assert ops.SMOOTH_MAX_ITEMS == (2 ** 31 - 1) // 6
    for call in (lambda: L.surf_smooth_edge_keys(None, big, 10, None, None, None),
                 lambda: L.surf_smooth_edge_keys(None, 10, big, None, None, None),
                 lambda: L.surf_smooth_adjacency(None, None, big, 10, 0, None, None, None),
                 lambda: L.surf_smooth_step(None, None, big, None, None, 10, None, 1, 0.5, None),
                 lambda: L.surf_smooth_cap(None, None, big, 0.0, None, None, None, None),
                 lambda: L.surf_smooth_sum256(None, big, None, None),
                 lambda: L.surf_smooth_normals(None, big, None, 10, None, None, None, None, None, None),
                 lambda: L.surf_smooth_normals(None, 10, None, big, None, None, None, None, None, None)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            call()
    for call in (lambda: L.surf_smooth_edge_keys(None, 10, 10, None, None, None),                      # null pointers
                 lambda: L.surf_smooth_adjacency(None, None, 10, 10, 61, None, None, None),            # nnz > 6 m
                 lambda: L.surf_smooth_step(None, None, 10, None, None, 10, None, 1, float("nan"), None),
                 lambda: L.surf_smooth_step(None, None, 10, None, None, 10, None, 1, 0.5, None),
                 lambda: L.surf_smooth_cap(None, None, 10, float("inf"), None, None, None, None),
                 lambda: L.surf_smooth_cap(None, None, 10, 1e200, None, None, None, None),
                 lambda: L.surf_smooth_sum256(None, 10, None, None),
                 lambda: L.surf_smooth_normals(None, 10, None, 10, None, None, None, None, None, None)):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            call()
    assert L.surf_smooth_edge_keys(None, 0, 10, None, None, None) == 0                                 # empty launches return at once
    assert L.surf_smooth_step(None, None, 0, None, None, 0, None, 1, 0.5, None) == 0
    assert L.surf_smooth_cap(None, None, 0, 0.0, None, None, None, None) == 0
    assert L.surf_smooth_sum256(None, 0, None, None) == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MESHES) + list(BIG))
def test_device_equals_host(name):
    v, f = mesh(name)
    g = np.random.default_rng(len(name))
    given = g.standard_normal(v.shape).astype(np.float32)
    assert np.array_equal(boundary_flags(f, len(v), backend="device", device=DEV), boundary_flags(f, len(v))), name
    # a cap that some vertices hit and others do not: the median movement of the uncapped free Taubin run
    ref = smooth_mesh(v, f, iterations=3, pin_boundary=False)
    cap = float(np.median(np.linalg.norm(ref[0].astype(np.float64) - v.astype(np.float64), axis=1))) or 1e-3
    for kind, sched in SCHEDULES.items():
        for pin in (True, False):
            for max_move in (None, cap):
                for normals in (True, given):
                    kw = dict(iterations=3, pin_boundary=pin, max_move=max_move, normals=normals, **sched)
                    want = smooth_mesh(v, f, **kw)
                    got = smooth_mesh(v, f, backend="device", device=DEV, **kw)
                    assert_same(got, want, (name, kind, pin, max_move, normals is True))
    want = smooth_mesh(v, f)
    print(f"{name}: {len(v)} vertices, {len(f)} faces, {want[2]}")
    assert_same(smooth_mesh(v, f, backend="device", device=DEV), want, name + " defaults")
    assert_same(smooth_mesh(v, f, iterations=0, backend="device", device=DEV), smooth_mesh(v, f, iterations=0), name + " zero")


@pytest.mark.gpu
def test_the_cap_is_hit_and_missed():
    v, f = mesh("noisy_sphere")
    info = smooth_mesh(v, f, lam=0.5, mu=None, max_move=0.004, backend="device", device=DEV)[2]
    assert 0 < info["capped"] < len(v)


@pytest.mark.gpu
def test_the_bits_repeat():
    v, f = mesh("big_sphere")
    a = smooth_mesh(v, f, iterations=3, normals=True, max_move=2e-4, backend="device", device=DEV)
    b = smooth_mesh(v, f, iterations=3, normals=True, max_move=2e-4, backend="device", device=DEV)
    assert_same(a, b, "second run")
    hv, hf = mesh("fan")
    a = smooth_mesh(hv, hf, pin_boundary=False, normals=True, backend="device", device=DEV)
    b = smooth_mesh(hv, hf, pin_boundary=False, normals=True, backend="device", device=DEV)
    assert_same(a, b, "second run, hub")


@pytest.mark.gpu
def test_tensors_stay_on_the_device():
    """return_tensors=True: device tensors in, device tensors out, and exactly ops.SMOOTH_HOST_READS = 2 reads of the device on the
    way - [neighbour entries, face index range, vertices finite] and the five numbers of info."""
    from surf_amd import ops
    v, f = mesh("noisy_sphere")
    want = smooth_mesh(v, f, normals=True, max_move=0.01)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    smooth_mesh(tv, tf, normals=True, max_move=0.01, backend="device", device=DEV, return_tensors=True)      # warm the allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = smooth_mesh(tv, tf, normals=True, max_move=0.01, backend="device", device=DEV, return_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchron" in str(w.message).lower()]
    for w in syncs:
        print(f"{os.path.relpath(w.filename, ROOT)}:{w.lineno}: {w.message}")
    assert ops.SMOOTH_HOST_READS == 2 and len(syncs) == ops.SMOOTH_HOST_READS
    assert torch.is_tensor(got[0]) and got[0].is_cuda and got[1].is_cuda
    assert_same((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2]), want, "tensors")
    assert np.array_equal(bits(tv.cpu().numpy()), bits(v)) and np.array_equal(tf.cpu().numpy(), f)     # inputs untouched
    # an empty face list reads nothing and returns the input
    torch.cuda.set_sync_debug_mode("error")
    try:
        e = smooth_mesh(tv, tf[:0], backend="device", device=DEV, return_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert e[0].data_ptr() == tv.data_ptr() and e[1] is None and e[2]["isolated_vertices"] == len(v)
    with pytest.raises(RuntimeError, match="no host fall-back"):
        smooth_mesh(v, f, backend="device", device="cpu")


@pytest.mark.gpu
def test_device_refusals_raise_like_the_host_path():
    v, f = mesh("two_triangles")
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="vertex 2 is not finite"):
            smooth_mesh(bad, f, backend="device", device=DEV)
    with pytest.raises(ValueError, match=r"face indices span \[0, 4\]"):
        smooth_mesh(v, np.array([[0, 1, 4]], np.int32), backend="device", device=DEV)
    with pytest.raises(ValueError, match=r"face indices span \[-1, 2\]"):
        smooth_mesh(v, np.array([[0, -1, 2]], np.int32), backend="device", device=DEV)
    with pytest.raises(ValueError, match="mu"):
        smooth_mesh(v, f, mu=-0.1, backend="device", device=DEV)
    with pytest.raises(ValueError, match="iterations"):
        smooth_mesh(v, f, iterations=10001, backend="device", device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_extract_mesh_smooth(sparse):
    """extract_mesh(smooth=...) of a fused synthetic sphere, device and host backends: smooth_mesh of extract_mesh()'s arrays;
    with simplify_cell too, smooth then simplify; with smooth=None the arrays of the call without the argument."""
    from surf_amd.fusion import FusionVolume
    from surf_amd.mesh_simplify import simplify_mesh
    from tests.test_fusion_sparse_host import sphere_scene
    axes, views, trunc = sphere_scene()
    params = {"iterations": 4, "max_move": 0.02}
    cell = 3.0 / 128
    for backend in ("device", "host"):
        vol = FusionVolume(axes, trunc=trunc, colors=True, backend=backend, device=DEV, sparse=sparse)
        vol.integrate(views)
        v, t, c = vol.extract_mesh()
        assert len(t) > 1000
        none = vol.extract_mesh(smooth=None)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(none, (v, t, c)))
        want_v, _, info = smooth_mesh(v, t, **params)
        assert info["moved_max"] > 0
        got = vol.extract_mesh(smooth=params)
        assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.uint8
        assert np.array_equal(got[0], want_v.astype(np.float64)) and np.array_equal(got[1], t) and np.array_equal(got[2], c)
        want = simplify_mesh(want_v, t, cell, colors=c)
        both = vol.extract_mesh(simplify_cell=cell, smooth=params)
        assert 100 < len(both[1]) < len(t) // 3
        assert np.array_equal(both[0], want[0].astype(np.float64)) and np.array_equal(both[1], want[1]) and np.array_equal(both[2], want[2])
        with pytest.raises(ValueError, match="unknown key"):
            vol.extract_mesh(smooth={"iters": 3})


def _synthetic_conf(tmp_path):
    """The synthetic DTU-format scene and conf of tests/test_mesh_simplify_gpu.py::test_fuse_scene_script_simplify."""
    import json
    from bench import surf_conf
    from tests.test_end_to_end_dtu import _write_scene
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    return conf_path


@pytest.mark.gpu
def test_fuse_scene_script_smooth(tmp_path):
    """scripts/fuse_scene.py --smooth_iters 10 on the synthetic DTU-format scene: a PLY of the same faces and colours whose
    positions are the host path's smoothing of the mesh the run without the flag wrote, `smooth` as the record's only new key,
    and with --simplify_mm too the simplification of the smoothed mesh."""
    import json
    import sys
    from surf_amd import mesh_io
    from surf_amd.mesh_simplify import simplify_mesh
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuse_scene
    common = ["--conf", str(_synthetic_conf(tmp_path)), "--scan", "24", "--ref_views", "1", "2", "--colors", "--logit_override",
              "sphere", "--resolution", "64"]
    state = {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), state)
    assert "smooth" not in plain and plain["triangles"] > 100
    v0, t0, c0 = state["vertices"], state["triangles"], state["colors"]
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--smooth_iters", "10", "--smooth_backend", "device",
                                                         "--out_dir", str(tmp_path / "smooth")]))
    assert set(rec) - set(plain) == {"smooth"} and set(rec["ms"]) == set(plain["ms"])
    block = rec["smooth"]
    want_v, _, info = smooth_mesh(v0, t0)
    assert set(block) == {"iterations", "lam", "mu", "pin_boundary", "max_move", "ms"} | set(info)
    assert {k: block[k] for k in info} == info and info["moved_max"] > 0
    assert (block["iterations"], block["lam"], block["mu"], block["pin_boundary"], block["max_move"]) == (10, 0.5, -0.53, True, None)
    assert (rec["vertices"], rec["triangles"]) == (plain["vertices"], plain["triangles"])
    assert json.load(open(tmp_path / "smooth" / "fused_scan24.json"))["smooth"]["moved_rms"] == info["moved_rms"]
    v, t, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert np.array_equal(bits(v), bits(want_v)) and np.array_equal(t, t0) and np.array_equal(attrs["colors"], c0)
    # Laplacian, capped, free boundary, host backend, then simplified
    cell = 3.0 * plain["voxel"]
    rec2 = fuse_scene.run(fuse_scene.parse_args(common + ["--smooth_iters", "3", "--smooth_laplacian", "--smooth_lambda", "0.25",
                                                          "--smooth_max_move_mm", repr(0.5 * plain["voxel"]), "--smooth_free_boundary",
                                                          "--simplify_mm", repr(cell), "--out_dir", str(tmp_path / "both")]), state)
    assert set(rec2) - set(plain) == {"smooth", "simplify"} and rec2["smooth"]["mu"] is None and not rec2["smooth"]["pin_boundary"]
    sv = smooth_mesh(v0, t0, iterations=3, lam=0.25, mu=None, pin_boundary=False, max_move=0.5 * plain["voxel"])[0]
    want = simplify_mesh(sv, t0, cell, colors=c0)
    assert np.array_equal(bits(state["vertices"]), bits(want[0])) and np.array_equal(state["triangles"], want[1])
    with pytest.raises(SystemExit, match="mu"):
        fuse_scene.run(fuse_scene.parse_args(common + ["--smooth_iters", "3", "--smooth_mu", "-0.1", "--out_dir", str(tmp_path / "bad")]))


@pytest.mark.gpu
def test_chamfer_script_smooth(tmp_path):
    """scripts/dtu_chamfer.py --smooth_iters with --vertex_colors on the synthetic scene (evaluation files as in
    tests/test_mesh_simplify_gpu.py::test_chamfer_script_simplify): the evaluator scores the smoothed mesh, the normals are the
    rule's, recomputed on the side of the ones they replace, and `smooth` is the record's only new key."""
    import sys
    from scipy.io import savemat
    from surf_amd import mesh_io
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
            "--downsample_density", "4.0", "--logit_override", "sphere", "--mesh_resolution", "64", "--vertex_colors"]
    state = {}
    plain = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "plain")]), state)
    v0, t0 = state["vertices"], state["triangles"]
    n0 = state["model"].vertex_attributes(v0)["normals"]
    rec = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "smooth"), "--smooth_iters", "5",
                                                         "--smooth_max_move", "0.05", "--smooth_backend", "device"]), state)
    assert "smooth" not in plain and set(rec) - set(plain) == {"smooth"} and np.isfinite(rec["chamfer"])
    want_v, want_n, info = smooth_mesh(v0, t0, iterations=5, max_move=0.05, normals=n0)
    assert {k: rec["smooth"][k] for k in info} == info and info["moved_max"] > 0 and rec["smooth"]["max_move"] == 0.05
    assert np.array_equal(bits(state["vertices"]), bits(want_v)) and np.array_equal(state["triangles"], t0)
    assert (rec["vertices"], rec["triangles"]) == (plain["vertices"], plain["triangles"])
    v, t, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert np.array_equal(t, t0) and attrs["colors"].shape == v.shape
    # the file's normals are want_n taken to the world frame; the rule's normals agree with the ones they replace in direction
    unit = np.linalg.norm(attrs["normals"].astype(np.float64), axis=1)
    assert np.allclose(unit[unit > 0], 1.0, atol=1e-5)
    both = (np.linalg.norm(want_n, axis=1) > 0) & (np.linalg.norm(n0, axis=1) > 0)
    assert (np.einsum("ij,ij->i", want_n[both].astype(np.float64), n0[both].astype(np.float64)) >= 0).all()
