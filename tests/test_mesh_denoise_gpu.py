"""The device path of mesh denoising (csrc/mesh_denoise.hip, surf_amd.mesh_denoise backend="device") against the host path, bit for
bit (uint32 views), on the meshes of tests/mesh_denoise_scenes.py: positions, normals, info, the neighbour CSR and the face
records after the normal stage.  Both paths evaluate the one fp64 operation sequence of include/surf_hip.h with sequential sums,
and fp64 division and sqrt round correctly on the device as in numpy.  Nothing here compares the device path with itself, except
one run-twice check that the bits repeat."""
import os

import numpy as np
import pytest
import torch

from surf_amd import _lib
from surf_amd.mesh_denoise import MAX_NEIGHBOURS, denoise_mesh, denoise_mesh_host, face_neighbours_host
from tests.mesh_denoise_scenes import LARGE, SCENES, WAVE_ROW, big_cube, big_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW_SYMBOLS = ["surf_denoise_face_records", "surf_denoise_neighbour_count", "surf_denoise_neighbour_emit",
               "surf_denoise_normal_step", "surf_denoise_vertex_step"]
BIG = {"big_sphere": big_sphere, "big_cube": big_cube}
# (normal, vertex) iterations of the settings matrix, 3 + 3 where nothing is said; big_sphere runs 2 + 2.  The fan alone cannot
# afford three: every one of its 5000 faces has the other 4999 for neighbours, the numpy mirror lists those 25 million pairs,
# and one normal iteration over them takes it seconds per setting with the list itself shared (neighbours()).
ITERATIONS = {"fan": (1, 1), "big_sphere": (2, 2)}
GIVEN_SIGMA_S = {"big_sphere": 0.02, "big_cube": 0.03}
_cache = {}


def mesh(name):
    if name not in _cache:
        _cache[name] = SCENES[name] if name in SCENES else BIG[name]()
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


# The matrix: pin_boundary on and off, with and without the cap, sigma_s absent and given; every scene runs the full product, one
# test per (scene, setting).  The runs without a cap come first: the cap is taken from one of them.
SETTINGS = [(pin, capped, sigma) for capped in (False, True) for pin in (True, False) for sigma in (False, True)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    """Fails on the parent commit: the surf_denoise_* group is new.  The ABI version stays 41 (entry points added, none changed)."""
    with open(os.path.join(ROOT, "include", "surf_hip.h")) as f:
        header = f.read()
    assert "#define SURF_ABI_VERSION 41" in header and _lib.ABI_VERSION == 41
    assert f"#define SURF_DENOISE_WAVE_ROW {WAVE_ROW}\n" in header
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
    assert MAX_NEIGHBOURS == 2 ** 31 - 1 and not hasattr(ops, "MAX_NEIGHBOURS")
    for call in (lambda: L.surf_denoise_face_records(None, big, None, 10, None, None, None),
                 lambda: L.surf_denoise_face_records(None, 10, None, big, None, None, None),
                 lambda: L.surf_denoise_neighbour_count(None, big, 10, None, None, None, None),
                 lambda: L.surf_denoise_neighbour_count(None, 10, big, None, None, None, None),
                 lambda: L.surf_denoise_neighbour_emit(None, big, 10, None, None, None, 10, None, None),
                 lambda: L.surf_denoise_neighbour_emit(None, 10, 10, None, None, None, 2 ** 31, None, None),
                 lambda: L.surf_denoise_normal_step(None, None, big, None, None, 10, 1.0, 1.0, None),
                 lambda: L.surf_denoise_normal_step(None, None, 10, None, None, 2 ** 31, 1.0, 1.0, None),
                 lambda: L.surf_denoise_vertex_step(None, None, big, None, 10, None, None, None, None, 1, None),
                 lambda: L.surf_denoise_vertex_step(None, None, 10, None, big, None, None, None, None, 1, None)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            call()
    for call in (lambda: L.surf_denoise_face_records(None, 10, None, 10, None, None, None),               # null pointers
                 lambda: L.surf_denoise_neighbour_count(None, 10, 10, None, None, None, None),
                 lambda: L.surf_denoise_neighbour_emit(None, 10, 10, None, None, None, 10, None, None),
                 lambda: L.surf_denoise_neighbour_emit(None, 10, 10, None, None, None, -1, None, None),
                 lambda: L.surf_denoise_normal_step(None, None, 10, None, None, 10, 1.0, 1.0, None),
                 lambda: L.surf_denoise_normal_step(None, None, 10, None, None, 10, float("nan"), 1.0, None),
                 lambda: L.surf_denoise_normal_step(None, None, 10, None, None, 10, 1.0, float("inf"), None),
                 lambda: L.surf_denoise_normal_step(None, None, 10, None, None, 10, -1.0, 1.0, None),
                 lambda: L.surf_denoise_vertex_step(None, None, 10, None, 10, None, None, None, None, 1, None)):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            call()
    assert L.surf_denoise_face_records(None, 10, None, 0, None, None, None) == 0                           # empty launches
    assert L.surf_denoise_neighbour_count(None, 0, 10, None, None, None, None) == 0
    assert L.surf_denoise_neighbour_emit(None, 10, 10, None, None, None, 0, None, None) == 0
    assert L.surf_denoise_normal_step(None, None, 0, None, None, 0, 1.0, 1.0, None) == 0
    assert L.surf_denoise_vertex_step(None, None, 0, None, 0, None, None, None, None, 1, None) == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def neighbours(name):
    """face_neighbours_host of a scene, built once: around the fan's hub of 5000 it lists 25 million pairs."""
    if ("neighbours", name) not in _cache:
        v, f = mesh(name)
        _cache["neighbours", name] = face_neighbours_host(f, len(v))
    return _cache["neighbours", name]


def host(name, **kw):
    v, f = mesh(name)
    ni, vi = ITERATIONS.get(name, (3, 3))
    return denoise_mesh_host(v, f, normal_iterations=ni, vertex_iterations=vi, neighbours=neighbours(name), **kw)


def a_cap(name, free_run=None):
    """A cap that some vertices hit and others do not: the median movement of the scene's free run without one, sigma_s absent
    (1e-3 if nothing moves).  That run is a case of the matrix, which hands its result in as free_run."""
    if ("cap", name) not in _cache:
        v, _ = mesh(name)
        moved = (free_run or host(name, pin_boundary=False))[0].astype(np.float64) - v.astype(np.float64)
        _cache["cap", name] = float(np.median(np.linalg.norm(moved, axis=1))) or 1e-3
    return _cache["cap", name]


@pytest.mark.gpu
@pytest.mark.parametrize("pin,capped,sigma", SETTINGS, ids=[f"{'pinned' if p else 'free'}-{'cap' if c else 'nocap'}-"
                                                            f"{'given' if s else 'absent'}" for p, c, s in SETTINGS])
@pytest.mark.parametrize("name", list(SCENES) + list(BIG))
def test_device_equals_host(name, pin, capped, sigma):
    """Vertices, normals and info for every scene under every setting of the matrix, and in the first setting the intermediate
    arrays too: the neighbour CSR and the face records after the normal stage."""
    from surf_amd import ops
    v, f = mesh(name)
    ni, vi = ITERATIONS.get(name, (3, 3))
    given = np.random.default_rng(len(name)).standard_normal(v.shape).astype(np.float32)
    kw = dict(pin_boundary=pin, sigma_s=GIVEN_SIGMA_S.get(name, 0.3) if sigma else None, normals=given if capped else True,
              max_move=a_cap(name) if capped else None)
    first = (pin, capped, sigma) == SETTINGS[0]
    keep_host = {}
    want = host(name, keep=keep_host if first else None, **kw)
    if (pin, capped, sigma) == (False, False, False):
        a_cap(name, free_run=want)
    kw.update(normal_iterations=ni, vertex_iterations=vi)
    if not first:
        got = denoise_mesh(v, f, backend="device", device=DEV, **kw)
    else:
        tv, tf = torch.from_numpy(np.ascontiguousarray(v)).to(DEV), torch.from_numpy(np.ascontiguousarray(f)).to(DEV)
        keep = {}
        got = ops.denoise_mesh(tv, tf, keep=keep, **kw)
        got = (got[0].cpu().numpy(), got[1].cpu().numpy(), got[2])
        rows, nbr, rec = (keep[key].cpu().numpy() for key in ("face_row_start", "face_neighbours", "records"))
        assert rows.dtype == np.int32 and nbr.dtype == np.int32 and rec.shape == (len(f), 8)
        assert np.array_equal(rows, keep_host["face_row_start"]) and np.array_equal(nbr, keep_host["face_neighbours"]), name
        diff = bits(rec[:, :7]) != bits(keep_host["records"][:, :7])
        assert not diff.any(), (name, "records", int(diff.any(axis=1).sum()))
    assert_same(got, want, (name, pin, capped, sigma))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name in SCENES if name not in LARGE])
def test_device_equals_host_defaults_and_empty_stages(name):
    v, f = mesh(name)
    for kw in (dict(), dict(normal_iterations=0, vertex_iterations=0), dict(normal_iterations=0, vertex_iterations=3),
               dict(normal_iterations=3, vertex_iterations=0, normals=True)):
        want = denoise_mesh(v, f, **kw)
        assert_same(denoise_mesh(v, f, backend="device", device=DEV, **kw), want, (name, kw))
    print(f"{name}: {len(v)} vertices, {len(f)} faces")


@pytest.mark.gpu
def test_the_cap_is_hit_and_missed():
    v, f = mesh("noisy_cube8")
    info = denoise_mesh(v, f, max_move=0.02, backend="device", device=DEV)[2]
    assert 0 < info["capped"] < len(v)


@pytest.mark.gpu
def test_the_bits_repeat():
    v, f = mesh("big_cube")
    a = denoise_mesh(v, f, normal_iterations=3, vertex_iterations=3, normals=True, max_move=2e-3, backend="device", device=DEV)
    b = denoise_mesh(v, f, normal_iterations=3, vertex_iterations=3, normals=True, max_move=2e-3, backend="device", device=DEV)
    assert_same(a, b, "second run")
    hv, hf = mesh("fan200")
    a = denoise_mesh(hv, hf, pin_boundary=False, normals=True, backend="device", device=DEV)
    b = denoise_mesh(hv, hf, pin_boundary=False, normals=True, backend="device", device=DEV)
    assert_same(a, b, "second run, hub")


@pytest.mark.gpu
def test_tensors_stay_on_the_device_and_refusals():
    from surf_amd import ops
    v, f = mesh("noisy_cube8")
    want = denoise_mesh(v, f, normals=True, max_move=0.01)
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    got = denoise_mesh(tv, tf, normals=True, max_move=0.01, backend="device", device=DEV, return_tensors=True)
    assert torch.is_tensor(got[0]) and got[0].is_cuda and got[1].is_cuda and ops.DENOISE_HOST_READS == 3
    assert_same((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2]), want, "tensors")
    assert np.array_equal(bits(tv.cpu().numpy()), bits(v)) and np.array_equal(tf.cpu().numpy(), f)     # inputs untouched
    torch.cuda.set_sync_debug_mode("error")                            # an empty face list reads nothing and returns the input
    try:
        e = denoise_mesh(tv, tf[:0], backend="device", device=DEV, return_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert e[0].data_ptr() == tv.data_ptr() and e[1] is None and e[2]["faces"] == 0
    with pytest.raises(RuntimeError, match="no host fall-back"):
        denoise_mesh(v, f, backend="device", device="cpu")
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="denoise_mesh: vertex 2 is not finite"):
            denoise_mesh(bad, f, backend="device", device=DEV)
    with pytest.raises(ValueError, match=r"face indices span \[0, 1000\]"):
        denoise_mesh(v, np.array([[0, 1, 1000]], np.int32), backend="device", device=DEV)
    with pytest.raises(ValueError, match="mean side length.*0.0"):
        denoise_mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32), backend="device", device=DEV)
    with pytest.raises(ValueError, match="sigma_r"):
        denoise_mesh(v, f, sigma_r=0.0, backend="device", device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_extract_mesh_denoise(sparse):
    """extract_mesh(denoise={}) of a fused synthetic sphere, device and host backends: denoise_mesh of extract_mesh()'s arrays;
    with smooth and simplify_cell too, denoise, then smooth, then simplify; with denoise=None the arrays of the call without it."""
    from surf_amd.fusion import FusionVolume
    from surf_amd.mesh_simplify import simplify_mesh
    from surf_amd.mesh_smooth import smooth_mesh
    from tests.test_fusion_sparse_host import sphere_scene
    axes, views, trunc = sphere_scene()
    cell = 3.0 / 128
    for backend in ("device", "host"):
        vol = FusionVolume(axes, trunc=trunc, colors=True, backend=backend, device=DEV, sparse=sparse)
        vol.integrate(views)
        v, t, c = vol.extract_mesh()
        assert len(t) > 1000
        none = vol.extract_mesh(denoise=None)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(none, (v, t, c)))
        want_v, _, info = denoise_mesh(v, t)
        assert info["moved_max"] > 0
        got = vol.extract_mesh(denoise={})
        assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.uint8
        assert np.array_equal(got[0], want_v.astype(np.float64)) and np.array_equal(got[1], t) and np.array_equal(got[2], c)
        params = {"normal_iterations": 3, "vertex_iterations": 4, "max_move": 0.02}
        step1 = denoise_mesh(v, t, **params)[0]
        step2 = smooth_mesh(step1, t, iterations=2)[0]
        want = simplify_mesh(step2, t, cell, colors=c)
        all3 = vol.extract_mesh(simplify_cell=cell, smooth={"iterations": 2}, denoise=params)
        assert np.array_equal(all3[0], want[0].astype(np.float64)) and np.array_equal(all3[1], want[1]) and np.array_equal(all3[2], want[2])
        with pytest.raises(ValueError, match="unknown key"):
            vol.extract_mesh(denoise={"iterations": 3})
