"""The device path of the DTU protocol's mesh cleaner (csrc/dtu_clean.hip, surf_amd.evaluation.clean_dtu backend="device")
against the host path, stage by stage, and against the reference's recorded results (tests/golden/clean_dtu.npz).  Nothing here
compares the device path with itself.

Host and device evaluate the same float64 operations in the same order (IEEE multiply, add, divide, rint; no contraction on
either side), so device counts must equal the host's for EVERY vertex: no band.  Only the comparison with the reference, whose
np.matmul has no defined summation order, leaves out the vertices within 1e-6 px of a rounding tie (at most 0.1 %; see
tests/test_clean_dtu_host.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import _lib, ops
from surf_amd.evaluation import clean_dtu as D
from tests import test_clean_dtu_host as HT
from tests.golden import dtu_test_scene as S
from tests.golden.dtu_scene import write_cam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["surf_dtu_clean_dilate", "surf_dtu_clean_points_in_masks", "surf_dtu_clean_keep"]


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _small_views(nv, h=37, w=53):
    """float32 K4 @ E of nv ring cameras whose images are h x w, and grey uint8 masks."""
    K4 = np.eye(4, dtype=np.float32)
    K4[0, 0] = K4[1, 1] = 60.0
    K4[0, 2], K4[1, 2] = 26.3, 18.1
    P_list = [K4 @ E.astype(np.float32) for E in S.ring_cams(nv)]
    g = np.random.default_rng(nv)
    masks = []
    for i in range(nv):
        m = np.where(g.random((h, w)) < 0.4, g.integers(100, 256, (h, w)), 0).astype(np.uint8)
        m[:: 5 + i] = 128                                    # the threshold is > 128: these rows are unset
        masks.append(m)
    return P_list, masks


def _points(n, seed):
    """World-mm points around the object, a share far off the images, behind the cameras and at a camera centre's depth."""
    g = np.random.default_rng(seed)
    p = g.standard_normal((n, 3)) * 120.0
    far = g.random(n) < 0.2
    p[far] *= 8.0
    return p


def test_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "surf_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert f" {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name


@pytest.mark.parametrize("k", [1, 3, 11])
def test_dilation_equals_the_host(k):
    for h, w in ((37, 53), (64, 64)):
        base = HT.dilation_masks(h, w, seed=k)
        for nv in (1, 4):
            stack = np.stack([base[i % 3] for i in range(nv)]) if nv > 1 else base[0][None]
            got = _np(D.dilate_ellipse_device(stack, k))
            assert got.dtype == np.uint8 and got.shape == stack.shape
            for i in range(nv):
                assert np.array_equal(got[i], D.dilate_ellipse(stack[i], k)), (k, h, w, nv, i)
        for m in base[1:]:                                   # all-zero and all-set, as a single (h, w) mask
            assert np.array_equal(_np(D.dilate_ellipse_device(m, k)), m)


@pytest.mark.parametrize("n", [1, 63, 1000, 4097])
def test_counts_equal_the_host_for_every_vertex(n):
    for nv in (1, 2, 3, 4):
        P_list, masks = _small_views(nv)
        p = _points(n, 10 * n + nv)
        for dilate in (11, None):
            host = D.points_in_masks(p, P_list, masks, dilate)
            dev = _np(D.points_in_masks_device(p, P_list, masks, dilate))
            assert dev.dtype == np.int32 and np.array_equal(dev, host), (n, nv, dilate, int((dev != host).sum()))
        if n >= 1000:
            assert 0 < host.max() <= nv and (host == 0).any()


def test_constructed_cases_on_the_device():
    pts, P_list, masks, want = HT.constructed_cases()
    got = _np(D.points_in_masks_device(pts, P_list, masks, None))
    assert got.tolist() == want.tolist(), [(p, int(a), int(b)) for p, a, b in zip(pts.tolist(), got, want) if a != b]
    assert np.array_equal(got, D.points_in_masks(pts, P_list, masks, None))
    full = np.full((6, 8), 255, np.uint8)
    edge = np.array([[-1.0, 2, 1], [8.0, 2, 1], [7.0, 2, 1], [2.0, -1, 1], [2.0, 6, 1], [2.0, 5, 1]])
    assert _np(D.points_in_masks_device(edge, [HT.IDENTITY], [full], None)).tolist() == [1, 0, 1, 1, 0, 1]


def test_golden_at_full_resolution():
    g = HT.golden()
    masks = np.stack(g["masks"])
    dil = _np(D.dilate_ellipse_device(masks, 11))
    assert np.array_equal(dil, np.stack(g["dilated"]))
    count = D.points_in_masks_device(g["vertices"], g["P"], masks, 11)
    assert np.array_equal(_np(count), D.points_in_masks(g["vertices"], g["P"], g["dilated"], None))
    v1, f1 = D.clean_faces_by_mask_device(g["vertices"], g["faces"], count, 1)
    assert v1.dtype == torch.float64 and f1.dtype == torch.int64
    HT.check_against_golden(_np(count), _np(v1), _np(f1))


def test_vertex_compaction_keeps_order_and_unreferenced_vertices():
    g = np.random.default_rng(3)
    v = g.standard_normal((700, 3))
    f = g.integers(0, 700, (1500, 3))
    for count in (g.integers(0, 4, 700).astype(np.int32),            # a mixture
                  np.zeros(700, np.int32),                           # nothing kept
                  np.full(700, 3, np.int32)):                        # everything kept
        hv, hf = D.clean_faces_by_mask(v, f, count, 1)
        dv, df = D.clean_faces_by_mask_device(v, f, count, 1)
        assert np.array_equal(_np(dv), hv) and np.array_equal(_np(df), hf) and _np(df).shape == hf.shape
    count = np.zeros(700, np.int32)
    count[::2] = 2                                                   # every face has an odd vertex: no face survives
    f_odd = f.copy()
    f_odd[:, 0] |= 1
    hv, hf = D.clean_faces_by_mask(v, f_odd, count, 1)
    dv, df = D.clean_faces_by_mask_device(v, f_odd, count, 1)
    assert len(hv) == 350 and hf.shape == (0, 3) and np.array_equal(_np(dv), hv) and tuple(df.shape) == (0, 3)
    v32 = v.astype(np.float32)                                       # vertices keep the dtype they came in
    dv, _ = D.clean_faces_by_mask_device(v32, f, np.full(700, 2, np.int32), 1)
    assert dv.dtype == torch.float32 and np.array_equal(_np(dv), v32)
    # empty meshes come back empty
    dv, df = D.clean_faces_by_mask_device(v, f[:0], np.full(700, 2, np.int32), 1)
    assert np.array_equal(_np(dv), v) and tuple(df.shape) == (0, 3)
    dv, df = D.clean_faces_by_mask_device(v[:0], f[:0], np.zeros(0, np.int32), 1)
    assert tuple(dv.shape) == (0, 3) and tuple(df.shape) == (0, 3)
    P_list, masks = _small_views(2)
    assert tuple(D.points_in_masks_device(v[:0], P_list, masks, 11).shape) == (0,)
    for backend in ("host", "device"):
        ev, ef = D.clean_dtu(v[:0], f[:0], P_list, masks, backend=backend)
        assert ev.shape == (0, 3) and ef.shape == (0, 3)
        ev, ef, ei = D.clean_dtu(v, f[:0], P_list, masks, backend=backend, return_index=True)
        assert ev.shape == (0, 3) and ef.shape == (0, 3) and ei.shape == (0,)


def _sphere(res, radius, half=0.6):
    dev = torch.device("cuda:0")
    ax = torch.linspace(-half, half, res, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v, t = ops.marching_cubes((radius - torch.sqrt(x * x + y * y + z * z)).contiguous(), 0.0)
    return (v / (res - 1) * (2 * half) - half).double().cpu().numpy(), t.long().cpu().numpy()


def test_whole_scan_host_and_device_agree_and_the_floater_goes(tmp_path):
    root = tmp_path / "DTU_TEST"
    S.write_tree(str(root))
    sv, st = _sphere(72, 0.47)
    bv, bt = _sphere(8, 0.5)
    assert 15000 < len(st) < 30000 and 0 < len(bt) < 500
    centre = np.array([0.0, -10.0, -95.0])                           # in front of the sphere, inside all three masks' images
    v = np.concatenate([sv * 150.0, bv * 0.03 * 150.0 + centre[None]])
    f = np.concatenate([st, bt + len(sv)])
    # the floater passes the first stage (so only the component filter can remove it)
    _, P_list, masks = D.read_scan_views(str(root), S.SCAN)
    count = D.points_in_masks(v, P_list, masks, 11)
    assert (count[len(sv):] > 1).all() and 0 < (count[:len(sv)] > 1).sum() < len(sv)
    hv, hf, hi = D.clean_dtu_scan(v, f, str(root), S.SCAN, backend="host", return_index=True)
    dv, df, di = D.clean_dtu_scan(v, f, str(root), S.SCAN, backend="device", return_index=True)
    print(f"{len(f)} faces -> {len(hf)}; {len(v)} vertices -> {len(hv)}")
    assert hv.dtype == dv.dtype == np.float64 and np.array_equal(hv, dv) and np.array_equal(hf, df) and np.array_equal(hi, di)
    assert 500 <= len(hf) < len(st) and np.array_equal(v[hi], hv) and len(np.unique(hf)) == len(hv)
    assert np.linalg.norm(hv - centre[None], axis=1).min() > 10.0    # the floater (4.5 mm across) is gone
    tv, tf = D.clean_dtu_scan(v, f, str(root), S.SCAN, backend="device", return_tensors=True)
    assert tv.is_cuda and tf.is_cuda and np.array_equal(_np(tv), hv) and np.array_equal(_np(tf), hf)
    # stage by stage
    v1, f1 = D.clean_faces_by_mask(v, f, count, 1)
    h2 = D.clean_faces_outside_frustum(v1, f1, P_list, masks)
    d2 = D.clean_faces_outside_frustum_device(v1, f1, P_list, masks)
    assert np.array_equal(h2[0], _np(d2[0])) and np.array_equal(h2[1], _np(d2[1])) and np.array_equal(h2[1], hf)


def test_chamfer_script_with_the_protocol_cleaner(tmp_path):
    """scripts/dtu_chamfer.py on the synthetic DTU-format scene of tests/test_end_to_end_dtu.py: --clean_protocol dtu_test gives
    the same numbers with --clean_backend host and device; the default protocol is the runner's cleaner, unchanged."""
    from scipy.io import savemat
    from bench import surf_conf
    from tests.test_datasets import _ring_cams
    from tests.test_end_to_end_dtu import _write_scene
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    test_root = tmp_path / "DTU_TEST"
    os.makedirs(test_root / "cameras")
    os.makedirs(test_root / "scan24" / "mask")
    from PIL import Image
    K = np.array([[2892.33, 0, 823.2], [0, 2883.18, 619.07], [0, 0, 1.0]])
    for vid, w2c, m in zip(S.VIEW_IDS, _ring_cams(4), S.masks()):
        write_cam(str(test_root / "cameras" / f"{vid:08d}_cam.txt"), w2c, K, 425.0, 2.5)
        Image.fromarray(m).save(test_root / "scan24" / "mask" / f"{vid:03d}.png")
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    # evaluation files: a ball shell filled with points around the frusta's centre; the numbers only have to be reproducible
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
    lo, hi = np.full(3, -800.0), np.full(3, 800.0)
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8), "BB": np.stack([lo, hi]).astype(np.float32),
                                                  "Res": np.float32(1600.0 / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, 801.0]])})
    base = ["--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--downsample_density", "4.0",
            "--logit_override", "sphere"]

    def run(out, *extra):
        return dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / out)] + list(extra)))
    numbers = ("d2s", "s2d", "chamfer", "vertices", "triangles")
    plain = run("plain", "--mesh_resolution", "128")
    assert plain["clean_protocol"] is None and not plain["cleaned"]
    host = run("host", "--mesh_resolution", "128", "--clean_mesh", "--clean_protocol", "dtu_test", "--dtu_test_dir", str(test_root))
    devi = run("devi", "--mesh_resolution", "128", "--clean_mesh", "--clean_protocol", "dtu_test", "--dtu_test_dir", str(test_root),
               "--clean_backend", "device", "--vertex_colors")
    print({k: (plain[k], host[k], devi[k]) for k in numbers})
    assert host["clean_protocol"] == devi["clean_protocol"] == "dtu_test" and host["cleaned"] and devi["clean_backend"] == "device"
    assert all(host[k] == devi[k] for k in numbers) and np.isfinite(host["chamfer"])
    assert 0 < host["triangles"] < plain["triangles"] and host["seconds"]["clean"] > 0
    from surf_amd import mesh_io
    hv, hf = mesh_io.read_ply(host["mesh"])
    dv, df, attrs = mesh_io.read_ply(devi["mesh"], attributes=True)                   # --vertex_colors: same geometry, gathered attributes
    assert np.array_equal(hv, dv) and np.array_equal(hf, df)
    assert attrs["normals"].shape == dv.shape and attrs["colors"].shape == dv.shape
    # the default protocol is the runner's cleaner: naming it changes nothing
    r0 = run("r0", "--mesh_resolution", "128", "--clean_mesh")
    r1 = run("r1", "--mesh_resolution", "128", "--clean_mesh", "--clean_protocol", "runner")
    assert r0["clean_protocol"] == r1["clean_protocol"] == "runner" and all(r0[k] == r1[k] for k in numbers)
    assert open(r0["mesh"], "rb").read() == open(r1["mesh"], "rb").read()
    with pytest.raises(SystemExit):
        run("bad", "--clean_mesh", "--clean_protocol", "dtu_test")
