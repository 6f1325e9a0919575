"""GPU: csrc/ray_cast.hip against the host mirror fusion.ray_cast_host (the rule of the kernel's header comment in numpy fp32) -
equal arrays, not tolerances - on the lattices of tests/test_ray_cast_host.py: dense and brick-major state, image sizes with
partial tiles and partial wavefronts, cameras outside and inside the lattice; dense against brick-sparse on the device; the
ray-cast depth against the rasterised depth of the extracted mesh; the C ABI's status codes; and scripts/fuse_scene.py
--render_views."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import _lib, fusion, ops
from surf_amd.fusion import FusionVolume
from tests.test_fusion_gpu import camera
from tests.test_fusion_host import look_at
from tests.test_fusion_sparse_host import lattice_bricks, sphere_scene
from tests.test_ray_cast_host import (SPHERE_H, SPHERE_LO, SPHERE_SHAPE, sphere_camera, sphere_lattice, sphere_volume)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [(1, 1), (7, 5), (65, 9), (64, 64)]        # one lane; a partial 8 x 8 tile; five block rows with a ragged edge; 16 full tiles


@pytest.fixture(scope="module")
def analytic():
    """The analytic sphere written into a dense device volume, and its state on the host."""
    tsdf, weight, color = sphere_lattice()
    vol = sphere_volume(backend="device", device=DEV)
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    vol.color.copy_(torch.from_numpy(color))
    return vol, (tsdf, weight, color)


@pytest.fixture(scope="module")
def fused():
    """The sphere scene of the brick-sparse fusion tests fused on the device, dense and brick-sparse, and the sparse state on the
    host (the device state: the host mirror of the ray cast runs on exactly what the kernel reads)."""
    axes, views, trunc = sphere_scene()
    lo, h, shape = np.array([-0.375, -0.34, -0.40]), 1.0 / 128, (97, 89, 104)
    grid = (lo, lo + h * (np.array(shape) - 1), h)
    dense = FusionVolume(grid, trunc=trunc, colors=True, device=DEV)
    sparse = FusionVolume(grid, trunc=trunc, colors=True, device=DEV, sparse=True)
    assert dense.shape == shape and all(np.array_equal(a, b) for a, b in zip(dense.axes_host, axes))
    dense.integrate(views)
    sparse.integrate(views)
    sparse.finalize()
    n_box = lattice_bricks(shape)
    assert 27 <= sparse.n_bricks < n_box                    # some brick inside the lattice box is not allocated
    host_state = tuple(x.cpu().numpy() for x in (sparse.tsdf, sparse.weight, sparse.color, sparse.table))
    return dense, sparse, host_state, views


def fused_camera(which, hw):
    H, W = hw
    if which == "outside":
        return camera((-0.6, 0.2, -2.0), (0.6, -0.2, 2.0), 160.0 * max(H, W) / 64.0, H, W)
    return camera((0.05, -0.33, -0.39), (0.0, 0.3, 0.4), 30.0 * max(H, W) / 64.0, H, W)         # inside the lattice


def assert_equal(dev_out, host_out, what):
    for k, h in zip(("depth", "normal", "color"), host_out):
        d = dev_out[k]
        assert d.dtype == np.float32 and d.shape == h.shape, (what, k)
        assert np.array_equal(d, h), (what, k, int((d != h).sum()), float(np.abs(d - h).max()))


@pytest.mark.parametrize("which", ["outside", "inside"])
@pytest.mark.parametrize("hw", SIZES)
def test_dense_device_equals_host(analytic, hw, which):
    vol, (tsdf, weight, color) = analytic
    P = sphere_camera(which, hw)
    host = fusion.ray_cast_host(tsdf, weight, color, SPHERE_SHAPE, fusion.ray_lift(P, SPHERE_LO, SPHERE_H), hw)
    out = vol.ray_cast(P, hw)
    assert_equal(out, host, (hw, which))
    hits = int((host[0] > 0).sum())
    print(f"{hw} {which}: {hits} of {hw[0] * hw[1]} rays hit")
    assert hits >= 1 and (hw[0] * hw[1] < 30 or hits < hw[0] * hw[1])           # hits and (on an image of any size) misses
    if hw == (7, 5):                                         # isovalues, z_min and normals=False take the same path
        for kw in (dict(isovalue=0.5), dict(isovalue=-0.5), dict(z_min=1.0)):
            lvl = -kw.get("isovalue", 0.0)
            h2 = fusion.ray_cast_host(tsdf, weight, color, SPHERE_SHAPE, fusion.ray_lift(P, SPHERE_LO, SPHERE_H), hw, kw.get("z_min", 0.0), lvl)
            assert_equal(vol.ray_cast(P, hw, **kw), h2, (hw, which, kw))
        bare = vol.ray_cast(P, hw, normals=False)
        assert bare["normal"] is None and np.array_equal(bare["depth"], host[0]) and np.array_equal(bare["color"], host[2])
        plain = ops.fuse_ray_cast(vol.tsdf, vol.weight, None, fusion.ray_lift(P, SPHERE_LO, SPHERE_H), hw)
        assert plain[2] is None and np.array_equal(plain[0].cpu().numpy(), host[0]) and np.array_equal(plain[1].cpu().numpy(), host[1])


@pytest.mark.parametrize("which", ["outside", "inside"])
@pytest.mark.parametrize("hw", SIZES)
def test_sparse_device_equals_host(fused, hw, which):
    dense, sparse, (tsdf, weight, color, table), _ = fused
    P = fused_camera(which, hw)
    lo, voxel = sparse.lattice()
    host = fusion.ray_cast_host(tsdf, weight, color, sparse.shape, fusion.ray_lift(P, lo, voxel), hw, table=table)
    assert_equal(sparse.ray_cast(P, hw), host, (hw, which))
    hits = int((host[0] > 0).sum())
    print(f"{hw} {which}: {hits} of {hw[0] * hw[1]} rays hit")
    assert hits >= 1 and (hw[0] * hw[1] < 30 or hits < hw[0] * hw[1])


def test_dense_device_equals_sparse_device(fused):
    dense, sparse, _, views = fused
    cams = [(views[0].P, tuple(views[0].depth.shape)), (views[3].P, tuple(views[3].depth.shape)),
            (fused_camera("inside", (40, 56)), (40, 56)), (fused_camera("outside", (65, 9)), (65, 9))]
    for P, hw in cams:
        for iso in (0.0, 0.5, -0.5):
            a, b = dense.ray_cast(P, hw, isovalue=iso), sparse.ray_cast(P, hw, isovalue=iso)
            for k in ("depth", "normal", "color"):
                assert np.array_equal(a[k], b[k]), (hw, iso, k, int((a[k] != b[k]).sum()))
            assert (a["depth"] > 0).sum() >= 50 and (a["depth"] == 0).sum() >= 50
    # return_tensors: device tensors, no host copy, the numpy result's values
    P, hw = cams[0]
    for vol in (dense, sparse):
        t, a = vol.ray_cast(P, hw, return_tensors=True), vol.ray_cast(P, hw)
        for k in ("depth", "normal", "color"):
            assert torch.is_tensor(t[k]) and t[k].is_cuda and t[k].dtype == torch.float32 and np.array_equal(t[k].cpu().numpy(), a[k]), k
    # the model reproduces the view it was fused from
    res = fusion.view_residual(views[0], dense.ray_cast(views[0].P, views[0].depth.shape))
    assert res["hit_share"] > 0.9 and res["median_voxels"] < 1.0
    # nothing allocated: no hit, on the device
    empty = FusionVolume((np.zeros(3), np.ones(3), 0.25), device=DEV, sparse=True)
    out = empty.ray_cast(P, (4, 6), return_tensors=True)
    assert out["depth"].is_cuda and not out["depth"].any() and out["color"] is None and out["normal"].shape == (4, 6, 3)


def test_ray_cast_depth_against_the_rasterised_mesh(analytic):
    """Ray-cast depth against the depth of extract_mesh()'s triangle that raster_first_hit finds through the same pixel.  On a
    pixel whose own hit and whose eight neighbours' hits exist in both maps (away from the silhouette) both surfaces lie in the same
    lattice cell - marching cubes' triangles and the interpolant's zero set share the cell's edge crossings - so the depths differ
    by less than the cell's diagonal: sqrt(3) lattice steps along the ray."""
    vol, _ = analytic
    H = W = 64
    K, w2c = look_at((0.9, -0.7, -3.2), 120.0, H, W)
    P = (K @ w2c[:3, :4]).astype(np.float32)
    cast = vol.ray_cast(P, (H, W))["depth"].astype(np.float64)
    v, t, _ = vol.extract_mesh()
    assert len(t) > 1000
    K4 = np.eye(4)
    K4[:3, :3] = K
    face = ops.raster_first_hit(torch.from_numpy(v.astype(np.float32)).to(DEV), torch.from_numpy(t.astype(np.int32)).to(DEV),
                                torch.from_numpy(K4).float(), torch.from_numpy(np.linalg.inv(w2c)).float(), (H, W)).cpu().numpy()
    # z-depth of the pixel's ray on the plane of its triangle, float64
    M_inv = np.linalg.inv(P.astype(np.float64)[:, :3])
    o = -M_inv @ P.astype(np.float64)[:, 3]
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ M_inv.T
    tri = v[t[np.maximum(face, 0)]]                                            # (H, W, 3, 3)
    nrm = np.cross(tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :])
    with np.errstate(all="ignore"):
        mesh = np.where(face >= 0, ((tri[..., 0, :] - o) * nrm).sum(-1) / (d * nrm).sum(-1), 0.0)
    both = (cast > 0) & (face >= 0)

    def eroded(m):
        p = np.pad(m, 1)
        return np.logical_and.reduce([p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    inner = eroded(cast > 0) & eroded(face >= 0)
    steps = np.abs(cast - mesh) * np.linalg.norm(d, axis=-1) / SPHERE_H        # along the ray, in lattice steps
    print(f"{int((cast > 0).sum())} ray-cast hits, {int((face >= 0).sum())} raster hits, {int(inner.sum())} compared: "
          f"max {steps[inner].max():.3f}, median {np.median(steps[inner]):.4f} lattice steps")
    assert inner.sum() >= 100 and (inner <= both).all()
    assert steps[inner].max() < np.sqrt(3.0)


def test_status_codes_through_the_c_abi(analytic):
    vol, _ = analytic
    L = _lib.lib()
    for name in ("surf_fuse_ray_cast", "surf_fuse_ray_cast_bricks"):
        assert name in _lib.SIGNATURES and getattr(L, name).errcheck is not None
    nx, ny, nz = SPHERE_SHAPE
    lift = np.ascontiguousarray(fusion.ray_lift(sphere_camera("outside", (4, 4)), SPHERE_LO, SPHERE_H))
    lp = lift.ctypes.data_as(_lib.ctypes.c_void_p)
    ts, we = vol.tsdf.data_ptr(), vol.weight.data_ptr()
    out = torch.full((4, 4), 7.0, device=DEV)
    table = torch.full((6 ** 3,), -1, dtype=torch.int32, device=DEV)
    ok = dict(tsdf=ts, weight=we, color=None, nx=nx, ny=ny, nz=nz, lift=lp, H=4, W=4, z_min=0.0, level=0.0, depth=out.data_ptr(),
              normal=None, out_color=None)

    def call(bricks=False, **kw):
        a = {**ok, **kw}
        head = (a["tsdf"], a["weight"], a["color"]) + ((a.get("table", table.data_ptr()), a.get("n_slots", 4)) if bricks else ())
        fn = L.surf_fuse_ray_cast_bricks if bricks else L.surf_fuse_ray_cast
        return fn(*head, a["nx"], a["ny"], a["nz"], a["lift"], a["H"], a["W"], a["z_min"], a["level"], a["depth"], a["normal"],
                  a["out_color"], None)
    for bricks in (False, True):
        for bad in (dict(tsdf=None), dict(weight=None), dict(lift=None), dict(depth=None), dict(nx=0), dict(nz=-3), dict(H=-1),
                    dict(level=1.0), dict(level=-1.0), dict(z_min=-0.5), dict(z_min=float("nan")), dict(color=vol.color.data_ptr()),
                    dict(out_color=out.data_ptr())):
            with pytest.raises(_lib.SurfHipError, match="invalid"):
                call(bricks, **bad)
        for zero in (dict(H=0), dict(W=0), dict(H=0, W=0)):                     # H W == 0: success, nothing launched
            assert call(bricks, **zero) == 0
        for big in (dict(H=50000, W=50000), dict(H=(1 << 24) + 1, W=1), dict(nx=1, ny=1, nz=(1 << 24) + 1)):
            with pytest.raises(_lib.SurfHipError, match="exceeds"):
                call(bricks, **big)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        call(True, table=None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        call(True, n_slots=-1)
    for big in (dict(nx=70000), dict(ny=1 << 16, nz=1 << 15)):                  # surf_fuse_integrate's limits
        with pytest.raises(_lib.SurfHipError, match="exceeds"):
            call(False, **big)
    for big in (dict(nx=8193), dict(n_slots=1 << 22)):                          # surf_fuse_integrate_bricks' limits
        with pytest.raises(_lib.SurfHipError, match="exceeds"):
            call(True, **big)
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                   # none of these calls wrote anything
    assert call(False) == 0
    torch.cuda.synchronize()
    assert (out != 7.0).all()                                                   # every pixel is written, hit or not


def test_fuse_scene_render_views(tmp_path):
    """scripts/fuse_scene.run on the synthetic DTU-format scene with and without --render_views: the switch adds the maps, the
    `model_residual` block and `render_views_ms`; everything else - the record, the mesh file - is byte for byte what it is without."""
    from bench import surf_conf
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
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--resolution", "64", "--colors", "--logit_override",
              "sphere", "--out_dir", str(tmp_path / "out")]
    plain = fuse_scene.run(fuse_scene.parse_args(common))
    plain_json = open(tmp_path / "out" / "fused_scan24.json").read()
    plain_mesh = open(plain["mesh"], "rb").read()
    assert "model_residual" not in plain and "render_views_ms" not in plain and not (tmp_path / "out" / "renders").exists()
    state = {}
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--render_views"]), state)
    assert open(rec["mesh"], "rb").read() == plain_mesh
    extra = {"model_residual", "render_views_ms"}
    assert set(rec) - set(plain) == extra and rec["render_views_ms"] > 0
    strip = lambda r: {k: ({m: 0 for m in v} if k == "ms" else v) for k, v in r.items() if k not in extra}      # noqa: E731
    assert json.dumps(strip(rec)) == json.dumps(strip(plain)) == json.dumps(strip(json.loads(plain_json)))       # same keys, order, values
    block = rec["model_residual"]
    assert block["dir"] == str(tmp_path / "out" / "renders" / "scan24") and len(block["views"]) == 2
    vol = state["volume"]
    for entry in block["views"]:
        depth, _ = mvs_io.read_pfm(os.path.join(block["dir"], entry["view"] + "_depth.pfm"))
        assert depth.shape == (H // 2, W // 2) and entry["hit"] <= (depth > 0).sum()
        for kind in ("normal", "color"):
            from PIL import Image
            img = np.array(Image.open(os.path.join(block["dir"], f"{entry['view']}_{kind}.png")))
            assert img.shape == (H // 2, W // 2, 3) and img.dtype == np.uint8 and (img[depth == 0] == 0).all() and img[depth > 0].any()
        assert 0 < entry["hit"] <= entry["measured"] and entry["hit_share"] == entry["hit"] / entry["measured"]
        assert entry["median"] <= entry["p90"] and abs(entry["median_voxels"] * rec["voxel"] - entry["median"]) < 1e-9
    pooled = block["pooled"]
    assert pooled["hit"] == sum(e["hit"] for e in block["views"]) and 0 <= pooled["median_voxels"] <= pooled["p90_voxels"]
    assert sorted(e["view"] for e in block["views"]) == ["scan24_view001", "scan24_view002"]
    assert json.load(open(tmp_path / "out" / "fused_scan24.json"))["model_residual"]["pooled"] == pooled
    assert vol.n_views == 2 and len(os.listdir(block["dir"])) == 6
    assert fuse_scene.parse_args(common + ["--render_views", "maps"]).render_views == "maps"        # a directory of one's own
