"""GPU: csrc/fuse.hip and surf_mc_classify_observed against the host path of surf_amd.fusion (the numpy-fp32 mirror of the update
sequence in fuse.hip's header comment) and oracle/mcubes_oracle.py - equality, not tolerances - plus the public interface above
them: FusionVolume, ipts["extract_geometry"] = False and scripts/fuse_scene.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import fusion, ops
from surf_amd.fusion import DepthView, FusionVolume
from tests.test_fusion_host import PLANE_H, index_to_world, lattice_of, neighbour_delta, observed_triangles, plane_scene, sort_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPE = (13, 9, 70)              # nz is no multiple of 64: wavefronts straddle rows; 8190 points = 32 blocks of 256, the last partial


def ragged_axes():
    """13 x 9 x 70 lattice points, unevenly spaced (any spacing is allowed)."""
    g = np.random.default_rng(2)
    axes = []
    for n, (lo, hi) in zip(SHAPE, ((-0.6, 0.6), (-0.4, 0.4), (-1.0, 1.2))):
        steps = 1.0 + 0.3 * g.random(n - 1)
        axes.append((lo + (hi - lo) * np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum()).astype(np.float32))
    return axes


def camera(centre, forward, f, H, W):
    """P (3, 4) fp32 of a pinhole camera at `centre` whose optical axis is `forward`."""
    c, z = np.asarray(centre, np.float64), np.asarray(forward, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z) if abs(z[1]) < 0.9 else np.cross([1.0, 0.0, 0.0], z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), c
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return (K @ np.linalg.inv(c2w)[:3, :4]).astype(np.float32)


def ragged_views():
    """Three views on the ragged lattice:
    a (11, 17): in front of the lattice, sees nearly all of it; its map holds a 0, a negative, a NaN and an inf; the surface
                (depth ~ 3 from z = -3) cuts the lattice, whose far end lies beyond trunc behind it;
    b (8, 8):   INSIDE the lattice (part of it is behind the camera), depth in units of 1 / 2.5 (dscale 2.5);
    c (5, 23):  from the side with a long lens: its frustum covers a part of the lattice only."""
    g = np.random.default_rng(3)
    da = (3.0 + 0.3 * g.standard_normal((11, 17))).astype(np.float32)
    da[2, 3], da[4, 9], da[7, 1], da[9, 15] = 0.0, -1.5, np.nan, np.inf
    db = ((0.6 + 0.2 * g.random((8, 8))) / 2.5).astype(np.float32)
    dc = (3.0 + 0.2 * g.standard_normal((5, 23))).astype(np.float32)
    imgs = [(0.05 + 0.9 * g.random(d.shape + (3,))).astype(np.float32) for d in (da, db, dc)]
    return [DepthView(camera((0.0, 0.0, -3.0), (0, 0, 1), 30.0, 11, 17), da, 1.0, imgs[0]),
            DepthView(camera((0.05, 0.0, 0.1), (0.1, 0, 1), 3.0, 8, 8), db, 2.5, imgs[1]),
            DepthView(camera((-3.0, 0.05, 0.1), (1, 0, 0), 40.0, 5, 23), dc, 1.0, imgs[2])]


def fused(axes, views, trunc, backend, colors=True, splits=()):
    vol = FusionVolume(axes, trunc=trunc, colors=colors, backend=backend, device=DEV)
    start = 0
    for s in tuple(splits) + (len(views),):
        vol.integrate(views[start:s])
        start = s
    return vol


def assert_state_equal(dev_vol, host_vol):
    for k in ("tsdf", "weight", "color"):
        a, b = getattr(dev_vol, k), getattr(host_vol, k)
        if b is None:
            assert a is None
            continue
        b = b if torch.is_tensor(b) else torch.from_numpy(b)
        assert torch.equal(a.cpu(), b.cpu()), (k, int((a.cpu() != b.cpu()).sum()))


def test_integrate_device_equals_host():
    axes, views, trunc = ragged_axes(), ragged_views(), 0.25
    stats = {}
    host = FusionVolume(axes, trunc=trunc, colors=True, backend="host")
    host.integrate(views, stats=stats)
    # conditions on the inputs: every skip reason fires, some point is updated by two views, nothing is near a denormal
    assert all(stats[k] > 0 for k in fusion.SKIP_REASONS + ("updated",)), stats
    assert float(host.weight.max()) >= 2.0 and 0.1 < host.observed_share() < 0.95
    seen = host.weight > 0
    assert float(np.abs(host.tsdf[seen]).min()) > 1e-30 and float(host.color[seen].min()) > 1e-3
    per_view = []
    for v in views:                                            # each view alone updates some points and skips others
        one = FusionVolume(axes, trunc=trunc, backend="host")
        one.integrate([v._replace(image=None)])
        per_view.append(one.observed_share())
    assert all(0.0 < s < 1.0 for s in per_view), per_view
    dev = fused(axes, views, trunc, "device")
    assert_state_equal(dev, host)
    assert dev.n_views == 3 and dev.tsdf.is_cuda and tuple(dev.color.shape) == SHAPE + (3,)
    # without colours: the other instantiation of the kernel
    assert_state_equal(fused(axes, views, trunc, "device", colors=False), fused(axes, views, trunc, "host", colors=False))


def test_seventeen_views_take_two_launches():
    axes, trunc = ragged_axes(), 0.3
    g = np.random.default_rng(4)
    views = []
    for i in range(17):
        a = 2 * np.pi * i / 17
        c = np.array([2.5 * np.sin(a), 0.4 * np.cos(3 * a), -2.5 * np.cos(a)])
        views.append(DepthView(camera(c, -c, 4.0, 4, 5), (2.5 + 0.4 * g.standard_normal((4, 5))).astype(np.float32), 1.0,
                               (0.05 + 0.9 * g.random((4, 5, 3))).astype(np.float32)))
    assert len(views) > ops.FUSE_MAX_VIEWS
    host = fused(axes, views, trunc, "host")
    assert float(host.weight.max()) >= 8.0
    dev = fused(axes, views, trunc, "device")
    assert_state_equal(dev, host)
    for split in (1, 9, 16):
        assert_state_equal(fused(axes, views, trunc, "device", splits=(split,)), host)
    from surf_amd import _lib
    with pytest.raises(_lib.SurfHipError, match="limit"):
        ops.fuse_integrate(dev.tsdf, dev.weight, None, dev.axes,
                           [(v.P, torch.from_numpy(v.depth).to(DEV), 1.0, None) for v in views], trunc)


def tri9(v, t):
    return sort_rows(v[t.astype(np.int64)].reshape(-1, 9))


def test_marching_cubes_observed_only():
    g = np.random.default_rng(7)
    u = g.standard_normal((9, 10, 11)).astype(np.float32)
    full = torch.from_numpy(u).to(DEV)
    u[g.random(u.shape) < 0.15] = np.nan
    assert 0.1 < np.isnan(u).mean() < 0.2
    v, t = ops.marching_cubes(torch.from_numpy(u).to(DEV), 0.0, observed_only=True)
    v, t = v.cpu().numpy(), t.cpu().numpy()
    ref = observed_triangles(u)
    assert len(ref) > 200 and np.isfinite(v).all()
    assert np.array_equal(tri9(v, t), ref)
    assert len(np.unique(t)) == len(v) and t.min() == 0 and t.max() == len(v) - 1           # no vertex is unreferenced
    # fewer triangles than the cells of the full lattice give, and vertices were dropped: the rule and the compaction both act
    v_plain, t_plain = ops.marching_cubes(torch.from_numpy(u).to(DEV), 0.0)
    assert len(t) < len(t_plain) and len(v) < len(v_plain)
    # all finite: the default call, array for array
    a, b = ops.marching_cubes(full, 0.0, observed_only=True), ops.marching_cubes(full, 0.0)
    assert len(b[1]) > 500 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].dtype == torch.float64 and a[1].dtype == torch.int32
    # nothing observed: an empty mesh
    v0, t0 = ops.marching_cubes(torch.full((4, 5, 6), float("nan"), device=DEV), 0.0, observed_only=True)
    assert tuple(v0.shape) == (0, 3) and tuple(t0.shape) == (0, 3)
    # vertices without a fully observed cell around them and no triangle at all
    lone = torch.full((3, 3, 3), float("nan"), device=DEV)
    lone[1, 1, 1], lone[1, 1, 2] = -1.0, 1.0
    v1, t1 = ops.marching_cubes(lone, 0.0, observed_only=True)
    assert tuple(v1.shape) == (0, 3) and tuple(t1.shape) == (0, 3)


def test_plane_scene_on_the_device():
    axes, views, trunc = plane_scene()
    host = FusionVolume(axes, trunc=trunc, backend="host")
    host.integrate(views)
    dev = fused(axes, views, trunc, "device", colors=False)
    assert_state_equal(dev, host)
    u = ops.fuse_lattice(dev.tsdf, dev.weight)
    u_host = lattice_of(host.tsdf, host.weight)
    assert np.array_equal(u.cpu().numpy(), u_host, equal_nan=True)
    ref = observed_triangles(u_host)
    v, t = ops.marching_cubes(u, 0.0, observed_only=True)
    assert len(ref) == 3290 and np.array_equal(tri9(v.cpu().numpy(), t.cpu().numpy()), ref)
    # the public call: world frame, the derived distance bound (tests/test_fusion_host.py), the x range
    vw, tw = dev.extract_mesh()
    assert vw.dtype == np.float64 and tw.dtype == np.int64 and np.array_equal(tw, t.cpu().numpy())
    assert np.allclose(tri9(vw, tw), sort_rows(index_to_world(tri9(v.cpu().numpy(), t.cpu().numpy()), axes)), rtol=0, atol=1e-6)
    bound = PLANE_H + max(neighbour_delta(x.depth) for x in views)
    dist = float(np.abs(vw[:, 2]).max())
    print(f"plane scene on the device: {len(tw)} triangles, max distance {dist:.4f}, bound {bound:.4f}")
    assert dist <= bound and vw[:, 0].min() <= -0.5 + PLANE_H and vw[:, 0].max() >= 0.5 - PLANE_H
    assert float(dev.weight.max()) == 3.0
    # the host backend's mesh step runs on the device: the same mesh
    vh, th = host.extract_mesh()
    assert np.array_equal(vh, vw) and np.array_equal(th, tw)


def vertex_colors_mirror(vertices, color):
    """The rule of fuse.hip's header comment in numpy: fp32, one operation per operator."""
    f32 = np.float32
    n = np.array(color.shape[:3])
    fl = np.clip(np.floor(vertices), 0, n - 1)
    fr = vertices - fl
    axis = np.argmax(fr != 0, axis=1)                               # the first axis with a fractional part (none: 0)
    rows = np.arange(len(vertices))
    f = fr[rows, axis].astype(f32)
    lo = fl.astype(np.int64)
    hi = lo.copy()
    hi[rows, axis] = np.minimum(lo[rows, axis] + 1, n[axis] - 1)
    c_lo, c_hi = color[lo[:, 0], lo[:, 1], lo[:, 2]], color[hi[:, 0], hi[:, 1], hi[:, 2]]
    c = c_lo + (c_hi - c_lo) * f[:, None]
    q = np.minimum(np.maximum(c * f32(256.0), f32(0.0)), f32(255.0))
    return q.astype(np.uint8)


def test_vertex_colours_equal_the_numpy_mirror():
    axes, views, trunc = plane_scene(colors=True)
    dev = fused(axes, views, trunc, "device")
    v, t = ops.marching_cubes(ops.fuse_lattice(dev.tsdf, dev.weight), 0.0, observed_only=True)
    got = ops.fuse_vertex_colors(v, dev.color).cpu().numpy()
    want = vertex_colors_mirror(v.cpu().numpy(), dev.color.cpu().numpy())
    assert got.dtype == np.uint8 and got.shape == (len(v), 3) and np.array_equal(got, want)
    assert len(np.unique(got)) > 50                                 # real colours, not one value
    # a colour lattice that leaves [0, 1) and synthetic vertices on every axis, on lattice points and on the last plane
    g = np.random.default_rng(9)
    color = torch.from_numpy((g.standard_normal((5, 6, 7, 3)) * 0.8 + 0.5).astype(np.float32)).to(DEV)
    pts = g.integers(0, [5, 6, 7], size=(300, 3)).astype(np.float64)
    ax = g.integers(0, 3, size=300)
    frac = np.where(g.random(300) < 0.2, 0.0, g.random(300))
    last = pts[np.arange(300), ax] == np.array([4, 5, 6])[ax]
    pts[np.arange(300), ax] += np.where(last, 0.0, frac)
    got = ops.fuse_vertex_colors(torch.from_numpy(pts).to(DEV), color).cpu().numpy()
    assert np.array_equal(got, vertex_colors_mirror(pts, color.cpu().numpy())) and got.min() == 0 and got.max() == 255
    # extract_mesh returns them as its third array
    mesh = dev.extract_mesh()
    assert len(mesh) == 3 and mesh[2].dtype == np.uint8 and np.array_equal(mesh[2], ops.fuse_vertex_colors(v, dev.color).cpu().numpy())


def test_val_forward_without_geometry(scene):
    """ipts["extract_geometry"] = False on the tiny scene of test_hip_parity's end-to-end `val` test: no mesh keys, every other
    output bit-equal to the default forward's."""
    from surf_amd import conf
    from surf_amd.surf import SuRF
    from tests.golden.make_golden import MODEL_CONF
    cfg = {k: v for k, v in MODEL_CONF.items()}
    cfg["reg_network"] = {"d_in": [8, 16, 16, 16], "d_base": [8] * 4, "d_out": [8] * 4}
    torch.manual_seed(1)
    model = SuRF(conf.from_dict(cfg)).eval()
    with torch.no_grad():
        model.implicit_surface.deviation_network.variance.fill_(0.45)
        for net in model.reg_network.nets:
            net.out_lin.weight.mul_(4.0)
    model = model.to(DEV)
    ipts = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in scene.items()}
    ipts["bound_min"], ipts["bound_max"] = torch.tensor([-0.8] * 3), torch.tensor([0.8] * 3)
    ipts["hw"] = (7, 8)
    ipts["mesh_resolution"] = 32
    with torch.no_grad():
        full = model("val", ipts, 1.0)
        bare = model("val", {**ipts, "extract_geometry": False}, 1.0)
    assert "vertices" in full and "triangles" in full and len(full["triangles"]) > 0
    assert set(full) - set(bare) == {"vertices", "triangles"} and set(bare) <= set(full)
    assert {"sdf_depth", "render_depth", "color_fine", "img_fine"} <= set(bare)
    for k, b in bare.items():
        a = full[k]
        if torch.is_tensor(a):
            assert torch.equal(a.cpu(), b.cpu()), k
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b, equal_nan=True), k
        else:
            assert a == b, k


def test_fuse_scene_script(tmp_path):
    """scripts/fuse_scene.run on the synthetic DTU-format scene of tests/test_end_to_end_dtu.py: two reference views, 64 lattice
    points along the longest side."""
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
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import fuse_scene
    state = {}
    rec = fuse_scene.run(fuse_scene.parse_args(["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--resolution", "64",
                                                "--colors", "--logit_override", "sphere", "--out_dir", str(tmp_path / "out")]), state)
    assert {"scan", "views_fused", "lattice", "observed_share", "vertices", "triangles", "ms", "mesh"} <= set(rec)
    assert {"load", "lattice", "forward", "integrate", "extract", "write"} <= set(rec["ms"]) and "chamfer" not in rec
    assert rec["views_fused"] == 2 and len(rec["lattice"]) == 3 and max(rec["lattice"]) == 64 and 0.0 < rec["observed_share"] < 1.0
    assert float(state["volume"].weight.max()) == 2.0
    v, t, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert len(v) == rec["vertices"] > 100 and len(t) == rec["triangles"] > 100 and attrs["colors"].shape == (len(v), 3)
    assert np.isfinite(v).all() and t.max() == len(v) - 1
    assert json.load(open(tmp_path / "out" / "fused_scan24.json"))["triangles"] == rec["triangles"]
