"""GPU: csrc/fuse_sparse.hip against the host mirror (equal brick lists, tables and state) and the brick-sparse FusionVolume's mesh
against the dense volume's, array for array - also on a lattice of 2.7 G points that the dense path cannot hold - plus
scripts/fuse_scene.py --sparse.  Equality, not tolerances (one float64 rounding bound in the large-lattice test is derived there)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import fusion
from surf_amd.fusion import FusionVolume
from tests.test_fusion_gpu import DEV, ragged_axes
from tests.test_fusion_sparse_host import SCENES, seventeen_views, sphere_views

pytestmark = pytest.mark.gpu

# triangles of the dense mesh at isovalue 0 (the condition "at least 1000" comes from the dense path: these are the counts of
# tests/test_fusion_host.py's observed_triangles on the dense host lattice); the ragged scene's lattice is 13 x 9 x 70 points
TRIANGLES = {"slab": 11084, "sphere": 35359}


def volume(axes, views, trunc, backend, colors=True, sparse=True):
    vol = FusionVolume(axes, trunc=trunc, colors=colors, backend=backend, device=DEV, sparse=sparse)
    vol.integrate(views if colors else [v._replace(image=None) for v in views])
    return vol


def assert_sparse_state_equal(dev, host):
    for k in ("bricks", "table", "tsdf", "weight", "color"):
        a, b = getattr(dev, k), getattr(host, k)
        if b is None:
            assert a is None, k
            continue
        b = torch.from_numpy(b)
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, tuple(a.shape), tuple(b.shape))
        assert torch.equal(a.cpu(), b), (k, int((a.cpu() != b).sum()))
    assert dev.n_bricks == host.n_bricks and dev.allocated_share() == host.allocated_share()
    assert dev.observed_share() == host.observed_share() and dev.state_bytes() == host.state_bytes()


@pytest.fixture(scope="module")
def scenes():
    """name -> (axes, views, trunc, sparse device volume with colours), built once."""
    cache = {}

    def get(name):
        if name not in cache:
            axes, views, trunc = SCENES[name]()
            cache[name] = (axes, views, trunc, volume(axes, views, trunc, "device"))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["slab", "sphere", "ragged"])
def test_device_equals_host(scenes, name):
    axes, views, trunc, dev = scenes(name)
    host = volume(axes, views, trunc, "host")
    assert host.n_bricks > 30 and dev.bricks.dtype == torch.int32 and dev.tsdf.shape == (dev.n_bricks * 512,)
    assert_sparse_state_equal(dev, host)
    # without colours: the other instantiation of the kernel
    assert_sparse_state_equal(volume(axes, views, trunc, "device", colors=False), volume(axes, views, trunc, "host", colors=False))


def test_seventeen_views_take_two_launches():
    axes, views, trunc = ragged_axes(), seventeen_views(), 0.3
    assert len(views) > fusion.ops.FUSE_MAX_VIEWS
    host = volume(axes, views, trunc, "host")
    assert float(host.weight.max()) >= 8.0
    assert_sparse_state_equal(volume(axes, views, trunc, "device"), host)
    split = FusionVolume(axes, trunc=trunc, colors=True, backend="device", device=DEV, sparse=True)
    split.integrate(views[:9])
    assert split.finalize().n_views == 9
    split.integrate(views[9:])                               # after finalize(): rebuilt from all seventeen
    assert_sparse_state_equal(split, host)


def assert_mesh_equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (a.dtype, a.shape, b.shape)


@pytest.mark.parametrize("name", ["slab", "sphere", "ragged"])
def test_mesh_equals_the_dense_mesh(scenes, name):
    axes, views, trunc, sparse = scenes(name)
    dense = volume(axes, views, trunc, "device", sparse=False)
    want = dense.extract_mesh()
    print(f"{name}: {len(want[1])} triangles, {len(want[0])} vertices; {sparse.n_bricks} bricks, allocated share "
          f"{sparse.allocated_share():.3f}, observed share {dense.observed_share():.3f}")
    assert len(want) == 3 and want[2].dtype == np.uint8
    if name in TRIANGLES:
        assert len(want[1]) == TRIANGLES[name] >= 1000
        assert len(np.unique(want[2])) > 50                  # real colours
    assert_mesh_equal(sparse.extract_mesh(), want)
    assert sparse.observed_share() <= dense.observed_share()
    if name == "sphere":
        for iso in (-0.5, 0.5):
            want_iso = dense.extract_mesh(iso)
            assert len(want_iso[1]) > 1000 and not np.array_equal(want_iso[0][:100], want[0][:100])
            assert_mesh_equal(sparse.extract_mesh(iso), want_iso)
        # without colours, and from the host backend's state (uploaded for the mesh step)
        assert_mesh_equal(volume(axes, views, trunc, "device", colors=False).extract_mesh(), want[:2])
        assert_mesh_equal(volume(axes, views, trunc, "host").extract_mesh(), want)
        for iso in (-1.0, 1.0, float("nan")):
            with pytest.raises(ValueError, match="isovalue"):
                sparse.extract_mesh(iso)


def interior_triangles(v, t, axes, lo, n):
    """The (F, 9) world-coordinate rows, in mesh order, of the triangles whose cell (the one that holds the centroid) has its
    origin index in [lo + 1, lo + n - 3] on every axis: at least one cell inside the window of n points that starts at lo."""
    rows = v[t].reshape(-1, 3, 3)
    centre = rows.mean(axis=1)
    keep = np.ones(len(rows), bool)
    for a in range(3):
        cell = np.searchsorted(axes[a].astype(np.float64), centre[:, a], side="right") - 1
        keep &= (cell >= lo[a] + 1) & (cell <= lo[a] + n - 3)
    return rows[keep].reshape(-1, 9)


def test_a_lattice_the_dense_path_cannot_hold():
    """1400^3 = 2.7 G lattice points (the dense mesh step stops at 2^31; the dense state would be 22 GB): the sparse volume fuses
    the sphere scene's views there, and inside a window of 120^3 points its mesh is the mesh of a dense volume on that window,
    whose axes are slices of the same fp32 arrays and whose state is therefore the large lattice's state there.
    Recorded on an MI355X: 212 153 bricks, 4.0 % of the table, 0.89 GB of state; the window holds 59 793 interior triangles
    (estimate of the brick count from the pixel footprints beforehand: 1.5 - 2 x 10^5)."""
    n, w = 1400, 120
    h = 0.75 / (n - 1)
    views = [v._replace(image=None) for v in sphere_views()]
    big = FusionVolume(([-0.375] * 3, [0.375] * 3, h), trunc=4 * h, backend="device", device=DEV, sparse=True)
    assert big.shape == (n, n, n) and int(np.prod(big.shape, dtype=np.int64)) >= 2 ** 31
    big.integrate(views)
    assert big.finalize() is big and 0 < big.n_bricks * 512 < 2 ** 31
    print(f"1400^3: {big.n_bricks} bricks, allocated share {big.allocated_share():.4f}, state {big.state_bytes() / 1e9:.2f} GB")
    assert 100000 < big.n_bricks < 300000
    vb, tb = big.extract_mesh()
    # a patch of the sphere all four views see: towards (0.6, 0.1, -0.8)
    p = 0.3 * np.array([0.6, 0.1, -0.8]) / np.linalg.norm([0.6, 0.1, -0.8])
    lo = [int(round((p[a] + 0.375) / h)) - w // 2 for a in range(3)]
    axes = [big.axes_host[a][lo[a]:lo[a] + w] for a in range(3)]
    win = FusionVolume(axes, trunc=big.trunc, backend="device", device=DEV)
    win.integrate(views)
    assert float(win.weight.max()) == 4.0
    vw, tw = win.extract_mesh()
    got = interior_triangles(vb, tb, big.axes_host, lo, w)
    want = interior_triangles(vw, tw, big.axes_host, lo, w)
    print(f"window {lo}: {len(want)} interior triangles of {len(tw)}")
    assert len(want) > 500 and got.shape == want.shape
    # Both meshes list their triangles in ascending (x, y, z) cell order, so the rows correspond one to one.  A vertex is
    # axis[i] + (axis[i + 1] - axis[i]) * ((s + i) - i) with the same fp32 axis values and the same interpolation weight s in
    # float64; only the rounding of s + i differs with the size of the index i: at most 2^-43 (half an ulp of 1400) of a lattice
    # step of 5.4e-4, i.e. 6e-17, plus an ulp of the coordinate (5.6e-17 below 0.5) for the final sum.  Bound: 2e-16.
    assert float(np.abs(got - want).max()) <= 2e-16


def test_fuse_scene_script_sparse(tmp_path):
    """scripts/fuse_scene.py --sparse on the synthetic scene of tests/test_fusion_gpu.py::test_fuse_scene_script: the same PLY as
    without it, the new fields in the JSON line, and an early exit that names --sparse for a dense lattice past 2^31 points."""
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
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import fuse_scene
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--colors", "--logit_override", "sphere"]
    dense = fuse_scene.run(fuse_scene.parse_args(common + ["--resolution", "64", "--out_dir", str(tmp_path / "dense")]))
    state = {}
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--resolution", "64", "--sparse", "--out_dir", str(tmp_path / "sparse")]), state)
    assert open(rec["mesh"], "rb").read() == open(dense["mesh"], "rb").read() and rec["triangles"] == dense["triangles"] > 100
    assert rec["sparse"] is True and set(rec) - set(dense) == {"sparse", "bricks", "allocated_share", "state_bytes"}
    assert set(rec["ms"]) - set(dense["ms"]) == {"finalize"}
    vol = state["volume"]
    assert rec["bricks"] == vol.n_bricks > 0 and rec["allocated_share"] == vol.allocated_share() and 0.0 < rec["allocated_share"] < 1.0
    assert rec["state_bytes"] == vol.state_bytes() and rec["observed_share"] <= dense["observed_share"] and rec["lattice"] == dense["lattice"]
    assert json.load(open(tmp_path / "sparse" / "fused_scan24.json"))["bricks"] == rec["bricks"]
    with pytest.raises(SystemExit, match="--sparse"):
        fuse_scene.run(fuse_scene.parse_args(common + ["--resolution", "2048", "--out_dir", str(tmp_path / "big")]))
