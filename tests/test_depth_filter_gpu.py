"""GPU: csrc/depth_filter.hip against the host path of surf_amd.fusion (consistency_host / finish_host, the numpy-fp32 mirror of
the rule in depth_filter.hip's header comment) - equality, not tolerances - at ragged map sizes, across the 16-source launch
boundary and on degenerate geometry, plus the public interface above it: filter_views and scripts/fuse_scene.py --min_consistent."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import fusion, ops
from surf_amd.fusion import DepthView, FusionVolume
from tests.test_depth_filter_host import HOLES, ring_centres, sphere_ring, sphere_view

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 64                     # guard elements on either side of count / zsum: a write outside the map would land there


def guarded(shape, dtype, fill):
    """(the (H, W) tensor, its guarded flat buffer): the map is the middle of a buffer whose ends must keep `fill`."""
    n = shape[0] * shape[1]
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    buf[PAD:PAD + n] = 0
    return buf[PAD:PAD + n].view(shape), buf


def device_state(views, r, sources, splits=(), tile_w=None):
    """count, zsum of view r against `sources` from ops.depth_consistency: 16 sources per call, or cut at `splits`."""
    depths = [torch.from_numpy(np.ascontiguousarray(v.depth, dtype=np.float32)).to(DEV) for v in views]
    shape = tuple(depths[r].shape)
    (count, count_buf), (zsum, zsum_buf) = guarded(shape, torch.int32, -7), guarded(shape, torch.float32, -7.0)
    cuts = list(splits) + [len(sources)] if splits else list(range(16, len(sources), 16)) + [len(sources)]
    start = 0
    for end in cuts:
        ops.depth_consistency((depths[r], views[r].dscale),
                              [(fusion.pair_transforms(views[r], views[s]), depths[s], views[s].dscale) for s in sources[start:end]],
                              count, zsum, tile_w=tile_w)
        start = end
    n = shape[0] * shape[1]
    for buf in (count_buf, zsum_buf):
        assert bool((buf[:PAD] == -7).all()) and bool((buf[PAD + n:] == -7).all()), "a write outside the map"
    return count, zsum


def assert_equals_host(views, r, sources, count, zsum, min_consistent=2):
    """count / zsum and both finishes (plain, average) against the mirror."""
    h_count, h_zsum = fusion.consistency_host(views, r, sources)
    assert torch.equal(count.cpu(), torch.from_numpy(h_count)), int((count.cpu() != torch.from_numpy(h_count)).sum())
    assert torch.equal(zsum.cpu(), torch.from_numpy(h_zsum)), int((zsum.cpu() != torch.from_numpy(h_zsum)).sum())
    depth = torch.from_numpy(np.ascontiguousarray(views[r].depth, dtype=np.float32)).to(DEV)
    for average in (False, True):
        out, keep = ops.depth_consistency_finish((depth, views[r].dscale), count, zsum, min_consistent, average)
        h_out, h_keep = fusion.finish_host(views[r], h_count, h_zsum, min_consistent, average)
        assert out.dtype == torch.float32 and keep.dtype == torch.uint8
        assert torch.equal(out.cpu(), torch.from_numpy(h_out)), average
        assert torch.equal(keep.cpu(), torch.from_numpy(h_keep.astype(np.uint8))), average
    return h_count, h_zsum


def mixed_views():
    """Five views of the sphere, 37 x 53 and 24 x 40 (no side a multiple of 64; 37 x 53 = 7.66 blocks of 256, 2 x 5 tiles of
    32 x 8), focal lengths 48 to 85, one with dscale 2.5, each with holes of the four kinds sprinkled over 6 % of its pixels."""
    g = np.random.default_rng(21)
    spec = (((0.0, 2.0, -1.5), 75.0, 37, 53, 1.0), ((1.2, 1.9, -1.0), 48.0, 24, 40, 1.0), ((-1.0, 2.1, -0.9), 85.0, 37, 53, 2.5),
            ((0.6, 2.2, 1.0), 52.0, 24, 40, 1.0), ((-0.4, 1.2, -2.1), 70.0, 37, 53, 1.0))
    views = []
    for centre, f, H, W, dscale in spec:
        v = sphere_view(centre, f, H, W, dscale=dscale)
        depth = v.depth.copy()
        holes = g.random(depth.shape) < 0.06
        depth[holes] = g.choice(np.array(HOLES, dtype=np.float32), size=int(holes.sum()))
        views.append(v._replace(depth=depth))
    return views


def test_device_equals_host_on_mixed_views():
    views = mixed_views()
    kinds = np.concatenate([v.depth.reshape(-1) for v in views])
    assert (kinds == 0).any() and (kinds < 0).any() and np.isnan(kinds).any() and np.isinf(kinds).any()
    agreed = 0
    for r in range(len(views)):
        sources = [s for s in range(len(views)) if s != r]
        count, zsum = device_state(views, r, sources)
        h_count, _ = assert_equals_host(views, r, sources, count, zsum)
        agreed += int(h_count.sum())
        assert 0 < int((h_count >= 2).sum()) < int((views[r].depth > 0).sum())          # kept and rejected pixels both occur
        for tile_w in (64, 16, 8):                                                       # every thread-to-pixel mapping
            c, z = device_state(views, r, sources, tile_w=tile_w)
            assert torch.equal(c, count) and torch.equal(z, zsum), tile_w
    assert agreed > 3000
    # the public call, average off and on
    for average in (False, True):
        stats_d, stats_h = {}, {}
        dev = fusion.filter_views(views, 2, average=average, backend="device", device=DEV, stats=stats_d)
        host = fusion.filter_views(views, 2, average=average, backend="host", stats=stats_h)
        for v, d, h in zip(views, dev, host):
            assert d.depth.is_cuda and d.P is v.P and d.dscale == v.dscale
            assert torch.equal(d.depth.cpu(), torch.from_numpy(h.depth)), average
        assert stats_d["measured"] == stats_h["measured"] and stats_d["kept"] == stats_h["kept"]
        assert all(np.array_equal(a, b) for a, b in zip(stats_d["count_hist"], stats_h["count_hist"]))
    with pytest.raises(TypeError):
        ops.depth_consistency((torch.zeros(4, 4), 1.0), [], torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4))     # host tensors
    d = torch.zeros(4, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.depth_consistency((d, 1.0), [], torch.zeros(4, 5, dtype=torch.int32, device=DEV), torch.zeros(4, 4, device=DEV))
    with pytest.raises(ValueError, match="24"):
        ops.depth_consistency((d, 1.0), [(np.zeros(12, np.float32), d, 1.0)], torch.zeros(4, 4, dtype=torch.int32, device=DEV),
                              torch.zeros(4, 4, device=DEV))


def test_eighteen_sources_take_two_launches():
    views = [sphere_view(c, 24.0, 13, 17) for c in ring_centres(19)]
    sources = list(range(1, 19))
    assert len(sources) > ops.FUSE_MAX_VIEWS
    count, zsum = device_state(views, 0, sources)                                       # 16 + 2
    h_count, _ = assert_equals_host(views, 0, sources, count, zsum, min_consistent=3)
    assert int(h_count.max()) >= 8
    c, z = device_state(views, 0, sources, splits=(5,))                                 # 5 + 13
    assert torch.equal(c, count) and torch.equal(z, zsum)
    dev = fusion.filter_views(views, 3, backend="device", device=DEV)
    host = fusion.filter_views(views, 3, backend="host")
    assert all(torch.equal(d.depth.cpu(), torch.from_numpy(h.depth)) for d, h in zip(dev, host))
    from surf_amd import _lib
    depth = torch.from_numpy(views[0].depth).to(DEV)
    with pytest.raises(_lib.SurfHipError, match="limit"):
        ops.depth_consistency((depth, 1.0), [(fusion.pair_transforms(views[0], views[s]), depth, 1.0) for s in range(1, 18)],
                              torch.zeros(13, 17, dtype=torch.int32, device=DEV), torch.zeros(13, 17, device=DEV))


def aimed_view(centre, forward, f, H, W, depth):
    """A camera at `centre` whose optical axis is `forward`, with a constant depth map."""
    c, z = np.asarray(centre, np.float64), np.asarray(forward, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), c
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return DepthView((K @ np.linalg.inv(c2w)[:3, :4]).astype(np.float32), np.full((H, W), depth, np.float32), 1.0)


def test_degenerate_sources():
    ref, good = sphere_view((0.0, 2.0, -1.5), 75.0, 37, 53), sphere_view((1.0, 2.0, -1.1), 75.0, 37, 53)
    behind = aimed_view((0.0, 0.0, 3.0), (0.0, 0.0, 1.0), 60.0, 24, 40, 2.0)             # looks away: every point is behind it
    outside = aimed_view((0.0, 0.0, -2.5), (1.0, 0.0, 0.3), 300.0, 24, 40, 2.0)          # in front, far off its narrow image
    dot = aimed_view((0.0, 2.0, -1.5), (0.0, -2.0, 1.5), 75.0, 1, 1, 2.0)                # a 1 x 1 map: sx = sy = 0 or nothing
    views = [ref, good, behind, outside, dot]
    alone = fusion.consistency_host(views, 0, [1])[0]
    assert alone.sum() > 300
    for s in (2, 3, 4):
        count, zsum = device_state(views, 0, [s])
        h_count, _ = assert_equals_host(views, 0, [s], count, zsum, min_consistent=1)
        # the 1 x 1 map sits on the reference's own central ray: at most that one pixel can land on it
        assert h_count.sum() <= (1 if s == 4 else 0)
    for sources in ([1, 2, 3, 4], [4, 3, 2, 1], [2, 1]):
        count, zsum = device_state(views, 0, sources)
        h_count, _ = assert_equals_host(views, 0, sources, count, zsum, min_consistent=1)
        assert np.array_equal(h_count, alone + (fusion.consistency_host(views, 0, [4])[0] if 4 in sources else 0))
    # the 1 x 1 map as the reference: one thread, one pixel
    count, zsum = device_state(views, 4, [0, 1])
    assert_equals_host(views, 4, [0, 1], count, zsum, min_consistent=1)


def test_filtered_views_integrate_to_the_same_lattice():
    views = sphere_ring()
    g = np.random.default_rng(5)
    views = [v._replace(image=g.random(v.depth.shape + (3,)).astype(np.float32)) for v in views]
    axes = [np.linspace(-0.6, 0.6, 25, dtype=np.float32)] * 3
    vols = {}
    for backend in ("device", "host"):
        kept = fusion.filter_views(views, 2, backend=backend, device=DEV)
        vols[backend] = FusionVolume(axes, trunc=0.2, colors=True, backend=backend, device=DEV)
        vols[backend].integrate(kept)
    for k in ("tsdf", "weight", "color"):
        assert torch.equal(getattr(vols["device"], k).cpu(), torch.from_numpy(getattr(vols["host"], k))), k
    plain = FusionVolume(axes, trunc=0.2, backend="host")
    plain.integrate(views)
    assert 0.0 < vols["host"].observed_share() < plain.observed_share()


def test_fuse_scene_script_min_consistent(tmp_path):
    """scripts/fuse_scene.run on the synthetic DTU-format scene of tests/test_end_to_end_dtu.py: three reference views, with
    --min_consistent 1 and without."""
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
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "3", "--resolution", "64", "--logit_override", "sphere"]
    plain_state, state = {}, {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]), plain_state)
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--min_consistent", "1", "--out_dir", str(tmp_path / "out")]), state)
    # without the flag: exactly the record of before
    assert set(plain) == {"scan", "views_fused", "lattice", "voxel", "trunc", "observed_share", "vertices", "triangles", "depth",
                          "colors", "cleaned", "mesh", "ms"}
    assert set(plain["ms"]) == {"load", "lattice", "forward", "integrate", "extract", "write"}
    assert plain["views_fused"] == 3 and float(plain_state["volume"].weight.max()) == 3.0
    # with it
    assert set(rec) == set(plain) | {"min_consistent", "kept_share"} and set(rec["ms"]) == set(plain["ms"]) | {"filter"}
    assert rec["min_consistent"] == 1 and 0.0 < rec["kept_share"] <= 1.0 and rec["ms"]["filter"] > 0.0
    print(f"fuse_scene --min_consistent 1: kept share {rec['kept_share']:.3f}, observed share {rec['observed_share']:.3f} "
          f"(unfiltered {plain['observed_share']:.3f})")
    assert rec["views_fused"] == 3 and float(state["volume"].weight.max()) <= 3.0
    assert 0.0 < rec["observed_share"] <= plain["observed_share"]
    v, t = mesh_io.read_ply(rec["mesh"])
    assert len(v) == rec["vertices"] > 0 and len(t) == rec["triangles"] > 0 and np.isfinite(v).all()
    assert json.load(open(tmp_path / "out" / "fused_scan24.json"))["kept_share"] == rec["kept_share"]
