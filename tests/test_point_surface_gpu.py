"""csrc/point_surface.hip through surf_amd/point_surface.py, backend="device", against the numpy mirror (backend="host", itself pinned
by tests/test_point_surface_host.py): EQUAL arrays - bricks, table, tsdf, weight, colour - on the host tests' scenes, on
tests/point_filter_scenes.py's cloud with estimated normals, and with more candidates in one brick than an LDS tile holds; then the
methods PointSetVolume inherits (mesh, colours, simplification, ray casting) and scripts/fuse_scene.py --cloud_mesh."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import point_filter as PF
from surf_amd import point_surface as PS
from surf_amd.fusion import PointCloud
from tests import point_filter_scenes as F
from tests import point_surface_scenes as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 256                           # kThreads of point_surface.hip: raw candidates per staging step, half the LDS tile


def volumes(P, N, lat, radius, min_points=4, colors=None, alloc_reach=None):
    out = []
    for backend in ("device", "host"):
        vol = PS.PointSetVolume(lat.axes, radius, min_points, colors=colors is not None, backend=backend,
                                device=DEV if backend == "device" else None)
        vol._alloc_reach = alloc_reach
        out.append(vol.set_cloud(PointCloud(P, colors, None), N))
    return out


def assert_equal_state(dev, host):
    names = ("bricks", "table", "tsdf", "weight", "color")
    for name, d, h in zip(names, dev.finalize()._state, host.finalize()._state):
        if h is None:
            assert d is None, name
            continue
        d = d.cpu().numpy()
        assert d.dtype == h.dtype and d.shape == h.shape, name
        assert np.array_equal(d, h), (name, int((d != h).sum()), d.size)


# ---- 6. device equals host ----

@pytest.mark.parametrize("where", list(S.CENTRES))
@pytest.mark.parametrize("rv", (2.5, 4.0))
def test_sphere_device_equals_host(where, rv):
    P, N, lat = S.sphere_scene(where)
    col = np.random.default_rng(3).integers(0, 256, P.shape).astype(np.uint8)
    dev, host = volumes(P, N, lat, rv * lat.voxel, colors=col)
    assert_equal_state(dev, host)
    assert dev.n_bricks == 27 and float((dev.weight > 0).sum()) > 1000
    cs, hs = dev.cloud_stats(), host.cloud_stats()
    assert cs == hs, (cs, hs)


def test_plane_device_equals_host():
    P, N, lat = S.plane_scene()
    assert_equal_state(*volumes(P, N, lat, 3.0 * lat.voxel))


def rule_edge_scenes():
    P, N, lat = S.sphere_scene("origin")
    bad_p = np.array([[np.nan, 0, 0], [0.1, np.inf, 0], [0, 0, 0.4], [0, 0.4, 0], [0.4, 0, 0]], np.float32)
    bad_n = np.array([[0, 0, 1], [0, 1, 0], [np.nan, 0, 1], [0, -np.inf, 0], [0, 0, 0]], np.float32)
    at = np.array([0, 300, 300, 700, 1000])
    yield "bad_rows", np.insert(P, at, bad_p, axis=0), np.insert(N, at, bad_n, axis=0), lat, 2.5, 4
    yield "duplicates", np.concatenate([P, P]), np.concatenate([N, N]), lat, 2.5, 4
    for mp in (5, 6, 7):
        yield f"min_points_{mp}", P, N, lat, 2.5, mp
    grid = S.lattice((0, 0, 0), (0.75, 0.75, 0.75), 2.0 ** -5)
    yield "exactly_R", np.array([[8, 8, 8]], np.float32) * np.float32(2.0 ** -5), np.array([[0, 0, 1]], np.float32), grid, 3.0, 1
    unit = S.lattice((0, 0, 0), (1.0, 1.0, 1.0), 1.0 / 20)
    v = unit.voxel
    Q = np.array([[-1.5 * v, 0.5, 0.5], [-9.5 * v, 0.5, 0.5], [0.5, 1.0 + 12 * v, 0.5], [0.3, 0.3, 0.3], [1e30, 0.0, -1e30]], np.float32)
    yield "outside", Q, np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (5, 1)), unit, 3.0, 1
    v = 1.56 / 22
    lo = np.array([-0.68, -0.78, -0.88])
    yield "ragged", P, N, S.lattice(lo, lo + v * np.array([20, 22, 25]), v), 2.5, 4
    yield "ring_2", P, N, S.sphere_scene("origin", 25)[2], 9.0, 4
    yield "empty", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), lat, 2.5, 1
    yield "one_point", np.array([[0.01, 0.02, 0.03]], np.float32), np.array([[0.6, 0.0, 0.8]], np.float32), lat, 2.5, 1
    yield "blanket", P, N, S.sphere_scene("origin", 45)[2], 2.5, 4


@pytest.mark.parametrize("case", [c[0] for c in rule_edge_scenes()])
def test_rule_edges_device_equal_host(case):
    _, P, N, lat, rv, mp = next(c for c in rule_edge_scenes() if c[0] == case)
    dev, host = volumes(P, N, lat, rv * lat.voxel, mp, alloc_reach=8.0 if case == "blanket" else None)
    assert_equal_state(dev, host)
    if case == "ragged":
        assert lat.shape == (21, 23, 26)
    if case == "empty":
        assert dev.n_bricks == 0 and dev.extract_mesh()[0].shape == (0, 3)


@functools.lru_cache(maxsize=None)
def filter_cloud(where):
    """tests/point_filter_scenes.py's cloud with its estimate_normals normals (starved points: (0, 0, 0)) and random colours, on a
    lattice of voxel 0.01 (the plane's spacing) over the plane and the sphere; the outliers and the far pair lie outside it."""
    scene = F.build(0, S.CENTRES[where])
    N = PF.estimate_normals(scene.points, None, k=16, max_dist=0.05, backend="device", device=DEV)
    col = np.random.default_rng(7).integers(0, 256, scene.points.shape).astype(np.uint8)
    c = np.asarray(S.CENTRES[where], np.float64)
    return scene.points, N, col, S.lattice(c + (-0.05, -0.05, -0.1), c + (0.55, 0.45, 0.45), 0.01)


@pytest.mark.parametrize("where", list(S.CENTRES))
def test_filter_cloud_device_equals_host(where):
    P, N, col, lat = filter_cloud(where)
    assert (~N.any(axis=1)).sum() > 0                                 # some points are starved: they take no part
    dev, host = volumes(P, N, lat, 3.0 * lat.voxel, colors=col)
    assert_equal_state(dev, host)
    assert dev.n_bricks > 50 and float((dev.weight > 0).sum()) > 8000


@pytest.mark.parametrize("n", (3000, 2 * TILE, TILE, TILE + 1))
def test_more_candidates_than_a_tile_in_one_brick(n):
    """n points inside ONE brick of a 24^3 lattice: the centre brick and its 26 neighbours all run through n candidates, more than
    the LDS tile holds (3000), exact multiples of the staging step (512, 256) and one more (257)."""
    lat = S.lattice((0, 0, 0), (23.0, 23.0, 23.0), 1.0)
    g = np.random.default_rng(n)
    P = g.uniform(8.5, 14.5, (n, 3)).astype(np.float32)
    N = g.normal(size=(n, 3)).astype(np.float32)
    col = g.integers(0, 256, (n, 3)).astype(np.uint8)
    dev, host = volumes(P, N, lat, 3.0, colors=col)
    assert_equal_state(dev, host)
    assert dev.cloud_stats()["candidates_max"] == n and dev.n_bricks == 27


def test_two_runs_are_bit_equal():
    P, N, col, lat = filter_cloud("world")
    a, b = (PS.PointSetVolume(lat.axes, 3.0 * lat.voxel, colors=True, device=DEV).set_cloud(PointCloud(P, col, None), N).finalize()
            for _ in range(2))
    for x, y in zip(a._state, b._state):
        assert torch.equal(x, y)


# ---- 7. the inherited methods ----

def euler(v, t):
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return len(v) - len(np.unique(e, axis=0)) + len(t)


def components(nv, t):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])
    return connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)[0]


@pytest.mark.parametrize("rv", (2.5, 4.0))
def test_sphere_mesh_is_closed_and_near_the_sphere(rv):
    P, N, lat = S.sphere_scene("origin")
    R = rv * lat.voxel
    col = np.tile(np.array([[200, 17, 96]], np.uint8), (len(P), 1))
    dev = volumes(P, N, lat, R, colors=col)[0]
    v, t, c = dev.extract_mesh()
    assert v.dtype == np.float64 and t.dtype == np.int64 and len(v) > 500
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key, rev = e[:, 0] * len(v) + e[:, 1], e[:, 1] * len(v) + e[:, 0]
    assert len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))      # closed and oriented
    assert euler(v, t) == 2 and components(len(v), t) == 1                                      # one genus-0 component
    off = np.abs(np.linalg.norm(v, axis=1) - S.SPHERE_R)
    print(f"sphere mesh R = {rv} voxels: {len(v)} vertices, worst {off.max() / lat.voxel:.3f} voxel off the sphere")
    assert off.max() <= R * R / (2 * S.SPHERE_R) + lat.voxel
    assert (c == np.array([200, 17, 96], np.uint8)).all()            # one colour in, exactly that colour on every vertex
    # ... and oriented one way all over: every triangle's normal on the same side of the sphere's radius
    nrm = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert abs(np.sign((nrm * v[t].mean(axis=1)).sum(axis=1)).mean()) > 0.99


def test_mesh_does_not_depend_on_the_allocation():
    P, N, lat = S.sphere_scene("origin", 45)
    tight = volumes(P, N, lat, 2.5 * lat.voxel)[0]
    blanket = volumes(P, N, lat, 2.5 * lat.voxel, alloc_reach=8.0)[0]
    assert tight.n_bricks < blanket.n_bricks
    for a, b in zip(tight.extract_mesh(), blanket.extract_mesh()):
        assert np.array_equal(a, b)


def test_plane_mesh_simplify_and_ray_cast():
    """The plane of the host test: the mesh lies on z = 0.125 to the worst node's rounding bound, (2 m + 2) 2^-24 |z - 0.125| with
    |z - 0.125| < R - a vertex is interpolated between two such nodes; simplify_cell and ray_cast run on the volume, and a camera
    looking straight down at the plane from z = 1 sees it at depth 0.875 within one voxel."""
    P, N, lat = S.plane_scene()
    R = 3.0 * lat.voxel
    dev, host = volumes(P, N, lat, R)
    v, t = dev.extract_mesh()
    assert len(t) > 1000
    m = float(dev.weight.max())
    assert np.abs(v[:, 2] - 0.125).max() <= (2 * m + 2) * 2.0 ** -24 * R
    vs, ts = dev.extract_mesh(simplify_cell=4 * lat.voxel)
    assert 0 < len(ts) < len(t) / 4 and np.abs(vs[:, 2] - 0.125).max() < 1e-6
    K = np.array([[40.0, 0, 15.5], [0, 40.0, 15.5], [0, 0, 1]])
    Rw2c = np.diag([1.0, -1.0, -1.0])
    Pm = K @ np.concatenate([Rw2c, (-Rw2c @ np.array([0.5, 0.5, 1.0]))[:, None]], axis=1)
    cast, cast_h = dev.ray_cast(Pm, (32, 32)), host.ray_cast(Pm, (32, 32))
    hit = cast["depth"] > 0
    assert hit.mean() > 0.95 and np.abs(cast["depth"][hit] - 0.875).max() <= lat.voxel
    assert (cast["normal"][hit][:, 2] > 0.99).all()
    assert np.array_equal(cast["depth"], cast_h["depth"]) and np.array_equal(cast["normal"], cast_h["normal"])


def test_reconstruct_equals_the_class_path():
    P, N, lat = S.sphere_scene("world")
    col = np.random.default_rng(3).integers(0, 256, P.shape).astype(np.uint8)
    cloud = PointCloud(P, col, None)
    R = 3.0 * lat.voxel
    lo, hi = PS.cloud_bounds(P, N, R)
    assert np.allclose(lo, P.min(axis=0) - R) and np.allclose(hi, P.max(axis=0) + R)
    st = {}
    got = PS.reconstruct(cloud, N, lat.voxel, device=DEV, stats=st)
    vol = PS.PointSetVolume((lo, hi, lat.voxel), R, colors=True, device=DEV).set_cloud(cloud, N)
    want = vol.extract_mesh()
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert st["points"] == 1000 and st["bricks"] == vol.n_bricks and st["vertices"] == len(want[0]) and st["faces"] == len(want[1])
    assert st["allocated_share"] == vol.allocated_share() and st["candidates_max"] > 0
    # without colours, simplified, on the host backend: the same entry point
    plain = PS.reconstruct(P, N, lat.voxel, device=DEV)
    assert len(plain) == 2 and np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
    small = PS.reconstruct(cloud, N, lat.voxel, simplify_cell=3 * lat.voxel, device=DEV)
    assert 0 < len(small[1]) < len(want[1]) and small[2].shape == (len(small[0]), 3)
    host = PS.reconstruct(cloud, N, lat.voxel, backend="host", device=DEV)
    assert all(np.array_equal(a, b) for a, b in zip(host, want))
    vol = PS.PointSetVolume((lo, hi, lat.voxel), R, device=DEV)
    with pytest.raises(TypeError):
        vol.integrate([])
    with pytest.raises(ValueError):
        vol.extract_mesh()                                            # no cloud yet


# ---- 8. the script ----

def test_fuse_scene_cloud_mesh(tmp_path):
    """scripts/fuse_scene.py --point_cloud --cloud_normals 16 --cloud_mesh on the synthetic DTU-format scene: <scan>_cloud_mesh.ply and
    the `cloud_mesh` record; without the flag the record and the files are what they were."""
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
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "3", "--resolution", "64", "--logit_override", "sphere",
              "--min_consistent", "1", "--colors", "--point_cloud", "--cloud_normals", "16"]
    s1 = {}
    plain = fuse_scene.run(fuse_scene.parse_args(common + ["--out_dir", str(tmp_path / "plain")]))
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--cloud_mesh", "--cloud_mesh_radius", "3.5", "--cloud_mesh_min_points", "3",
                                                         "--out_dir", str(tmp_path / "out")]), s1)
    assert set(rec) == set(plain) | {"cloud_mesh"}
    for k in ("scan", "views_fused", "lattice", "voxel", "trunc", "depth", "colors", "cleaned", "min_consistent"):
        assert rec[k] == plain[k], k
    assert not os.path.exists(tmp_path / "plain" / "meshes" / "fused" / "scan24_cloud_mesh.ply")
    cm = rec["cloud_mesh"]
    assert set(cm) == {"radius", "min_points", "points", "bricks", "allocated_share", "vertices", "faces", "file", "ms"}
    assert cm["radius"] == pytest.approx(3.5 * rec["voxel"]) and cm["min_points"] == 3 and cm["ms"] > 0
    assert 0 < cm["points"] <= rec["points"] and cm["bricks"] > 0 and 0 < cm["allocated_share"] <= 1
    assert cm["file"].endswith("scan24_cloud_mesh.ply")
    v, t, attrs = mesh_io.read_ply(cm["file"], attributes=True)
    assert len(v) == cm["vertices"] > 0 and len(t) == cm["faces"] > 0 and attrs["colors"].shape == (len(v), 3)
    # the file holds the mesh the library returned, and that mesh lies in the cloud: every vertex within the radius of a point
    want = s1["cloud_mesh"]
    assert np.allclose(want[0], v, atol=1e-4 * rec["voxel"]) and np.array_equal(want[1], t) and np.array_equal(want[2], attrs["colors"])
    from scipy.spatial import cKDTree
    assert cKDTree(s1["cloud"].points.astype(np.float64)).query(v)[0].max() < cm["radius"]
    for flags in (common[:-3] + ["--cloud_normals", "16", "--cloud_mesh"], common[:-2] + ["--cloud_mesh"]):
        with pytest.raises(SystemExit):
            fuse_scene.run(fuse_scene.parse_args(flags + ["--out_dir", str(tmp_path / "bad")]))
    print(f"fuse_scene --cloud_mesh: {cm['points']} points -> {cm['bricks']} bricks ({100 * cm['allocated_share']:.1f} %), "
          f"{cm['vertices']} vertices, {cm['faces']} faces in {cm['ms']:.1f} ms")
