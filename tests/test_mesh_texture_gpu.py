"""GPU: csrc/mesh_texture.hip against the host mirror of surf_amd/mesh_texture.py - equal bits, not tolerances - on the scenes of
tests/mesh_texture_scenes.py at every view count and three atlas densities; launches of 16 + 16 + 1 views against the host's one
pass; 65,712 faces (more than 256 blocks of texels); the mesh depth maps against the float64 ray caster; repeatability; and the
--texture switch of scripts/fuse_scene.py and scripts/dtu_chamfer.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import mesh_io
from surf_amd import mesh_texture as MT
from tests import mesh_texture_scenes as S
from tests.mesh_denoise_scenes import BIG_CUBE, cube

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TS = (4, 5, 8)
# tests/test_raster_kernel.py's measured margins on its generic scenes and its factor: depths agree within FACTOR * E_Z relative, and
# a ray that passes within FACTOR * E_EDGE (as a barycentric) of an edge of a face may go either way
FACTOR, E_Z_GENERIC, E_EDGE_GENERIC = 8.0, 2.87e-06, 8.58e-05
UNDECIDED_CAP = 0.01
SETTINGS = {4: dict(power=4, two_sided=False, colours=False), 5: dict(power=1, two_sided=True, colours=True),
            8: dict(power=3, two_sided=False, colours=True)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def both(v, f, views, depths, T, power=4, two_sided=False, vc=None, **kw):
    out = {}
    for backend in ("host", "device"):
        st = {}
        res = MT.bake_texture(v, f, views, texels_per_edge=T, depth_tol=S.DEPTH_TOL, min_cos=S.MIN_COS, power=power,
                              two_sided=two_sided, vertex_colors=vc, mesh_depths=depths, backend=backend, device=DEV, stats=st,
                              return_sums=True, **kw)
        out[backend] = res + (st,)
    return out["host"], out["device"]


def assert_equal_bits(host, device):
    for name, a, b in zip(("uv", "atlas", "sum_rgb", "sum_w"), host, device):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        same = np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
        assert same, f"{name}: {int((a != b).sum())} of {a.size} entries differ"
    assert host[4] == device[4]                                     # the statistics, views_per_seen_texel included


@pytest.mark.parametrize("count", S.VIEW_COUNTS)
@pytest.mark.parametrize("name", sorted(S.scenes()))
def test_device_equals_host_in_bits(name, count):
    scene = S.scenes()[name]
    views, depths = S.views_of(name, count)
    for T in TS:
        s = SETTINGS[T]
        host, device = both(scene["vertices"], scene["faces"], views, depths, T, s["power"], s["two_sided"],
                            S.vertex_colours(name) if s["colours"] else None)
        assert_equal_bits(host, device)
        if name in S.GROUND_TRUTH and count >= 16:
            assert (host[3] > 0).any()                              # something is seen (the ten texels of one face at T = 4 may not be)


def test_chunking_is_invisible():
    """33 views in launches of 16 + 16 + 1, and of 7 at a time, against the host's single pass over the views."""
    from surf_amd import ops
    assert ops.FUSE_MAX_VIEWS == MT.MAX_VIEWS == 16
    scene = S.scenes()["cube8"]
    views, depths = S.views_of("cube8", 33)
    T = 5
    uv, atlas, sum_rgb, sum_w = MT.bake_texture(scene["vertices"], scene["faces"], views, texels_per_edge=T, depth_tol=S.DEPTH_TOL,
                                                min_cos=S.MIN_COS, mesh_depths=depths, return_sums=True)
    _, cols, rows, Ha, Wa = MT.atlas_layout(len(scene["faces"]), T)
    v, f = torch.from_numpy(scene["vertices"]).to(DEV), torch.from_numpy(scene["faces"]).to(DEV)
    packed = [(w.P.reshape(12), MT.view_centre(w.P), torch.from_numpy(w.image).to(DEV), torch.from_numpy(d).to(DEV))
              for w, d in zip(views, depths)]
    for chunk in (None, 7):
        a, sums, cnt = ops.bake_texture(v, f, packed, T, cols, rows, S.DEPTH_TOL, S.MIN_COS, chunk=chunk, count=True)
        sums = sums.cpu().numpy()
        assert np.array_equal(bits(sums[..., :3]), bits(sum_rgb)) and np.array_equal(bits(sums[..., 3]), bits(sum_w))
        assert np.array_equal(a.cpu().numpy(), atlas)
        assert int(cnt.max()) > 16                                  # some texel is seen from more views than one launch holds
    with pytest.raises(ValueError, match="chunk.*17"):
        ops.bake_texture(v, f, packed, T, cols, rows, S.DEPTH_TOL, chunk=17)


def test_many_blocks_of_texels():
    """cube(74): 65,712 faces, 657,120 texels at T = 4 - more than 256 blocks of 256 - from three views whose photographs are
    analytic (the brute-force renderer is for the small scenes) and whose depth maps come from mesh_depth_maps."""
    v, f = cube(BIG_CUBE)
    v = (v - np.float32(0.5)).astype(np.float32)
    assert len(f) == 65712 and MT.atlas_layout(len(f), 4)[3] * MT.atlas_layout(len(f), 4)[4] > 256 * 256
    views = []
    for k in range(3):
        P, (H, W) = S.cameras()[k]
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        image = np.stack([0.5 + 0.4 * np.sin(0.3 * x + k), 0.5 + 0.4 * np.cos(0.2 * y - k), 0.5 + 0.4 * np.sin(0.1 * (x + y))], axis=-1)
        views.append(MT.TextureView(P, image.astype(np.float32)))
    depths = [d.cpu().numpy() for d in MT.mesh_depth_maps(v, f, views, DEV)]
    assert all((d > 0).any() for d in depths)
    host, device = both(v, f, views, depths, 4)
    assert_equal_bits(host, device)
    assert host[4]["seen_share"] > 0.2


@pytest.mark.parametrize("name", ["cube8", "quads", "bad"])
def test_mesh_depth_maps_against_float64_ray_caster(name):
    """Per pixel: the same hit set and the depth within tests/test_raster_kernel.py's tolerance; the pixels whose ray passes
    within that test's edge tolerance of an edge of any face are left out, at most 1 % of them."""
    scene = S.scenes()[name]
    count = 6
    cams = S.cameras()[:count]
    maps = MT.mesh_depth_maps(scene["vertices"], scene["faces"], [(P, hw) for P, hw in cams], DEV)
    undecided = total = 0
    for k, got in enumerate(maps):
        cast = S.photograph(name, k)[2]
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == cams[k][1]
        clear = cast["edge"] > FACTOR * E_EDGE_GENERIC
        undecided, total = undecided + int((~clear).sum()), total + clear.size
        assert np.array_equal((got > 0)[clear], (cast["depth"] > 0)[clear])
        hit = clear & (cast["depth"] > 0)
        assert hit.any()
        rel = np.abs(got[hit].astype(np.float64) - cast["depth"][hit]) / cast["depth"][hit]
        assert rel.max() <= FACTOR * E_Z_GENERIC, rel.max()
    assert undecided / total <= UNDECIDED_CAP, undecided / total
    # given TextureViews, the same maps
    views, _ = S.views_of(name, 2)
    for a, b in zip(MT.mesh_depth_maps(scene["vertices"], scene["faces"], views, DEV), maps):
        assert torch.equal(a, b)


def test_run_twice_same_bits():
    scene = S.scenes()["quads"]
    views, _ = S.views_of("quads", 17)
    runs = []
    for _ in range(2):                                              # the whole device path, its own depth maps included
        runs.append(MT.bake_texture(scene["vertices"], scene["faces"], views, texels_per_edge=8, depth_tol=S.DEPTH_TOL, min_cos=S.MIN_COS,
                                    backend="device", device=DEV, return_sums=True))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (runs[0][3] > 0).any()


def test_device_path_needs_a_device():
    scene = S.scenes()["single"]
    with pytest.raises(RuntimeError, match="no host fall-back"):
        MT.bake_texture(scene["vertices"], scene["faces"], [], depth_tol=0.1, mesh_depths=[], backend="device", device="cpu")


# ---- the scripts ----

def _synthetic_conf(tmp_path):
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
    return conf_path, (H, W)


def _check_block(block, vertices, triangles, views, colours, params, obj_path):
    """The `texture` block against a recomputation with the host path, and the files it names."""
    depths = [d.cpu().numpy() for d in MT.mesh_depth_maps(vertices, triangles, views, DEV)]
    uv, atlas, want = MT.texture_step(vertices, triangles, views, params, backend="host", vertex_colors=colours, mesh_depths=depths)
    assert list(block) == ["texels_per_edge", "atlas", "faces", "texels_owned", "texels_seen", "seen_share", "faces_unseen",
                           "views_per_seen_texel", "views", "depth_tol", "min_cos", "power", "ms", "files"]
    assert {k: v for k, v in block.items() if k not in ("ms", "files")} == {k: v for k, v in want.items() if k != "ms"}
    assert block["texels_seen"] > 0 and block["views"] == len(views) and block["faces"] == len(triangles)
    stem = os.path.splitext(obj_path)[0]
    assert block["files"] == [stem + ".obj", stem + ".mtl", stem + ".png"]
    back = mesh_io.read_obj(block["files"][0])
    assert np.array_equal(back["vertices"], np.asarray(vertices, np.float32)) and np.array_equal(back["faces"], triangles)
    assert np.array_equal(back["uv"], uv) and np.array_equal(back["atlas"], atlas)
    return want


def test_fuse_scene_texture(tmp_path):
    """scripts/fuse_scene.run on the synthetic DTU-format scene with and without --texture: the switch adds the `texture` block and
    the three files; everything else - the record, the PLY - is byte for byte what it is without."""
    conf_path, _ = _synthetic_conf(tmp_path)
    import fuse_scene
    common = ["--conf", str(conf_path), "--scan", "24", "--ref_views", "1", "2", "--resolution", "64", "--colors", "--logit_override",
              "sphere", "--out_dir", str(tmp_path / "out")]
    plain = fuse_scene.run(fuse_scene.parse_args(common))
    plain_mesh = open(plain["mesh"], "rb").read()
    fused = tmp_path / "out" / "meshes" / "fused"
    assert "texture" not in plain and sorted(os.listdir(fused)) == ["scan24.ply"]
    state = {}
    rec = fuse_scene.run(fuse_scene.parse_args(common + ["--texture", "--texture_texels", "4"]), state)
    assert open(rec["mesh"], "rb").read() == plain_mesh
    assert set(rec) - set(plain) == {"texture"}
    strip = lambda r: {k: ({m: 0 for m in v} if k == "ms" else v) for k, v in r.items() if k != "texture"}      # noqa: E731
    assert json.dumps(strip(rec)) == json.dumps(strip(plain))
    assert sorted(os.listdir(fused)) == ["scan24.ply", "scan24_textured.mtl", "scan24_textured.obj", "scan24_textured.png"]
    assert len(state["texture_views"]) == 2 and state["texture_views"][0].image.shape == (96, 128, 3)
    params = {"texels_per_edge": 4, "depth_tol": 2.0 * rec["voxel"]}
    want = _check_block(rec["texture"], state["vertices"], state["triangles"], state["texture_views"], state["colors"], params,
                        str(fused / "scan24_textured.obj"))
    assert want["depth_tol"] == 2.0 * rec["voxel"] and json.load(open(tmp_path / "out" / "fused_scan24.json"))["texture"] == rec["texture"]
    print(f"fuse_scene --texture: {rec['texture']['faces']} faces, atlas {rec['texture']['atlas']}, seen share "
          f"{rec['texture']['seen_share']:.3f}, {rec['texture']['ms']:.1f} ms")


def test_dtu_chamfer_texture(tmp_path):
    """scripts/dtu_chamfer.run on the same scene with and without --texture: all three photographs of the item are baked into the
    world-frame mesh that is written; the record without the switch and the PLY are what they were."""
    from scipy.io import savemat
    from surf_amd import conf
    from surf_amd.datasets import get_loader
    conf_path, _ = _synthetic_conf(tmp_path)
    import dtu_chamfer
    # evaluation files that can be read, as in tests/test_end_to_end_dtu.py, but from the item alone: the mesh is a near-sphere of
    # radius 0.4 .. 0.9 in the normalised frame, so the "scan" is a thick shell of points there (the scores are not what is tested)
    dconf = conf.from_dict(json.loads(conf_path.read_text())["val_dataset"])
    item = next(iter(get_loader(dconf, "val", False, num_workers=0)[0]))
    S_mat = item["scale_mat"].double().numpy().reshape(4, 4)
    centre_w, scale = S_mat[:3, 3], float(np.linalg.norm(S_mat[:3, 0]))
    ev = tmp_path / "dtu_eval"
    os.makedirs(ev / "ObsMask")
    os.makedirs(ev / "Points" / "stl")
    rng = np.random.default_rng(0)
    shell = rng.normal(size=(60000, 3))
    stl = centre_w + scale * rng.uniform(0.4, 0.9, (60000, 1)) * shell / np.linalg.norm(shell, axis=1, keepdims=True)
    with open(ev / "Points" / "stl" / "stl024_total.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n").encode())
        f.write(np.ascontiguousarray(stl, dtype="<f4").tobytes())
    lo, hi = centre_w - 2 * scale, centre_w + 2 * scale
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8), "BB": np.stack([lo, hi]).astype(np.float32),
                                                  "Res": np.float32(4.0 * scale / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, -(lo[2] - 1.0)]])})       # everything is above it
    common = ["--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--mesh_resolution", "64",
              "--downsample_density", str(0.65 * scale / 60.0), "--max_dist", str(scale), "--logit_override", "sphere",
              "--eval_device", "gpu", "--vertex_colors"]
    plain = dtu_chamfer.run(dtu_chamfer.parse_args(common + ["--out_dir", str(tmp_path / "plain")]))
    state = {}
    rec = dtu_chamfer.run(dtu_chamfer.parse_args(common + ["--out_dir", str(tmp_path / "out"), "--texture", "--texture_texels", "4",
                                                           "--texture_power", "2"]), state)
    assert "texture" not in plain and set(rec) - set(plain) == {"texture"}
    assert open(rec["mesh"], "rb").read() == open(plain["mesh"], "rb").read()
    strip = lambda r: {k: v for k, v in r.items() if k not in ("texture", "seconds", "mesh")}                    # noqa: E731
    assert json.dumps(strip(rec)) == json.dumps(strip(plain))
    final = tmp_path / "out" / "meshes" / "final"
    assert sorted(os.listdir(final)) == ["scan24.ply", "scan24_textured.mtl", "scan24_textured.obj", "scan24_textured.png"]
    assert sorted(os.listdir(tmp_path / "plain" / "meshes" / "final")) == ["scan24.ply"]
    assert len(state["texture_views"]) == 3                          # the reference photograph and its two sources
    from surf_amd.fusion import similarity_scale
    step = similarity_scale(state["item"]["scale_mat"].numpy().reshape(4, 4)) * 2.0 / 63
    _, _, attrs = mesh_io.read_ply(rec["mesh"], attributes=True)
    _check_block(rec["texture"], state["world_vertices"], state["triangles"], state["texture_views"], attrs["colors"],
                 {"texels_per_edge": 4, "depth_tol": 2.0 * step, "power": 2}, str(final / "scan24_textured.obj"))
