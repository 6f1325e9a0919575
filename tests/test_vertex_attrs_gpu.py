"""Per-vertex mesh attributes on the GPU (ImplicitSurface.vertex_attributes, csrc/vertex_attrs.hip): normals = the SDF gradient
kernel's g / |g| and colours = the blend kernel's colour at the mesh vertices, against the CPU oracle; the two new stages bit for
bit against torch / a numpy fp32 mirror; chunking, the grey fallback, validate's switch and scripts/dtu_chamfer.py --vertex_colors.

Tolerances: the SDF gradient's of tests/test_hip_parity.py (1e-3 relative + 2e-4, on g before normalisation), the project's RGB
bound (1e-3 relative + 1e-5, tests/test_hip_parity.py's blend tests) and what follows from it for the quantised colour: at most one
uint8 level, and the same level wherever the oracle's c * 256 is further from a level boundary than that bound."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_vertex_attrs_host import (BOUNDARY_BAND, H, MAX_EXCLUDED, NV, ROOT, W, finish_mirror, make_model, make_scene_cpu,
                                          near_boundary, oracle_attributes, quantise)

pytestmark = pytest.mark.gpu

BMIN, BMAX = torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3)
RES = 64
PARENT_VALIDATE_KEYS = ["vertices", "triangles", "color_fine", "img_fine", "normal_img", "sdf_depth", "render_depth"]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def setup():
    """Model + scene on the device, the 64^3 mesh, its attributes (one launch) and the oracle's values at the same fp32 points:
    computed once, read by the tests below."""
    d = dev()
    model = make_model().to(d).eval()
    cpu = make_scene_cpu()
    scene = model.scene(cpu["mvol"].to(d), [v.to(d) for v in cpu["vols"]], [t.to(d) for t in cpu["tabs"]], None,
                        [f.to(d) for f in cpu["feats"]], cpu["imgs"].to(d), cpu["intrs"].to(d), cpu["c2ws"].to(d))
    v, t = model.extract_geometry(None, None, BMIN, BMAX, RES, 0.0, scene=scene)
    attrs = model.vertex_attributes(v, scene)
    pts = torch.from_numpy(v).float()
    g_ref, c_ref, n_ref = oracle_attributes(model, cpu, pts)
    return dict(model=model, scene=scene, cpu=cpu, v=v, t=t, attrs=attrs, pts=pts, g_ref=g_ref, c_ref=c_ref, n_ref=n_ref)


def test_attributes_match_the_oracle(setup):
    from surf_amd import ops
    s = setup
    v, a = s["v"], s["attrs"]
    V = len(v)
    assert v.dtype == np.float64 and 1000 <= V <= 10000, V
    assert a["normals"].dtype == np.float32 and a["normals"].shape == (V, 3)
    assert a["colors"].dtype == np.uint8 and a["colors"].shape == (V, 3)
    assert a["n_valid"].dtype == np.uint8 and a["n_valid"].shape == (V,)
    # n_valid: exactly the oracle's count; the mesh holds unseen, partly seen and fully seen vertices
    n_ref = s["n_ref"].numpy()
    assert np.array_equal(a["n_valid"].astype(np.int64), n_ref)
    assert (n_ref == 0).any() and (n_ref == NV - 1).any() and ((n_ref > 0) & (n_ref < NV - 1)).any()
    # normals: the gradient kernel's g at the same fp32 points within the SDF parity tolerance of the oracle's, and the returned
    # normals are that g through the finish stage
    d = dev()
    sdf_w, blend_w = s["model"].packed_weights(d)
    pts = s["pts"].to(d).contiguous()
    every = torch.arange(V, dtype=torch.int32, device=d)               # every vertex active, as vertex_attributes runs the kernels
    _, g = ops.sdf_mlp(pts, s["scene"].sv, sdf_w, active_idx=every)
    g = g.cpu()
    err = (g - s["g_ref"]).abs()
    print(f"V = {V}; max |g - g_oracle| = {float(err.max()):.3g} (|g| in [{float(s['g_ref'].norm(dim=1).min()):.3g}, "
          f"{float(s['g_ref'].norm(dim=1).max()):.3g}])")
    assert bool((err <= 2e-4 + 1e-3 * s["g_ref"].abs()).all()), float(err.max())
    col, nv = ops.blend(pts, s["scene"].feats_t4, s["scene"].imgs_t4, s["scene"].cams, blend_w, active_idx=every)
    n_m, c_m = finish_mirror(g.numpy(), col.cpu().numpy(), nv.cpu().numpy())
    assert np.array_equal(a["normals"], n_m) and np.array_equal(a["colors"], c_m)
    length = np.linalg.norm(a["normals"].astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() < 1e-6
    cos = (a["normals"].astype(np.float64) * (s["g_ref"] / s["g_ref"].norm(dim=1, keepdim=True)).double().numpy()).sum(1)
    assert cos.min() > 1.0 - 1e-5, cos.min()
    # colours, on the vertices a source view sees (the others: the grey fallback)
    seen = n_ref > 0
    assert (a["colors"][~seen] == 128).all()
    c_ref = s["c_ref"].numpy()
    excluded = near_boundary(c_ref) & seen
    share = float(excluded.sum()) / V
    keep = seen & ~excluded
    q_ref = quantise(c_ref)
    diff = np.abs(a["colors"].astype(np.int64) - q_ref.astype(np.int64))
    print(f"excluded share = {share:.3g}; levels off by one: {int((diff[keep] == 1).sum())} of {int(keep.sum()) * 3}; "
          f"max |c - c_oracle| = {float(np.abs(col.cpu().numpy() - c_ref)[seen].max()):.3g}")
    assert share <= MAX_EXCLUDED, share
    assert diff[keep].max() <= 1, int(diff[keep].max())
    # the RGB bound in level units, 256 (1e-3 |c| + 1e-5): further than that from a boundary the level is the oracle's
    lvl = c_ref.astype(np.float64) * 256.0
    margin = 256.0 * (1e-3 * np.abs(c_ref) + 1e-5) + BOUNDARY_BAND
    inner = np.clip(lvl, 0.0, 255.0)
    away = (np.minimum(inner - np.floor(inner), np.floor(inner) + 1.0 - inner) > margin) | (lvl < 1.0 - margin) | (lvl > 255.0 + margin)
    assert away[keep].mean() > 0.3
    assert (diff[keep][away[keep]] == 0).all()


def _special_rows():
    inf, nan = float("inf"), float("nan")
    g = np.array([[0, 0, 0], [-0.0, 0, 0], [1e-40, 0, 0], [1e-20, 1e-20, 0], [3e-39, -4e-39, 1e-42], [1e-30, 0, 0], [2.0 ** -40, 0, 0],
                  [inf, 0, 0], [0, -inf, 1], [nan, 1, 1], [1, 1, nan], [inf, nan, 0], [3e38, 3e38, 0], [1e19, 1e19, 1e19],
                  [3, 0, 4], [-1, 2, -2]], dtype=np.float32)
    c = np.array([[-0.5, 0.0, 0.5], [1.0, 1.5, 100.0], [-1e-30, 1e-40, 0.99999994], [0.00390624, 0.00390625, 0.00390626],
                  [0.99609375, 0.9960937, 0.996094], [nan, inf, -inf], [0.5, 0.5, 0.5], [255.0 / 256.0, 254.99999 / 256.0, 2.0]],
                 dtype=np.float32)
    return g, c


def test_finish_stage_is_bit_equal_to_the_numpy_mirror():
    from surf_amd import ops
    d = dev()
    rng = np.random.default_rng(4)
    gs, cs = _special_rows()
    n = 4099                                                            # 65 blocks, the last one partial
    g = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(-30, 30, (n, 1)))).astype(np.float32)
    c = rng.uniform(-0.25, 1.25, (n, 3)).astype(np.float32)
    k = rng.integers(0, 5, n).astype(np.uint8)
    # every special gradient row with every special colour row, seen (k = 1) and unseen (k = 0)
    gg = np.repeat(gs, len(cs), axis=0)
    cc = np.tile(cs, (len(gs), 1))
    g = np.concatenate([gg, gg, g])
    c = np.concatenate([cc, cc, c])
    k = np.concatenate([np.ones(len(gg), np.uint8), np.zeros(len(gg), np.uint8), k])
    assert (k == 0).sum() > len(gg) and np.isnan(g).any() and np.isinf(g).any() and (c < 0).any() and (c > 1).any()
    tiny = np.abs(g[np.isfinite(g) & (g != 0)])
    assert (tiny < np.finfo(np.float32).tiny).any()                     # denormal gradients
    normals, colors = ops.vertex_finish(torch.from_numpy(g).to(d), torch.from_numpy(c).to(d), torch.from_numpy(k).to(d))
    n_m, c_m = finish_mirror(g, c, k)
    assert normals.dtype == torch.float32 and colors.dtype == torch.uint8
    got_n, got_c = normals.cpu().numpy(), colors.cpu().numpy()
    bad = (got_n.view(np.uint32) != n_m.view(np.uint32)).any(axis=1)
    assert not bad.any(), (g[bad][:4], got_n[bad][:4], n_m[bad][:4])
    badc = (got_c != c_m).any(axis=1)
    assert not badc.any(), (c[badc][:4], k[badc][:4], got_c[badc][:4], c_m[badc][:4])
    assert not np.isnan(got_n).any()
    # the rules, on the device's output: zero rows for zero / non-finite gradients, grey for unseen rows
    zero = ~np.isfinite(g).all(axis=1) | (g == 0).all(axis=1)
    assert not got_n[zero].any() and (got_c[k == 0] == 128).all()
    # outputs written in place
    out_n = torch.full((len(g) + 2, 3), 7.0, device=d)
    out_c = torch.full((len(g) + 2, 3), 9, dtype=torch.uint8, device=d)
    ops.vertex_finish(torch.from_numpy(g).to(d), torch.from_numpy(c).to(d), torch.from_numpy(k).to(d), out_n[1:-1], out_c[1:-1])
    assert np.array_equal(out_n[1:-1].cpu().numpy().view(np.uint32), n_m.view(np.uint32)) and np.array_equal(out_c[1:-1].cpu().numpy(), c_m)
    assert bool((out_n[[0, -1]] == 7.0).all()) and bool((out_c[[0, -1]] == 9).all())      # nothing written past the rows


def test_point_stage_rounds_like_torch_float():
    from surf_amd import ops
    d = dev()
    rng = np.random.default_rng(6)
    for n in (1, 63, 64, 65, 4099):
        v = rng.uniform(-1, 1, (n, 3)) * np.exp(rng.uniform(-20, 5, (n, 1)))
        v[0, 0] = 1.0 + 2.0 ** -24                                      # a tie: rounds to even (1.0)
        if n > 1:
            v[1] = [1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24 + 2.0 ** -50), 0.1]
        pts, idx = ops.vertex_points(torch.from_numpy(v).to(d))
        assert pts.dtype == torch.float32 and idx.dtype == torch.int32 and pts.shape == (n, 3) and idx.shape == (n,)
        assert torch.equal(pts.cpu(), torch.from_numpy(v).float())
        assert torch.equal(idx.cpu(), torch.arange(n, dtype=torch.int32))
        v32 = v.astype(np.float32)
        p32, i32 = ops.vertex_points(torch.from_numpy(v32).to(d))
        assert np.array_equal(p32.cpu().numpy().view(np.uint32), v32.view(np.uint32))
        assert torch.equal(i32.cpu(), torch.arange(n, dtype=torch.int32))
    p0, i0 = ops.vertex_points(torch.zeros(0, 3, dtype=torch.float64, device=d))
    assert p0.shape == (0, 3) and i0.shape == (0,)
    with pytest.raises(TypeError):
        ops.vertex_points(torch.zeros(4, 3, dtype=torch.float16, device=d))


def _same(a, b):
    return all(a[k].dtype == b[k].dtype and np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8))
               for k in ("normals", "colors", "n_valid"))


def test_sizes_and_chunks(setup):
    s = setup
    model, scene, v = s["model"], s["scene"], s["v"]
    empty = model.vertex_attributes(np.zeros((0, 3)), scene)
    assert empty["normals"].shape == (0, 3) and empty["normals"].dtype == np.float32
    assert empty["colors"].shape == (0, 3) and empty["colors"].dtype == np.uint8
    assert empty["n_valid"].shape == (0,) and empty["n_valid"].dtype == np.uint8
    empty_t = model.vertex_attributes(torch.zeros(0, 3, device=dev()), scene)
    assert empty_t["normals"].shape == (0, 3) and empty_t["colors"].dtype == torch.uint8 and empty_t["n_valid"].shape == (0,)
    full = s["attrs"]
    pick = np.linspace(0, len(v) - 1, 257).astype(np.int64)             # spread over the mesh: every view count
    for n, chunk in ((1, None), (63, None), (64, None), (65, None), (257, 100), (257, 64), (65, 1), (257, 256)):
        rows = pick[:n]
        sub = np.ascontiguousarray(v[rows])
        one = model.vertex_attributes(sub, scene, chunk=1 << 20)        # a single launch of every stage
        got = model.vertex_attributes(sub, scene, chunk=chunk)
        assert _same(got, one), (n, chunk)
        assert _same(one, {k: full[k][rows] for k in full}), n          # ... and a row does not depend on its neighbours
    assert _same(model.vertex_attributes(v, scene, chunk=1000), full)   # ragged last chunk over the whole mesh
    # float32 vertices and device tensors: the same kernels on the same fp32 points
    f32 = model.vertex_attributes(v.astype(np.float32), scene)
    assert _same(f32, full)
    t = model.vertex_attributes(torch.from_numpy(v).to(dev()), scene, chunk=300)
    assert all(torch.is_tensor(t[k]) and t[k].is_cuda for k in t)
    assert _same({k: t[k].cpu().numpy() for k in t}, full)
    assert model.vertex_chunk_rows(dev(), NV) >= 256
    with pytest.raises(ValueError):
        model.vertex_attributes(v, scene, chunk=0)


def test_unseen_vertex_is_grey(setup):
    s = setup
    far = np.array([[0.0, 5.0, 0.0], [0.0, 0.0, -0.5], [0.0, -40.0, 0.3]])          # above / below every image; one in front of all
    _, _, n_ref = oracle_attributes(s["model"], s["cpu"], torch.from_numpy(far).float())
    assert n_ref.tolist() == [0, NV - 1, 0]
    a = s["model"].vertex_attributes(far, s["scene"])
    assert a["n_valid"].tolist() == [0, NV - 1, 0]
    assert a["colors"][0].tolist() == [128, 128, 128] and a["colors"][2].tolist() == [128, 128, 128]
    assert np.isfinite(a["normals"]).all()


def test_validate_switch(setup):
    from surf_amd import synthetic
    s = setup
    d = dev()
    model, scene, cpu = s["model"], s["scene"], s["cpu"]
    rays_o, rays_d = synthetic.pixel_rays(cpu["intrs"][0], cpu["c2ws"][0], H, W, 4, d)
    R = rays_o.shape[0]
    near = torch.full((R, 1), 0.95 * 1.5, device=d)
    far = torch.full((R, 1), 1.05 * 3.5, device=d)
    hw = (H // 4, W // 4)
    off = model.validate(rays_o, rays_d, near, far, scene, BMIN, BMAX, hw, mesh_resolution=RES)
    assert list(off) == PARENT_VALIDATE_KEYS
    on = model.validate(rays_o, rays_d, near, far, scene, BMIN, BMAX, hw, mesh_resolution=RES, vertex_attributes=True)
    assert list(on) == PARENT_VALIDATE_KEYS[:2] + ["vertex_normals", "vertex_colors", "vertex_n_valid"] + PARENT_VALIDATE_KEYS[2:]
    assert np.array_equal(off["vertices"], on["vertices"]) and np.array_equal(off["triangles"], on["triangles"])
    assert np.array_equal(off["vertices"], s["v"]) and np.array_equal(off["triangles"], s["t"])
    for k in PARENT_VALIDATE_KEYS[2:]:
        assert np.array_equal(np.asarray(off[k]), np.asarray(on[k])), k
    V = len(on["vertices"])
    assert on["vertex_normals"].shape == (V, 3) and on["vertex_colors"].shape == (V, 3) and on["vertex_n_valid"].shape == (V,)
    assert _same({"normals": on["vertex_normals"], "colors": on["vertex_colors"], "n_valid": on["vertex_n_valid"]}, s["attrs"])
    # no mesh, no attributes
    nomesh = model.validate(rays_o, rays_d, near, far, scene, BMIN, BMAX, hw, extract_geometry=False, vertex_attributes=True)
    assert list(nomesh) == PARENT_VALIDATE_KEYS[2:]


def test_dtu_chamfer_vertex_colors(tmp_path):
    """scripts/dtu_chamfer.py on the synthetic DTU-format scene of tests/test_end_to_end_dtu.py, without and with
    --vertex_colors: same positions, faces and Chamfer; the attributes in the PLY are vertex_attributes on the final vertex set
    (normals through scale_mat)."""
    from scipy.io import savemat
    from bench import surf_conf
    from surf_amd import conf, mesh_io
    from surf_amd.datasets import get_loader
    from tests.test_end_to_end_dtu import _write_scene
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    h, w = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, h, w)
    dconf = {"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
             "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [h, w],
             "total_views": 4}
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": surf_conf(base_dim=16), "val_dataset": dconf}, indent=1))
    # DTU evaluation files: a sphere around scale_mat's centre about where the initial surface lies
    loader, _, _ = get_loader(conf.from_dict(dconf), "val", False, num_workers=0)
    np.random.seed(0)
    S = next(iter(loader))["scale_mat"].double().numpy().reshape(4, 4)
    centre, r_world = S[:3, 3], 0.6 * float(np.linalg.norm(S[:3, 0]))
    density = r_world / 30.0
    ev = tmp_path / "dtu_eval"
    os.makedirs(ev / "ObsMask")
    os.makedirs(ev / "Points" / "stl")
    u = np.random.default_rng(1).standard_normal((20000, 3))
    stl = centre[None] + r_world * u / np.linalg.norm(u, axis=1, keepdims=True)
    with open(ev / "Points" / "stl" / "stl024_total.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n").encode())
        f.write(np.ascontiguousarray(stl, dtype="<f4").tobytes())
    lo, hi = centre - 2 * r_world, centre + 2 * r_world
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8), "BB": np.stack([lo, hi]).astype(np.float32),
                                                  "Res": np.float32(4.0 * r_world / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, -(lo[2] - 1.0)]])})
    base = ["--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--mesh_resolution", "64",
            "--downsample_density", str(density), "--max_dist", "1e6", "--logit_override", "sphere"]
    plain = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "plain")]))
    state = {}
    rec = dtu_chamfer.run(dtu_chamfer.parse_args(base + ["--out_dir", str(tmp_path / "coloured"), "--vertex_colors"]), state)
    assert rec["chamfer"] == plain["chamfer"] and rec["d2s"] == plain["d2s"] and rec["s2d"] == plain["s2d"]
    assert np.isfinite(rec["chamfer"]) and rec["vertices"] == plain["vertices"] and rec["triangles"] == plain["triangles"]
    assert "vertex_attributes" not in plain["seconds"] and rec["seconds"]["vertex_attributes"] > 0
    assert sorted(set(rec["seconds"]) - set(plain["seconds"])) == ["vertex_attributes"]
    v0, t0, a0 = mesh_io.read_ply(plain["mesh"], attributes=True)
    v1, t1, a1 = mesh_io.read_ply(rec["mesh"], attributes=True)
    assert a0 == {} and sorted(a1) == ["colors", "normals"]
    assert len(v1) > 500 and np.array_equal(v0, v1) and np.array_equal(t0, t1)
    ref = state["model"].vertex_attributes(state["vertices"])
    assert len(state["vertices"]) == len(v1)
    assert np.array_equal(a1["colors"], ref["colors"])
    assert np.array_equal(a1["normals"], mesh_io.transform_normals(ref["normals"], S))
    assert (ref["n_valid"] > 0).any() and len(np.unique(a1["colors"], axis=0)) > 10      # a coloured mesh, not a constant
    assert np.abs(np.linalg.norm(a1["normals"].astype(np.float64), axis=1) - 1.0).max() < 1e-5
