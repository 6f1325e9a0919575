"""Narrow-band mesh extraction (render.mesh_extraction = band, csrc/mesh_band.hip): the SDF only in 8^3-cell bricks near the
surface, and the same vertex / triangle arrays as the dense lattice sweep, in the same order."""
import numpy as np
import pytest
import torch

from tests.golden_cfg import CFG, pipeline_views

N_SAMPLES = [64, 32, 16, 16]
BMIN, BMAX = torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3)


def _model(precision="bf16x3", **render):
    from bench import model_conf
    from surf_amd.implicit_surface import ImplicitSurface
    conf = model_conf(N_SAMPLES, precision)
    for k, v in render.items():
        conf["render"][k] = v
    torch.manual_seed(0)
    return ImplicitSurface(conf)


@pytest.fixture(scope="module")
def bench_scene():
    """The bench scene: random-init network (geometric init, a sphere of radius ~0.5) on synthetic.sphere_pyramid(88)."""
    from surf_amd import synthetic
    from surf_amd.implicit_surface import _LatticeScene
    dev = torch.device("cuda:0")
    vols, tabs, _ = synthetic.sphere_pyramid(88, dev)
    return _LatticeScene(vols[::-1], tabs[::-1])


@pytest.fixture(scope="module")
def bench_models():
    return {p: _model(p).to("cuda:0") for p in ("f32", "bf16x3", "f16x2")}


def _golden_model(weights, noise=0.0):
    from surf_amd.implicit_surface import ImplicitSurface
    from bench import model_conf
    model = ImplicitSurface(model_conf(CFG["n_samples"]))
    sd = {k[len("implicit_surface."):]: v for k, v in weights.items() if k.startswith("implicit_surface.")}
    model.load_state_dict(sd, strict=True)
    if noise:
        g = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for p in model.sdf_network.parameters():
                p.add_(noise * float(p.std()) * torch.randn(p.shape, generator=g))
    return model.to("cuda:0")


@pytest.fixture(scope="module")
def golden_scene(golden_pipe):
    from surf_amd.implicit_surface import _LatticeScene
    vols, tabs, _, _ = pipeline_views(golden_pipe)
    return _LatticeScene([v.cuda() for v in vols], [t.cuda() for t in tabs])


def _components(t, nv):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if nv == 0:
        return 0
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])
    n, _ = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(nv, nv)), directed=False)
    return n


@pytest.fixture(scope="module")
def noisy_golden(weights, golden_grid, golden_scene):
    """The golden network with seeded noise on the SDF weights: the smallest of a fixed list of noise levels that breaks the
    512^3 mesh into several components."""
    for noise in (0.1, 0.2, 0.4, 0.8):
        model = _golden_model(weights, noise)
        v, t = model.extract_geometry(None, None, golden_grid["bound_min"], golden_grid["bound_max"], 128, 0.0, scene=golden_scene)
        if _components(t, len(v)) > 1:
            return model
    raise AssertionError("no noise level of the list splits the golden surface")


def _extract(model, scene, res, mode, bmin=BMIN, bmax=BMAX):
    v, t = model.extract_geometry(None, None, bmin, bmax, res, 0.0, scene=scene, mesh_extraction=mode)
    return v, t


def _assert_same(a, b):
    assert a[0].dtype == b[0].dtype == np.float64 and a[1].dtype == b[1].dtype == np.int64
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, (a[0].shape, b[0].shape, a[1].shape, b[1].shape)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])


def _band_equals_dense(model, scene, res, bmin, bmax, coords, values):
    """every band value (torch.equal) equals the dense lattice value at its point"""
    u = model.sdf_grid(scene, bmin, bmax, res)
    loc = torch.arange(512, device=u.device)
    g = coords.long()[:, None, :] * 8 + torch.stack([loc >> 6, (loc >> 3) & 7, loc & 7], dim=1)[None]
    ok = (g < res).all(dim=2)
    g = g.clamp(max=res - 1)
    dense = u[g[..., 0], g[..., 1], g[..., 2]]
    assert torch.equal(values[ok], dense[ok])
    assert bool(torch.isnan(values[~ok]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16x3", "f16x2"])
def test_band_mesh_equals_dense_on_bench_scene(bench_models, bench_scene, precision):
    m = bench_models[precision]
    dense = _extract(m, bench_scene, 512, "dense")
    band = _extract(m, bench_scene, 512, "band")
    assert len(dense[0]) > 100_000
    _assert_same(band, dense)


@pytest.mark.gpu
def test_band_mesh_equals_dense_on_golden_and_noisy_networks(weights, golden_grid, golden_scene, noisy_golden):
    bmin, bmax = golden_grid["bound_min"], golden_grid["bound_max"]
    for model in (_golden_model(weights), noisy_golden):
        dense = model.extract_geometry(None, None, bmin, bmax, 512, 0.0, scene=golden_scene, mesh_extraction="dense")
        band = model.extract_geometry(None, None, bmin, bmax, 512, 0.0, scene=golden_scene, mesh_extraction="band")
        assert len(dense[1]) > 1000
        _assert_same(band, dense)
    assert _components(dense[1], len(dense[0])) > 1


@pytest.mark.gpu
def test_band_mesh_equals_dense_at_1024(bench_models, bench_scene):
    m = bench_models["bf16x3"]
    dense = _extract(m, bench_scene, 1024, "dense")
    band = _extract(m, bench_scene, 1024, "band")
    _assert_same(band, dense)


@pytest.mark.gpu
def test_band_values_are_the_dense_lattice_values(bench_models, bench_scene, golden_grid, golden_scene, noisy_golden):
    for precision in ("bf16x3", "f32"):
        m = bench_models[precision]
        coords, values, stats = m.sdf_band(bench_scene, BMIN, BMAX, 512)
        assert coords.shape == (stats["bricks_evaluated"], 3) and values.shape == (stats["bricks_evaluated"], 512)
        # a few per cent of the lattice
        assert stats["band_points"] < 0.1 * 512 ** 3 and stats["points_evaluated"] == stats["band_points"] + 65 ** 3
        _band_equals_dense(m, bench_scene, 512, BMIN, BMAX, coords, values)
    bmin, bmax = golden_grid["bound_min"], golden_grid["bound_max"]
    coords, values, _ = noisy_golden.sdf_band(golden_scene, bmin, bmax, 512)
    _band_equals_dense(noisy_golden, golden_scene, 512, bmin, bmax, coords, values)


@pytest.mark.gpu
def test_band_growth_from_sign_change_seeds_only(bench_models, bench_scene):
    m = bench_models["bf16x3"]
    _, _, stats = m.sdf_band(bench_scene, BMIN, BMAX, 512, margin=0.0)
    assert stats["growth_iterations"] > 1 and stats["bricks_grown"] > 0, stats
    saved = m.mesh_band_margin
    try:
        m.mesh_band_margin = 0.0
        band = _extract(m, bench_scene, 512, "band")
    finally:
        m.mesh_band_margin = saved
    _assert_same(band, _extract(m, bench_scene, 512, "dense"))


@pytest.mark.gpu
@pytest.mark.parametrize("res,bmin,bmax", [
    (9, BMIN, BMAX), (100, BMIN, BMAX), (513, BMIN, BMAX),
    (100, BMIN, torch.tensor([1.0, 1.0, 0.0])), (257, BMIN, torch.tensor([1.0, 1.0, 0.0])),
    (64, torch.tensor([-0.3] * 3), torch.tensor([0.3] * 3)),
])
def test_band_edges(bench_models, bench_scene, res, bmin, bmax):
    m = bench_models["bf16x3"]
    dense = _extract(m, bench_scene, res, "dense", bmin, bmax)
    band = _extract(m, bench_scene, res, "band", bmin, bmax)
    _assert_same(band, dense)
    if float(bmax[0]) == 0.3:
        assert len(band[0]) == 0 and len(band[1]) == 0       # inside the sphere: no surface, no error
    elif float(bmax[2]) == 0.0:
        assert float(band[0][:, 2].max()) == 0.0              # the mesh reaches the cut face of the box
    elif res > 9:
        assert len(band[1]) > 100


@pytest.mark.gpu
def test_band_at_2048_cubed(bench_models, bench_scene):
    """Beyond the dense path's 2^31-point limit: closed, oriented, Euler characteristic of the 512 mesh, 16x its vertices."""
    from surf_amd import ops
    m = bench_models["bf16x3"]
    v512, t512 = _extract(m, bench_scene, 512, "band")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    v, t = _extract(m, bench_scene, 2048, "band")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < 8 * 2 ** 30, peak                                  # bound of this test: 8 GiB (the dense lattice alone: 32 GiB)
    nv, nt = len(v), len(t)
    assert 0.9 * 16 < nv / len(v512) < 1.1 * 16
    tl = torch.from_numpy(t).cuda()
    e = torch.cat([tl[:, [0, 1]], tl[:, [1, 2]], tl[:, [2, 0]]])
    key = e[:, 0] * nv + e[:, 1]
    rev = e[:, 1] * nv + e[:, 0]
    assert torch.unique(key).numel() == key.numel()                     # every directed edge once
    assert torch.equal(torch.sort(key).values, torch.sort(rev).values)  # ... and its reverse too: closed, oriented
    assert nv - (3 * nt) // 2 + nt == len(v512) - (3 * len(t512)) // 2 + len(t512)
    del tl, e, key, rev
    # the band values of one x-slab against the lattice kernel on that slab
    coords, values, _ = m.sdf_band(bench_scene, BMIN, BMAX, 2048)
    axes = m._lattice_axes(BMIN, BMAX, 2048, torch.device("cuda:0"))
    bx = 128
    x0 = 8 * bx
    slab = torch.empty(8, 2048, 2048, dtype=torch.float32, device="cuda:0")
    w, _ = m.packed_weights(torch.device("cuda:0"))
    ops.sdf_lattice([axes[0][x0:x0 + 8].contiguous(), axes[1], axes[2]], bench_scene.sv, w, slab, 0, 8, sign=-1.0)
    sel = coords[:, 0] == bx
    assert int(sel.sum()) > 100
    c, vals = coords[sel].long(), values[sel]
    loc = torch.arange(512, device=c.device)
    g = c[:, None, :] * 8 + torch.stack([loc >> 6, (loc >> 3) & 7, loc & 7], dim=1)[None]
    assert torch.equal(vals, slab[g[..., 0] - x0, g[..., 1], g[..., 2]])


@pytest.mark.gpu
def test_band_is_deterministic(bench_models, bench_scene):
    m = bench_models["f16x2"]
    _assert_same(_extract(m, bench_scene, 512, "band"), _extract(m, bench_scene, 512, "band"))


@pytest.mark.gpu
def test_surf_validate_with_band_extraction():
    """SuRF.forward("val") with render.mesh_extraction = band: the default model's mesh and images."""
    from bench import surf_conf
    from surf_amd import conf, synthetic
    from surf_amd.surf import SuRF
    dev = torch.device("cuda:0")
    H, W, nv = 120, 160, 3
    outs = []
    for mode in (None, "band"):
        mc = surf_conf(32)
        if mode is not None:
            mc["implicit_surface"]["render"]["mesh_extraction"] = mode
        torch.manual_seed(0)
        model = SuRF(conf.from_dict(mc)).eval().to(dev)
        model.logit_override = synthetic.sphere_logit
        assert model.implicit_surface.mesh_extraction == (mode or "dense")
        intrs, c2ws, near_fars = synthetic.ring_cameras(nv, H, W)
        rays_o, rays_d = synthetic.pixel_rays(intrs[0], c2ws[0], H, W, 1, dev)
        ipts = {"imgs": synthetic.procedural_images(nv, H, W, 0, dev), "intrs": intrs.to(dev), "c2ws": c2ws.to(dev),
                "near_fars": near_fars.to(dev), "near": near_fars[0, 0].reshape(1, 1).to(dev),
                "far": near_fars[0, 1].reshape(1, 1).to(dev), "rays_o": rays_o, "rays_d": rays_d, "bound_min": BMIN,
                "bound_max": BMAX, "hw": (H, W), "mesh_resolution": 256}
        with torch.no_grad():
            outs.append(model("val", ipts, 1.0))
    a, b = outs
    assert len(a["vertices"]) > 1000
    for k in ("vertices", "triangles", "img_fine", "normal_img", "sdf_depth", "render_depth"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_mesh_extraction_conf_key():
    """render.mesh_extraction / render.mesh_band_margin are read like render.sdf_precision; unknown values raise."""
    from surf_amd.implicit_surface import MESH_BAND_MARGIN
    assert _model().mesh_extraction == "dense"
    assert _model().mesh_band_margin == MESH_BAND_MARGIN > 0
    m = _model(mesh_extraction="band", mesh_band_margin=3.5)
    assert m.mesh_extraction == "band" and m.mesh_band_margin == 3.5
    with pytest.raises(ValueError):
        _model(mesh_extraction="octree")
    with pytest.raises(ValueError):
        _model(mesh_band_margin=-1.0)
    with pytest.raises(ValueError):
        m.extract_geometry(None, None, BMIN, BMAX, 64, 0.0, mesh_extraction="sparse")
