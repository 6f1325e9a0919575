"""GPU: per-scene fine-tuning.  The ray sampler of finetune_rays.hip against its own written-out fp32 sequence, the device-resident
reader against the REFERENCE's reader (tests/golden/finetune_items.npz), what a step uploads, the whole loop through
scripts/finetune.py on a synthetic scene in DTU's file formats, and the host-made against the device-made batch in one step."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from surf_amd import conf
from tests.golden.dtu_finetune_scene import (FINETUNE_CONF, SEEDS, add_finetune_folders, write_finetune_scene,
                                             write_sphere_pseudo_data)
from tests.test_dtu_finetune import compare_with_reference_item

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _dataset(tmp_path):
    from surf_amd.datasets import get_loader
    root = tmp_path / "dtu"
    write_finetune_scene(str(root))
    return get_loader(conf.from_dict(dict(FINETUNE_CONF, data_dir=str(root))), "finetune", False)


def mirror_rays(px, py, ki, c):
    """The operation list of finetune_rays.hip's header in numpy fp32: one rounding per operator, left to right as parenthesised."""
    px, py, ki, c = px.astype(f32), py.astype(f32), ki.astype(f32), c.astype(f32)
    dx = (ki[0] * px + ki[1] * py) + ki[2]
    dy = (ki[3] * px + ki[4] * py) + ki[5]
    dz = (ki[6] * px + ki[7] * py) + ki[8]
    n = np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx / n, dy / n, dz / n
    assert dx.dtype == f32 and n.dtype == f32
    rays_d = np.stack([(c[0] * dx + c[1] * dy) + c[2] * dz, (c[4] * dx + c[5] * dy) + c[6] * dz, (c[8] * dx + c[9] * dy) + c[10] * dz], 1)
    rays_o = np.broadcast_to(np.array([c[3], c[7], c[11]], f32), rays_d.shape)
    return rays_o, rays_d


def rays_d_float64(px, py, K, c2w):
    """The directions of the same pixels from the same K and c2w in float64."""
    p = torch.stack([px.double(), py.double(), torch.ones_like(px, dtype=torch.float64)], 1)
    d = p @ torch.inverse(K.double()[:3, :3]).T
    d = d / d.norm(dim=1, keepdim=True)
    return d @ c2w.double()[:3, :3].T


def texels(image, depth, px, py):
    """image / depth at (long(py), long(px)) - truncation towards zero - by plain indexing; zeros for a pixel outside the image."""
    x, y = px.long(), py.long()
    inside = (x >= 0) & (x < image.shape[1]) & (y >= 0) & (y < image.shape[0])
    at = (y.clamp(0, image.shape[0] - 1), x.clamp(0, image.shape[1] - 1))
    return (torch.where(inside[:, None], image[at], torch.zeros(1)), torch.where(inside, depth[at], torch.zeros(1)), inside)


def test_kernel_equals_its_written_out_sequence(tmp_path):
    """1200 x 1600 planes, the three cameras of the fixture rig with DTU's raw intrinsics, 20 000 random float pixels per view +
    the image corners + the three columns at which linspace(0, 1599, 400) is an exact integer (i = 133, 266, 399), every row of
    the validation lattice: rays_o / rays_d bit-equal to the numpy fp32 mirror of the header's operation list, colour / pseudo
    depth bit-equal to plain indexing; the int32 entry likewise; the point gather bit-equal to plain indexing.  Nine coordinates
    on and beyond the image's edges and four point indices outside the cloud pin the truncation and the zero fill."""
    from surf_amd import ops
    from tests.golden.dtu_scene import K_RAW
    dev = torch.device("cuda:0")
    ds = _dataset(tmp_path)
    H, W = 1200, 1600
    g = torch.Generator().manual_seed(3)
    tx, ty = torch.linspace(0, W - 1, W // 4), torch.linspace(0, H - 1, H // 4)
    cols = tx[[133, 266, 399]]
    assert cols.tolist() == [533.0, 1066.0, 1599.0]
    K = torch.eye(4)
    K[:3, :3] = torch.from_numpy(K_RAW).float()
    kinv = K.inverse()[:3, :3].reshape(-1).contiguous()
    for vid in range(3):
        image = torch.rand(H, W, 3, generator=g)
        depth = torch.rand(H, W, generator=g) + 0.5
        # ... and what the header promises off the image: (-1, 0) truncates to pixel 0; <= -1 or >= the size yields zeros
        edge_x = torch.tensor([-0.5, 3.25, -0.999, -1.0, float(W), 5.0, 5.0, -40.0, W + 0.5])
        edge_y = torch.tensor([3.25, -0.5, -0.999, 5.0, 5.0, float(H), -2.5, -40.0, H - 1.0])
        px = torch.cat([torch.rand(20000, generator=g) * (W - 1), torch.tensor([0.0, W - 1, 0.0, W - 1]), cols.repeat_interleave(len(ty)), edge_x])
        py = torch.cat([torch.rand(20000, generator=g) * (H - 1), torch.tensor([0.0, 0.0, H - 1, H - 1]), ty.repeat(3), edge_y])
        c2w = ds.c2ws[vid, :3, :4].reshape(-1).contiguous()
        for as_int in (False, True):
            qx, qy = (px.int(), py.int()) if as_int else (px, py)
            o, d, col, dep = ops.finetune_rays(qx.to(dev), qy.to(dev), kinv.to(dev), c2w.to(dev), image.to(dev), depth.to(dev))
            ro, rd = mirror_rays(qx.numpy(), qy.numpy(), kinv.numpy(), c2w.numpy())
            assert np.array_equal(d.cpu().numpy().view(np.uint32), rd.view(np.uint32)), (vid, as_int, np.abs(d.cpu().numpy() - rd).max())
            assert np.array_equal(o.cpu().numpy().view(np.uint32), np.ascontiguousarray(ro).view(np.uint32)), (vid, as_int)
            want_col, want_dep, inside = texels(image, depth, qx, qy)
            assert int((~inside).sum()) == 6 and bool(inside[-9:-6].all())
            assert torch.equal(col.cpu(), want_col) and torch.equal(dep.cpu(), want_dep), (vid, as_int)
            assert abs(float(d.norm(dim=1).mean()) - 1.0) < 1e-6
        o, d, col, dep = ops.finetune_rays(px.to(dev), py.to(dev), kinv.to(dev), c2w.to(dev), image.to(dev), None)    # validation: no depth
        assert dep is None and torch.equal(col.cpu(), texels(image, depth, px, py)[0])
    pts = torch.randn(3000, 3, generator=g)
    idx = torch.cat([torch.randint(0, 3000, [2048], generator=g), torch.tensor([0, 2999, -1, 3000, -2 ** 31, 2 ** 31 - 1])])
    ok = (idx >= 0) & (idx < 3000)
    want = torch.where(ok[:, None], pts[idx.clamp(0, 2999)], torch.zeros(1))
    assert torch.equal(ops.finetune_gather_pts(pts.to(dev), idx.int().to(dev)).cpu(), want) and int((~ok).sum()) == 4


def test_device_reader_equals_the_reference_reader(tmp_path):
    """Same fixture and seeds as tests/test_dtu_finetune.py, through dataset.to("cuda").  Every entry is a device tensor; against
    the REFERENCE's items: keys / shapes / dtypes, integers and view_ids equal, floats by the reader tolerance; against this
    reader's own host items: every gather and every camera entry bit-equal (they are copies; pseudo_pts is held in fp32 on the
    device: equal to the host rows rounded to fp32).  rays_d: with d64 the float64 directions of the same pixels from the same K
    and c2w, e_ref = max |fixture - d64| (the reference's own fp32 error) and e_dev = max |device - d64|; e_dev <= 4 e_ref.
    Measured on the MI355X (gfx950), (e_ref, e_dev): get_random_rays view 0 (9.347e-08, 9.347e-08), view 1 (1.172e-07, 1.172e-07),
    view 2 (1.172e-07, 1.172e-07); get_rays_at(0) (1.017e-07, 1.017e-07).  Equal maxima are not equal values: the number of
    components whose bits differ from the reference's is printed beside them.  The three seeded training draws (integer pixels)
    came out bit-equal to the reference's; of the 576 components of the validation lattice 3 differ, each by one ulp (5.96e-08) -
    the kernel's fixed summation order against the reference's matmuls.  That count is reported, not asserted: the issue's
    statement is the 4 e_ref bound."""
    from tests.conftest import load_npz
    gold = load_npz("finetune_items.npz")
    host, ds = _dataset(tmp_path), _dataset(tmp_path / "b")
    assert ds.to("cuda") is ds and ds.device.type == "cuda"
    figures = []

    def check(tag, item, ref_item, px, py, vid):
        d64 = rays_d_float64(px.float(), py.float(), ds.intrs[vid], ds.c2ws[vid])
        e_ref = float((gold[f"{tag}/rays_d"].double() - d64).abs().max())
        e_dev = float((item["rays_d"].cpu().double() - d64).abs().max())
        figures.append((tag, e_ref, e_dev))
        got_d, ref_d = item["rays_d"].cpu(), gold[f"{tag}/rays_d"]
        print(f"{tag}: e_ref = {e_ref:.3e}  e_dev = {e_dev:.3e}  components differing from the reference: {int((got_d != ref_d).sum())} of "
              f"{ref_d.numel()}, max |difference| = {float((got_d - ref_d).abs().max()):.3e}")

        def override(k, got, ref):
            if k == "rays_d":
                assert got.dtype == ref.dtype and got.shape == ref.shape and e_dev <= 4 * e_ref, (tag, e_dev, e_ref)
                return True
            if k == "pseudo_pts":
                assert got.dtype == torch.float32 and torch.equal(got, ref_item[k].float()), tag
                assert torch.allclose(got.double(), ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max() + 1))
                return True
            return False

        compare_with_reference_item(item, gold, tag, override)
        for k, v in item.items():
            if torch.is_tensor(v):
                assert v.is_cuda, (tag, k)
                if k not in ("rays_d", "pseudo_pts"):
                    assert torch.equal(v.cpu(), ref_item[k]), (tag, k)
            else:
                assert v == ref_item[k], (tag, k)

    compare_with_reference_item(ds.get_all_images(), gold, "all_images")
    for vid in range(3):
        torch.manual_seed(SEEDS["torch"])
        ref_item = host.get_random_rays(torch.tensor(vid))
        torch.manual_seed(SEEDS["torch"])
        px, py, _ = host.draw()
        torch.manual_seed(SEEDS["torch"])
        check(f"random_rays{vid}", ds.get_random_rays(torch.tensor(vid)), ref_item, px, py, vid)
    px, py = host.lattice()
    check("rays_at0", ds.get_rays_at(0), host.get_rays_at(0), px, py, 0)
    assert len(figures) == 4


def test_a_step_uploads_indices_only(tmp_path, monkeypatch):
    """After to(device): ten get_random_rays calls.  Each may send the packed int32 draw - (2 n_rays + 2048) x 4 bytes, 12 KB at
    512 rays - and nothing else: below 64 KB per call, by the reader's own count AND by a watch on every Tensor.to / .cuda that
    moves host memory to the device meanwhile.  `imgs` is the cached device tensor, not a new copy."""
    ds = _dataset(tmp_path).to("cuda")
    ds.get_random_rays(torch.tensor(0))
    seen = []
    real_to = torch.Tensor.to

    def watched_to(self, *a, **k):
        out = real_to(self, *a, **k)
        if not self.is_cuda and out.is_cuda:
            seen.append(self.numel() * self.element_size())
        return out

    monkeypatch.setattr(torch.Tensor, "to", watched_to)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: watched_to(self, "cuda"))
    ptrs = {}
    for call in range(10):
        before, n_seen = ds.uploaded_bytes, len(seen)
        item = ds.get_random_rays(torch.tensor(call % 3))
        sent = ds.uploaded_bytes - before
        assert sent == (2 * ds.n_rays + 2048) * 4 and sent < 64 * 1024, sent
        assert sum(seen[n_seen:]) == sent, (seen[n_seen:], sent)
        assert all(v.is_cuda for v in item.values() if torch.is_tensor(v))
        assert ptrs.setdefault(call % 3, item["imgs"].data_ptr()) == item["imgs"].data_ptr()
        assert tuple(item["imgs"].shape) == (3, 3, 48, 64) and item["imgs"].is_contiguous()
    before = ds.uploaded_bytes
    ds.get_rays_at(0)
    first = ds.uploaded_bytes - before                      # the lattice goes up once ...
    ds.get_rays_at(0)
    assert first == 2 * 192 * 4 and ds.uploaded_bytes - before == first          # ... and is cached


LOSS = {"color_weight": 1.0, "sparse_weight": 0.01, "igr_weight": 0.1, "sparse_scale_factor": 100, "mfc_weight": 1.0, "smooth_weight": 0.0001,
        "tv_weight": 0.0, "depth_weight": 0.0, "ptloss_weight": 1.0, "pseudo_auxi_depth_weight": 1.0, "pseudo_sdf_weight": 1.0,
        "stage_weights": [0.25, 0.5, 0.75, 1.0], "pseudo_depth_weight": 1.0}                    # confs/surf_finetune.conf:34-48


def _finetune_setup(tmp_path, H=96, W=128):
    """A 96 x 128 synthetic DTU-format scene (tests/test_end_to_end_dtu.py's) with the fine-tuning folders, a conf file and a seeded
    generalisation checkpoint."""
    from bench import surf_conf
    from surf_amd.surf import SuRF
    from tests.test_end_to_end_dtu import _write_scene
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    add_finetune_folders(str(root), n_views=4, hw=(H, W), n_points=2500, depth=(600.0, 0.0), spread=40.0)
    mcfg = surf_conf(base_dim=16)
    cfg = {"general": {"base_exp_dir": str(tmp_path / "exp")},
           "finetune_dataset": {"dataset_name": "DTUDatasetFinetune", "data_dir": str(root), "scene": "scan24", "factor": 1.0,
                                "interval_scale": 1.0, "num_interval": 192, "img_hw": [H, W], "n_rays": 256, "ref_view": 1,
                                "val_res_level": 2},
           "train": {"lr_conf": {"mlp_lr": 5e-4, "vol_lr": [1e-1, 1e-2, 1e-2, 1e-3]}, "epochs": 5000, "anneal_end": 0, "warmup": 0,
                     "alpha": 0.02, "save_freq": 6, "log_freq": 100, "val_freq": 6, "loss": LOSS},
           "model": mcfg}
    write_sphere_pseudo_data(cfg["finetune_dataset"])
    conf_path = tmp_path / "surf_finetune_synth.conf"
    conf_path.write_text(json.dumps(cfg, indent=1))                                             # (JSON is a HOCON subset)
    torch.manual_seed(0)
    ckpt = tmp_path / "general.ckpt"
    torch.save({"model": SuRF(conf.from_dict(mcfg)).state_dict()}, ckpt)
    return cfg, conf_path, ckpt


def _script():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import finetune as script
    return script


def test_the_loop_trains(tmp_path):
    """scripts/finetune.py, 12 steps, checkpoints and validation every 6: the loss falls, both parameter groups move, two
    checkpoints and two world-frame PLYs appear, the final checkpoint reproduces the live model's validation render bit for bit,
    and the final mesh is a closed genus-0 surface."""
    from surf_amd import mesh_io
    from surf_amd.finetune import to_device
    from surf_amd.surf import SuRF
    cfg, conf_path, ckpt = _finetune_setup(tmp_path)
    script = _script()
    state = {}
    rec = script.run(script.parse_args(["--conf", str(conf_path), "--resume", str(ckpt), "--steps", "12", "--mesh_resolution", "64",
                                        "--logit_override", "sphere"]), state=state)
    print("loss history:", rec["loss"], "ms/step:", rec["ms_per_step"], "ms/batch:", rec["ms_per_batch"])
    assert rec["steps"] == 12 and len(rec["loss"]) == 12 and rec["views"] == [1, 0, 2] and rec["batch"] == "device"
    scene_bytes = sum(t.numel() * 4 for t in (state["dataset"].images, state["dataset"].masks, state["dataset"].pseudo_depths))
    assert scene_bytes < rec["uploaded_bytes"] < scene_bytes + 12 * (2 * 256 + 2048) * 4 + 128 * 1024, rec["uploaded_bytes"]    # the scene ONCE + 12 steps' indices + cameras, points, lattice
    assert np.isfinite(rec["loss"]).all() and np.isfinite(rec["psnr"]).all() and rec["loss"][-1] < rec["loss"][0], rec["loss"]
    assert rec["max_parameter_change"]["implicit_surface"] > 0 and rec["max_parameter_change"]["volumes"] > 0
    assert len(rec["checkpoints"]) == 2 and all(os.path.exists(p) for p in rec["checkpoints"])
    assert [os.path.basename(p) for p in rec["checkpoints"]] == ["model_005.ckpt", "model_011.ckpt"]
    assert len(rec["meshes"]) == 2 and all(os.path.exists(p) for p in rec["meshes"])
    assert os.path.dirname(rec["meshes"][-1]) == str(tmp_path / "exp" / "scan24" / "view1" / "meshes")
    assert json.load(open(tmp_path / "exp" / "scan24" / "view1" / "finetune.json"))["loss"] == rec["loss"]
    saved = torch.load(rec["checkpoints"][-1], map_location="cpu", weights_only=False)
    assert saved["epoch"] == 11 and {"model", "optimizer", "lr_scheduler"} <= set(saved)

    # the final checkpoint IS the live model: same kernels, same inputs
    dev = torch.device("cuda:0")
    live, ds = state["model"].eval(), state["dataset"]
    fresh = SuRF(conf.from_dict(cfg["model"])).to(dev).eval()
    fresh.load_params_vol(rec["checkpoints"][-1], dev)
    inputs = to_device(ds.get_rays_at(0), dev)
    inputs["mesh_resolution"] = 64
    renders = []
    for m in (live, fresh):
        torch.manual_seed(9)
        with torch.no_grad():
            renders.append(m("val", inputs, cos_anneal_ratio=1.0))
    assert torch.equal(renders[0]["color_fine"], renders[1]["color_fine"])
    assert np.array_equal(renders[0]["triangles"], renders[1]["triangles"])

    # the final mesh: a closed 2-manifold of genus 0 (tests/test_end_to_end_dtu.py's check), in the world frame
    v, t = mesh_io.read_ply(rec["meshes"][-1])
    assert len(v) > 300 and len(t) > 600
    edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all() and len(v) - len(counts) + len(t) == 2
    S = ds.scale_mat.double().numpy()
    r_world = np.linalg.norm(v - S[:3, 3][None], axis=1)
    assert 0.3 * np.linalg.norm(S[:3, 0]) < r_world.mean() < 1.0 * np.linalg.norm(S[:3, 0])


def test_resuming_from_volumes_with_host_batches_and_mesh_cleaning(tmp_path):
    """The other switches of the one command, in one short run: --load_vol resumes from a get_params_vol checkpoint of an earlier
    run (no init_volumes), --host_batch feeds the reference's host batch + upload through the same loop, --clean_mesh cleans the
    validation mesh with the VALIDATION item's masks / cameras (the reference names a key its training batch does not have,
    runner.py:376).  The cleaner only removes faces: the cleaned PLY has fewer, and its vertices lie on the uncleaned run's surface."""
    from surf_amd import mesh_io
    cfg, conf_path, ckpt = _finetune_setup(tmp_path)
    script = _script()
    base = ["--conf", str(conf_path), "--mesh_resolution", "64"]
    first = script.run(script.parse_args(base + ["--resume", str(ckpt), "--steps", "2", "--logit_override", "sphere",
                                                 "--out_dir", str(tmp_path / "a")]))
    runs = {}
    for name, extra in (("plain", []), ("cleaned", ["--clean_mesh"])):
        state = {}
        rec = script.run(script.parse_args(base + ["--resume", first["checkpoints"][-1], "--load_vol", "--host_batch", "--steps", "2",
                                                   "--out_dir", str(tmp_path / name)] + extra), state=state)
        assert rec["batch"] == "host" and rec["load_vol"] and rec["uploaded_bytes"] == 0 and state["dataset"].device.type == "cpu"
        assert rec["voxels"] == first["voxels"] and np.isfinite(rec["loss"]).all() and len(rec["meshes"]) == 1
        assert rec["max_parameter_change"]["implicit_surface"] > 0 and rec["max_parameter_change"]["volumes"] > 0
        runs[name] = (rec, mesh_io.read_ply(rec["meshes"][-1]))
    assert runs["plain"][0]["loss"][0] == runs["cleaned"][0]["loss"][0]      # same state, same seed: cleaning touches the mesh only
    (v0, t0), (v1, t1) = runs["plain"][1], runs["cleaned"][1]
    print("faces:", len(t0), "->", len(t1), "after cleaning")
    assert 0 < len(t1) <= len(t0)
    # two runs of two steps agree up to the backward's summation order, so the meshes are compared as geometry: marching-cubes
    # vertices sit on lattice edges, and a cleaned vertex lies within one lattice cell (world units) of an uncleaned one
    from scipy.spatial import cKDTree
    cell = 2.0 / 63 * float(np.linalg.norm(state["dataset"].scale_mat[:3, 0].numpy()))
    dist, _ = cKDTree(v0).query(v1)
    print("cleaned -> uncleaned vertex distance: max", float(dist.max()), "cell", cell)
    assert float(dist.max()) < cell


def test_host_and_device_batches_drive_the_same_step(tmp_path):
    """One finetune_step from identical model state (one get_params_vol file, loaded afresh each time) and identical seeds, fed by
    the host-made batch (uploaded whole) and by the device-made batch.  The two batches differ in rays_d alone, by the fp32 error
    of two summation orders, so the losses agree up to what such a perturbation does to the render.  The yardstick is measured on
    the host path itself: its loss with its own rays_d shifted by +e_ref and by -e_ref (e_ref = max |host rays_d - float64|, this
    scene, this draw); spread = the larger of the two loss changes; |loss_device - loss_host| <= 4 spread.
    Measured on the MI355X (gfx950): e_ref = e_dev = 1.539e-07; loss_host = loss_device = 1.952055811882019, so
    |loss_device - loss_host| = 0; the shifted host runs gave 1.9520541429519653 and 1.952056646347046: spread = 1.669e-06."""
    from surf_amd import finetune as FT
    from surf_amd import synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.losses import Loss
    from surf_amd.surf import SuRF
    from surf_amd.training import finetune_step
    cfg, conf_path, ckpt = _finetune_setup(tmp_path)
    dev = torch.device("cuda:0")
    c = conf.from_dict(cfg)
    host = get_loader(c["finetune_dataset"], "finetune", False)
    device_ds = get_loader(c["finetune_dataset"], "finetune", False).to(dev)
    model = SuRF(c["model"])
    model.load_state_dict(torch.load(ckpt, map_location="cpu")["model"])
    model = model.to(dev).eval()
    model.logit_override = synthetic.sphere_logit
    model.init_volumes(FT.to_device(host.get_all_images(), dev))
    vol_path = tmp_path / "volumes.ckpt"
    torch.save({"model": model.get_params_vol()}, vol_path)
    loss_fn = Loss(c["train.loss"]).to(dev)

    def one_step(batch):
        m = SuRF(c["model"]).to(dev)
        m.load_params_vol(str(vol_path), dev)
        m.train()
        opt = torch.optim.Adam(m.get_optim_params(lr_conf=c["train.lr_conf"]))
        torch.manual_seed(21)
        return finetune_step(m, batch, batch, loss_fn, opt, 1.0, 2)["loss"]

    vid = torch.tensor(1)
    torch.manual_seed(20)
    px, py, _ = host.draw()
    torch.manual_seed(20)
    hb = host.get_random_rays(vid)
    torch.manual_seed(20)
    db = device_ds.get_random_rays(vid)
    for k, v in hb.items():                                   # the same batch but for rays_d
        if torch.is_tensor(v) and k not in ("rays_d", "pseudo_pts"):
            assert torch.equal(v, db[k].cpu()), k
    d64 = rays_d_float64(px.float(), py.float(), host.intrs[1], host.c2ws[1])
    e_ref = float((hb["rays_d"].double() - d64).abs().max())
    e_dev = float((db["rays_d"].cpu().double() - d64).abs().max())
    loss_host = one_step(FT.to_device(hb, dev))
    assert one_step(FT.to_device(hb, dev)) == loss_host       # the yardstick below measures rays_d, not run-to-run noise
    loss_dev = one_step(db)
    shifted = [one_step(FT.to_device(dict(hb, rays_d=hb["rays_d"] + s * e_ref), dev)) for s in (1.0, -1.0)]
    spread = max(abs(x - loss_host) for x in shifted)
    print(f"e_ref = {e_ref:.3e}  e_dev = {e_dev:.3e}  loss_host = {loss_host!r}  loss_dev = {loss_dev!r}  shifted = {shifted!r}  "
          f"spread = {spread:.3e}  |dev - host| = {abs(loss_dev - loss_host):.3e}")
    assert np.isfinite([loss_host, loss_dev] + shifted).all() and e_dev <= 4 * e_ref
    assert abs(loss_dev - loss_host) <= 4 * spread, (loss_dev, loss_host, spread)
