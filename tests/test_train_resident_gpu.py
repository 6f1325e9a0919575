"""GPU: the device-resident DTU training set.  The two kernels of train_batch.hip against numpy mirrors of their written-out
sequences, bit for bit; `DTUDeviceTrainSet` against the host reader and the REFERENCE's reader (tests/golden/dataset_items.npz)
on misses and hits; what a hit uploads; the budget; no aliasing of the cache; one training step from a host-made and from a
device-made batch."""
import numpy as np
import pytest
import torch

from surf_amd import conf
from tests.golden.dtu_scene import DATASET_CONF, SEEDS, write_dtu_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _scaled(d, scale):
    """(float)((double)d * scale): one fp64 product, one round-to-nearest conversion."""
    return (d.astype(np.float64) * np.float64(scale)).astype(f32)


def _planes(g, h, w, special=True):
    """A uint8 image, a 0/1 mask and two unscaled depth maps; the depths hold 0, a value whose scaled product is an fp32 denormal
    and an fp32 denormal itself."""
    image = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = (g.random((h, w)) > 0.4).astype(np.uint8)
    depth, pseudo = (400 + 600 * g.random((h, w))).astype(f32), (400 + 600 * g.random((h, w))).astype(f32)
    if special:
        depth.reshape(-1)[[0, 3, h * w - 1]] = [0.0, 3e-36, 1e-40]
        pseudo.reshape(-1)[[1, 2, h * w - 2]] = [3e-36, 0.0, 1e-40]
    return image, mask, depth, pseudo


SCALE = float(np.float64(1) / np.float64(337.7))


@pytest.mark.parametrize("hw", [(5, 7), (6, 8), (48, 64)])
@pytest.mark.parametrize("V", [1, 3, 5, 8])
def test_train_views_equals_its_numpy_mirror(hw, V):
    """imgs = texel / 256 transposed to CHW, masks as fp32, depths scaled by (float)((double)d * scale): bit-equal (compared as
    uint32).  35 pixels: one tail group of three; 48 pixels: a multiple of 4, not of 64; 3072: several blocks.  The view slots are
    a permutation of the pool with one view in two slots; the two map views are once the same view and once different ones."""
    from surf_amd import ops
    h, w = hw
    g = np.random.default_rng(100 * V + h)
    pool = [_planes(g, h, w) for _ in range(V)]
    dev = [[torch.from_numpy(a).to(DEV) for a in p] for p in pool]
    order = list(g.permutation(V))
    if V > 1:
        order[-1] = order[0]                                                    # one view in two slots
    assert _scaled(pool[0][2], SCALE).reshape(-1)[3] != 0 and abs(_scaled(pool[0][2], SCALE).reshape(-1)[3]) < np.finfo(f32).tiny
    for a, b in ((order[0], order[0]), (order[0], (order[0] + 1) % V)):
        imgs, masks, depths, pseudos = ops.train_views([dev[i][0] for i in order], [dev[a][1], dev[b][1]], [dev[a][2], dev[b][2]],
                                                       [dev[a][3], dev[b][3]], SCALE)
        assert tuple(imgs.shape) == (V, 3, h, w) and tuple(masks.shape) == tuple(depths.shape) == tuple(pseudos.shape) == (2, h, w)
        want = np.stack([pool[i][0].astype(f32).transpose(2, 0, 1) / f32(256) for i in order])
        assert np.array_equal(_bits(imgs), _bits(want)), (a, b)
        assert np.array_equal(_bits(masks), _bits(np.stack([pool[a][1], pool[b][1]]).astype(f32))), (a, b)
        assert np.array_equal(_bits(depths), _bits(np.stack([_scaled(pool[a][2], SCALE), _scaled(pool[b][2], SCALE)]))), (a, b)
        assert np.array_equal(_bits(pseudos), _bits(np.stack([_scaled(pool[a][3], SCALE), _scaled(pool[b][3], SCALE)]))), (a, b)


def mirror_train_rays(pick, fx, fy, inside, ki, c, image, mask, depth, pseudo, scale):
    """The operation list of train_batch.hip's header in numpy fp32: one rounding per operator, left to right as parenthesised."""
    h, w = mask.shape
    ki, c = ki.astype(f32), c.astype(f32)
    have_m = (pick >= 0) & (pick < len(inside))
    flat = inside[np.where(have_m, pick, 0)].astype(np.int64)
    x, y = np.concatenate([flat % w, fx.astype(np.int64)]), np.concatenate([flat // w, fy.astype(np.int64)])
    have = np.concatenate([have_m, np.ones(len(fx), bool)])
    px, py = x.astype(f32), y.astype(f32)
    dx = (ki[0] * px + ki[1] * py) + ki[2]
    dy = (ki[3] * px + ki[4] * py) + ki[5]
    dz = (ki[6] * px + ki[7] * py) + ki[8]
    n = np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx / n, dy / n, dz / n
    assert dx.dtype == f32 and n.dtype == f32
    rays_d = np.stack([(c[0] * dx + c[1] * dy) + c[2] * dz, (c[4] * dx + c[5] * dy) + c[6] * dz, (c[8] * dx + c[9] * dy) + c[10] * dz], 1)
    rays_o = np.broadcast_to(np.array([c[3], c[7], c[11]], f32), rays_d.shape)
    inimg = have & (x >= 0) & (x < w) & (y >= 0) & (y < h)
    at = np.where(inimg, y * w + x, 0)
    zero = f32(0)
    return {"pixels_x": np.where(have, px, zero), "pixels_y": np.where(have, py, zero), "rays_o": np.where(have[:, None], rays_o, zero),
            "rays_d": np.where(have[:, None], rays_d, zero),
            "color": np.where(inimg[:, None], image.reshape(-1, 3)[at].astype(f32) / f32(256), zero),
            "depth": np.where(inimg, _scaled(depth.reshape(-1)[at], scale), zero),
            "pseudo_depth": np.where(inimg, _scaled(pseudo.reshape(-1)[at], scale), zero),
            "mask": np.where(inimg, mask.reshape(-1)[at].astype(f32), zero)}, have, inimg


@pytest.mark.parametrize("inside_kind", ["one", "all"])
@pytest.mark.parametrize("n_rays", [1, 3, 63, 64, 65, 96])
def test_train_rays_equals_its_written_out_sequence(n_rays, inside_kind):
    """Every output bit-equal to the numpy fp32 mirror.  n_rays 1 and 3: no free pixels (n // 4 = 0); 63 / 64 / 65: one block
    and the first ray of a second; inside lists of one pixel and of all H W pixels.  Then the same call with one pick outside
    its list (every output of that ray zero) and, where there are free pixels, one or two of them outside the image (x = W; y = H) (coordinates and
    rays kept, the four gathered entries zero)."""
    from surf_amd import ops
    h, w = 11, 13
    g = np.random.default_rng(7 * n_rays + len(inside_kind))
    image, mask, depth, pseudo = _planes(g, h, w)
    inside = np.array([5 * w + 8], np.int32) if inside_kind == "one" else np.arange(h * w, dtype=np.int32)
    K = np.array([[115.69, 0.0, 6.59], [0.0, 115.33, 5.67], [0.0, 0.0, 1.0]], f32)
    ki = torch.inverse(torch.from_numpy(K)).numpy().reshape(-1)
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    c = np.concatenate([q, g.standard_normal((3, 1)) * 2], axis=1).astype(f32).reshape(-1)
    n_free = n_rays // 4
    pick = g.integers(0, len(inside), n_rays - n_free).astype(np.int32)
    fx, fy = g.integers(0, w, n_free).astype(np.int32), g.integers(0, h, n_free).astype(np.int32)
    up = lambda a: torch.from_numpy(a).to(DEV)                                                    # noqa: E731
    planes = [up(image), up(mask), up(depth), up(pseudo)]
    for faults in (False, True):
        if faults:
            pick[len(pick) // 2] = len(inside) if n_rays % 2 else -1
            if n_free:
                fx[n_free // 2], fy[0] = w, (h if n_free > 1 else fy[0])
        got = ops.train_rays(up(pick), up(fx), up(fy), up(inside), ki, c, *planes, SCALE)
        want, have, inimg = mirror_train_rays(pick, fx, fy, inside, ki, c, image, mask, depth, pseudo, SCALE)
        assert int((~have).sum()) == int(faults) and int((have & ~inimg).sum()) == (min(n_free, 2) if faults else 0)
        assert set(got) == set(want)
        for k, ref in want.items():
            assert tuple(got[k].shape) == ref.shape and got[k].dtype == torch.float32, k
            assert np.array_equal(_bits(got[k]), _bits(ref)), (k, faults)
        if faults:
            t = len(pick) // 2
            assert all(float(got[k][t].abs().max()) == 0.0 for k in got)
            if n_free:
                t = len(pick) + n_free // 2
                assert float(got["pixels_x"][t]) == w and float(got["rays_d"][t].norm()) > 0.99
                assert all(float(got[k][t].abs().max()) == 0.0 for k in ("color", "depth", "pseudo_depth", "mask"))
        else:
            assert np.allclose(np.linalg.norm(want["rays_d"], axis=1), 1.0, atol=1e-6)


# ---- the set against the host reader ------------------------------------------------------------------------------------------


def _sets(tmp_path, budget=None, **kw):
    from surf_amd.datasets import DTUDataset, DTUDeviceTrainSet
    root = tmp_path / "dtu"
    if not root.exists():
        write_dtu_scene(str(root))
    c = conf.from_dict(dict(DATASET_CONF, data_dir=str(root), n_rays=96, **kw))
    host = DTUDataset(c, "train")
    return host, DTUDeviceTrainSet(DTUDataset(c, "train"), DEV, **({} if budget is None else {"budget_bytes": budget}))


def _seeded(ds, idx, seeds):
    np.random.seed(seeds[0])
    torch.manual_seed(seeds[1])
    return ds[idx]


def assert_items_equal(got, ref):
    """Device item against the host reader's: same keys, dtypes and shapes; every tensor on the device and torch.equal to the
    host's but rays_d (the kernel's fixed summation order against the host's matmuls), which gets the reader tolerance."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k, r in ref.items():
        g = got[k]
        if not torch.is_tensor(r):
            assert not torch.is_tensor(g) and type(g) is type(r) and g == r, k
            continue
        assert g.is_cuda and g.dtype == r.dtype and tuple(g.shape) == tuple(r.shape), (k, g.dtype, r.dtype, g.shape, r.shape)
        if k == "rays_d":
            assert torch.allclose(g.cpu(), r, rtol=1e-6, atol=1e-6 * float(r.abs().max() + 1)), float((g.cpu() - r).abs().max())
        else:
            assert torch.equal(g.cpu(), r), k


def test_device_item_equals_the_host_readers_item(tmp_path):
    """The dtu_scene fixture (raw 60 x 80 -> img_hw 48 x 64, two source views), same seeds: the device item equals the host
    reader's item, pseudo_pts in fp64 included, on the miss and on the following hit, for two seed pairs; with dtu_scene.SEEDS it
    also equals the `train/` entries the REFERENCE's reader wrote (tests/test_datasets.py's comparison)."""
    from tests.conftest import load_npz
    from tests.test_datasets import _compare_with_reference_item
    gold = load_npz("dataset_items.npz")
    host, ds = _sets(tmp_path)
    for n, seeds in enumerate(((SEEDS["numpy"], SEEDS["torch"]), (3, 4))):
        ref = _seeded(host, 0, seeds)
        for call in range(2):
            hits, misses = ds.stats.hits, ds.stats.misses
            item = _seeded(ds, 0, seeds)
            assert_items_equal(item, ref)
            assert item["pseudo_pts"].dtype == torch.float64 and item["imgs"].is_contiguous()
            if n == 0:
                assert (ds.stats.misses > misses) == (call == 0) and (call == 0 or ds.stats.hits == hits + 5)
                _compare_with_reference_item({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in item.items()}, gold, "train")
    assert ds.stats.uncached == 0


def _resident_bytes(host, views):
    """What the cache holds for `views` of scan24, light 3, from the shapes: a uint8 image; a uint8 mask, its int32 inside list
    and two fp32 depth maps per view."""
    from surf_amd.datasets import mvs_io
    H, W = host.img_hw
    n_inside = [int((mvs_io.read_image(host.files.mask("scan24", v), host.img_hw) > 10).sum()) for v in views]
    return len(views) * (3 * H * W) + sum(H * W + 4 * n + 2 * 4 * H * W for n in n_inside)


def test_a_hit_uploads_indices_cameras_and_points_only(tmp_path, monkeypatch):
    """Five items (every view of the fixture is the reference view of one): after one pass a second pass uploads at most 64 KiB
    per item - by the set's own count AND by a watch on every Tensor.to that moves host memory to the device - `misses` does not
    grow and resident_bytes is the sum the shapes give.  warm() fills the same cache without a draw."""
    host, ds = _sets(tmp_path, ref_view=[0, 1, 2, 3, 4], total_views=5)
    assert len(ds) == 5
    np.random.seed(1)
    torch.manual_seed(2)
    for i in range(5):
        ds[i]
    want = _resident_bytes(host, range(5))
    assert ds.stats.resident_bytes == want and ds.stats.misses == 10 and ds.stats.uncached == 0
    assert want < ds.stats.uploaded_bytes < want + 5 * 64 * 1024
    seen = []
    real_to = torch.Tensor.to

    def watched_to(self, *a, **k):
        out = real_to(self, *a, **k)
        if not self.is_cuda and out.is_cuda:
            seen.append(self.numel() * self.element_size())
        return out

    monkeypatch.setattr(torch.Tensor, "to", watched_to)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: watched_to(self, "cuda"))
    for i in range(5):
        before, n_seen = ds.stats.uploaded_bytes, len(seen)
        item = ds[i]
        sent = ds.stats.uploaded_bytes - before
        assert 2048 * 3 * 8 < sent <= 64 * 1024 and sum(seen[n_seen:]) == sent, (sent, seen[n_seen:])
        assert all(v.is_cuda for v in item.values() if torch.is_tensor(v))
    assert ds.stats.misses == 10 and ds.stats.resident_bytes == want and ds.stats.hits >= 5 * 7
    monkeypatch.undo()
    _, warmed = _sets(tmp_path, ref_view=[0, 1, 2, 3, 4], total_views=5)
    state = (np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    warmed.warm(range(5))
    assert warmed.stats.resident_bytes == want and warmed.stats.misses == 10
    assert np.array_equal(np.random.get_state()[1], state[0]) and torch.equal(torch.get_rng_state(), state[1])


@pytest.mark.parametrize("budget", [1000, 60000])
def test_a_full_budget_changes_nothing_but_the_uploads(tmp_path, budget):
    """budget_bytes below one view's entries: 1000 (nothing is kept) and 60000 (the item's three 9216-byte images are kept, its
    32768-byte view entries - mask, inside list, two depth maps - are refused).  The items still equal the host reader's, for two
    seed pairs in a row, resident_bytes <= budget_bytes and uncached > 0."""
    host, ds = _sets(tmp_path, budget=budget)
    for seeds in ((SEEDS["numpy"], SEEDS["torch"]), (5, 6)):
        assert_items_equal(_seeded(ds, 0, seeds), _seeded(host, 0, seeds))
    assert ds.stats.resident_bytes <= budget and ds.stats.uncached > 0
    assert (ds.stats.resident_bytes == 0) == (budget == 1000)


def test_returned_tensors_do_not_alias_the_cache(tmp_path):
    host, ds = _sets(tmp_path)
    seeds = (SEEDS["numpy"], SEEDS["torch"])
    ref = _seeded(host, 0, seeds)
    item = _seeded(ds, 0, seeds)
    for k, v in item.items():
        if torch.is_tensor(v):
            v.fill_(7) if v.dtype.is_floating_point else v.zero_()
    assert float(item["imgs"].min()) == 7.0 and float(item["mask_ref"].min()) == 7.0
    assert_items_equal(_seeded(ds, 0, seeds), ref)


LOSS = {"color_weight": 1.0, "sparse_scale_factor": 100, "sparse_weight": 0.02, "igr_weight": 0.1, "mfc_weight": 0.5, "smooth_weight": 0.0001,
        "depth_weight": 0.0, "ptloss_weight": 1.0, "pseudo_auxi_depth_weight": 1.0, "pseudo_sdf_weight": 1.0, "pseudo_depth_weight": 1.0,
        "stage_weights": [0.25, 0.5, 0.75, 1.0]}


def test_host_and_device_batches_drive_the_same_training_step(tmp_path):
    """One train_step of the small model configuration (base volume 16^3, a 96 x 128 synthetic scene in DTU's file formats) from
    identical model state and seeds, fed by the host reader's batch (uploaded whole) and by the device-made batch.  The two
    differ in rays_d alone, by the fp32 error of two summation orders; the yardstick is tests/test_finetune_gpu.py's: the host
    path's own loss with its rays_d shifted by +e_ref and by -e_ref (e_ref = max |host rays_d - float64|), spread = the larger of
    the two loss changes, |loss_device - loss_host| <= 4 spread.
    Measured on the MI355X (gfx950): e_ref = e_dev = 1.084e-07 (0 of the 768 rays_d components differ from the host's);
    loss_host = loss_device = 7.583338260650635; the shifted host runs gave 7.583338737487793 and 7.583337783813477:
    spread = 4.768e-07."""
    from bench import surf_conf
    from surf_amd import synthetic
    from surf_amd.datasets import DTUDataset, DTUDeviceTrainSet
    from surf_amd.finetune import to_device
    from surf_amd.losses import Loss
    from surf_amd.surf import SuRF
    from surf_amd.training import train_step
    from tests.test_end_to_end_dtu import _write_scene
    from tests.test_finetune_gpu import rays_d_float64
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    c = conf.from_dict({"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
                        "num_src_view": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W], "total_views": 4,
                        "n_rays": 256})
    host, ds = DTUDataset(c, "train"), DTUDeviceTrainSet(DTUDataset(c, "train"), DEV)
    hb, db = _seeded(host, 0, (20, 21)), _seeded(ds, 0, (20, 21))
    assert_items_equal(db, hb)
    mcfg = conf.from_dict(surf_conf(base_dim=16))
    torch.manual_seed(0)
    state = SuRF(mcfg).state_dict()
    loss_fn = Loss(conf.from_dict(LOSS)).to(DEV)

    def one_step(batch):
        m = SuRF(mcfg)
        m.load_state_dict(state)
        m = m.to(DEV).train()
        m.logit_override = synthetic.sphere_logit
        opt = torch.optim.Adam(m.get_optim_params({"mlp_lr": 5e-4, "feat_lr": 1e-3}))
        torch.manual_seed(22)
        return train_step(m, batch, batch, loss_fn, opt, 1.0, 2)["loss"]

    d64 = rays_d_float64(hb["pixels_x"], hb["pixels_y"], hb["intrs"][0], hb["c2ws"][0])
    e_ref = float((hb["rays_d"].double() - d64).abs().max())
    e_dev = float((db["rays_d"].cpu().double() - d64).abs().max())
    loss_host = one_step(to_device(hb, DEV))
    assert one_step(to_device(hb, DEV)) == loss_host          # the yardstick below measures rays_d, not run-to-run noise
    loss_dev = one_step(db)
    shifted = [one_step(to_device(dict(hb, rays_d=hb["rays_d"] + s * e_ref), DEV)) for s in (1.0, -1.0)]
    spread = max(abs(x - loss_host) for x in shifted)
    print(f"e_ref = {e_ref:.3e}  e_dev = {e_dev:.3e}  loss_host = {loss_host!r}  loss_dev = {loss_dev!r}  shifted = {shifted!r}  "
          f"spread = {spread:.3e}  |dev - host| = {abs(loss_dev - loss_host):.3e}  rays_d components differing: "
          f"{int((db['rays_d'].cpu() != hb['rays_d']).sum())} of {hb['rays_d'].numel()}")
    assert np.isfinite([loss_host, loss_dev] + shifted).all() and e_dev <= 4 * e_ref
    assert abs(loss_dev - loss_host) <= 4 * spread, (loss_dev, loss_host, spread)
