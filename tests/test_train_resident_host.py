"""Device-resident DTU training set, host side (no GPU): the draw order of `DTUDeviceTrainSet.plan` against the REFERENCE's reader
(tests/golden/dataset_items.npz, `train/`), the uint8-first nearest-neighbour pick against `read_image`, `get_loader`'s default,
the refusal inside a DataLoader worker and the new entry points in header, binding and library."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from surf_amd import conf
from surf_amd.datasets import DTUDataset, DTUDeviceTrainSet, get_loader, mvs_io
from tests.golden.dtu_scene import DATASET_CONF, SEEDS, write_dtu_scene


def _train_conf(root, **kw):
    return conf.from_dict(dict(DATASET_CONF, data_dir=str(root), n_rays=96, **kw))


@pytest.fixture()
def dtu_root(tmp_path):
    root = tmp_path / "dtu"
    write_dtu_scene(str(root))
    return root


def test_plan_draws_what_the_reference_reader_draws(dtu_root):
    """plan(0) on the dtu_scene fixture, dtu_scene.SEEDS, n_rays = 96: pixels_x / pixels_y, src_idx and view_ids are the
    reference reader's (the three torch draws and the two numpy draws in its order); cameras and pseudo_pts by the reader
    tolerance of tests/test_datasets.py.  A second seeded plan - the mask and the cloud now come from the recorded sizes, not
    from a fresh read - draws the same."""
    from tests.conftest import load_npz
    gold = load_npz("dataset_items.npz")
    host = DTUDataset(_train_conf(dtu_root), "train")
    ds = DTUDeviceTrainSet(host, "cuda")
    assert len(ds) == len(host) == 1 and ds.img_hw == [48, 64]
    for _ in range(2):
        np.random.seed(SEEDS["numpy"])
        torch.manual_seed(SEEDS["torch"])
        p = ds.plan(0, pixels=True)
        assert torch.equal(p.pixels_x, gold["train/pixels_x"]) and torch.equal(p.pixels_y, gold["train/pixels_y"])
        assert p.pixels_x.dtype == gold["train/pixels_x"].dtype
        assert int(p.src_idx) == int(gold["train/src_idx"]) and p.view_ids == gold["train/view_ids"].tolist()
        for k, got in (("intrs", p.intrs), ("c2ws", p.c2ws), ("near_fars", p.near_fars), ("scale_mat", p.scale_mat), ("pseudo_pts", p.pseudo_pts)):
            ref = gold[f"train/{k}"]
            assert got.dtype == ref.dtype and got.shape == ref.shape, k
            assert torch.allclose(got, ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max() + 1)), k
    # ... and what this package's own reader makes of the same seeds, bit for bit
    np.random.seed(SEEDS["numpy"])
    torch.manual_seed(SEEDS["torch"])
    item = host[0]
    for k in ("pixels_x", "pixels_y", "intrs", "c2ws", "near_fars", "scale_mat", "pseudo_pts"):
        assert torch.equal(getattr(p, k), item[k]), k
    assert ds.stats.uploaded_bytes == 0 and ds.stats.misses == 0


@pytest.mark.parametrize("raw_hw,hw", [((7, 5), (13, 9)), ((60, 80), (48, 64)), ((9, 11), (9, 11))])
def test_nearest_pick_on_uint8_equals_the_readers(tmp_path, raw_hw, hw):
    """resize_nearest on the uint8 array, then fp32 / 256 == read_image (fp32 first, then the pick) / 256, bit for bit: colour
    images and grey masks, up-sampling, down-sampling and the identity."""
    from surf_amd.datasets.dtu_resident import _read_u8
    g = np.random.default_rng(raw_hw[0])
    for channels in (3, 0):
        u8 = (g.random(raw_hw + ((3,) if channels else ())) * 256).astype(np.uint8)
        path = str(tmp_path / f"img{channels}.png")
        Image.fromarray(u8).save(path)
        picked = mvs_io.resize_nearest(u8, hw)
        assert picked.dtype == np.uint8 and picked.shape[:2] == hw
        want = mvs_io.read_image(path, hw) / 256.0
        got = picked.astype(np.float32) / 256
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
        assert np.array_equal(got.astype(want.dtype), want)
        assert np.array_equal(_read_u8(path, hw, channels), picked)
    with pytest.raises(ValueError, match="8-bit"):
        _read_u8(str(tmp_path / "img0.png"), hw, 3)                                   # a grey file where an RGB image belongs


def test_loader_default_is_the_host_reader(dtu_root):
    """device=None: the three objects as before, the loader's dataset the plain DTUDataset with the workers asked for.  With a
    device: the same samplers and collate function over a DTUDeviceTrainSet, in this process; val mode and the other readers
    keep the host path."""
    from surf_amd.datasets import collect_fn
    from torch.utils.data import RandomSampler, SequentialSampler
    loader, sampler, dataset = get_loader(_train_conf(dtu_root), "train", False, num_workers=0)
    assert type(dataset) is DTUDataset and loader.dataset is dataset and isinstance(sampler, RandomSampler)
    assert loader.collate_fn is collect_fn and loader.drop_last and loader.batch_size == 1
    assert get_loader(_train_conf(dtu_root), "train", False)[0].num_workers == 8
    torch.manual_seed(0)
    np.random.seed(0)
    assert next(iter(loader))["rays_d"].shape == (96, 3)
    dl, ds_sampler, dset = get_loader(_train_conf(dtu_root), "train", False, device="cuda")
    assert isinstance(dset, DTUDeviceTrainSet) and dl.dataset is dset and type(dset.dataset) is DTUDataset
    assert dl.num_workers == 0 and isinstance(ds_sampler, RandomSampler) and dl.collate_fn is collect_fn and dl.drop_last
    vl, vs, vd = get_loader(_train_conf(dtu_root), "val", False, num_workers=0, device="cuda")
    assert type(vd) is DTUDataset and vl.dataset is vd and isinstance(vs, SequentialSampler)
    with pytest.raises(TypeError):
        DTUDeviceTrainSet(vd, "cuda")
    with pytest.raises(ValueError, match="GPU"):
        DTUDeviceTrainSet(dataset, "cpu")


def test_refuses_to_run_in_a_loader_worker(dtu_root):
    """The set holds device memory: inside a DataLoader worker __getitem__ raises before it touches anything."""
    from torch.utils.data import DataLoader
    ds = DTUDeviceTrainSet(DTUDataset(_train_conf(dtu_root), "train"), "cuda")
    with pytest.raises(RuntimeError, match="num_workers=0"):
        next(iter(DataLoader(ds, 1, num_workers=1, collate_fn=lambda d: d[0])))
    assert ds.stats.misses == 0


def test_train_batch_entry_points_are_declared_bound_and_exported():
    from surf_amd import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "surf_hip.h")).read()
    L = _lib.lib()
    for name in ("surf_train_views", "surf_train_rays"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).errcheck is not None
    assert _lib.ABI_VERSION == 41 and L.surf_abi_version() == 41
    assert _lib.SIGNATURES["surf_train_views"][1][7] is _lib.ctypes.c_double            # the scale: a double by value
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_train_views(None, 0, 0, 0, None, None, None, 1.0, None, None, None, None, None)
