"""Per-scene fine-tuning, host side: the reader `surf_amd.datasets.DTUDatasetFinetune` against the REFERENCE's own reader, and the
learning-rate schedule against the reference's.  tests/golden/finetune_items.npz holds what datasets/dtu_finetune.py's
`get_all_images`, `get_random_rays` (views 0, 1, 2, seeded) and `get_rays_at(0)` returned for the synthetic scene of
tests/golden/dtu_finetune_scene.py, and `WarmupCosineLR`'s multipliers (tests/golden/make_golden_finetune.py; cv2 / plyfile stood
in for as in make_golden_dataset.py).  None of this needs a GPU."""
import os
import re

import pytest
import torch

from surf_amd import conf
from tests.golden.dtu_finetune_scene import FINETUNE_CONF, SCHEDULE_STEPS, SCHEDULES, SEEDS, write_finetune_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("surf_finetune_rays", "surf_finetune_gather_pts")


def compare_with_reference_item(item, gold, tag, override=None):
    """Keys, dtypes, shapes; integers and `view_ids` equal; floats by tests/test_datasets.py:183's comparison (rtol 1e-6,
    atol 1e-6 * (max|ref| + 1)).  `override(key, got, ref)` -> True takes a key over where a caller has its own statement to make."""
    want_keys = {k.split("/")[1] for k in gold if k.startswith(tag + "/") and not k.startswith(tag + "/str/")}
    want_strs = {k.split("/")[2]: k.split("/")[3] for k in gold if k.startswith(tag + "/str/")}
    assert set(item) == want_keys | set(want_strs), set(item) ^ (want_keys | set(want_strs))
    for k, v in want_strs.items():
        assert item[k] == v
    for k in sorted(want_keys):
        ref, got = gold[f"{tag}/{k}"], item[k]
        if isinstance(got, list):                                   # view_ids: a Python list in the reference too
            assert [int(x) for x in got] == ref.tolist(), k
            continue
        got = got.cpu()
        if override is not None and override(k, got, ref):
            continue
        assert got.dtype == ref.dtype and tuple(got.shape) == tuple(ref.shape), (k, got.dtype, ref.dtype, got.shape, ref.shape)
        if not got.dtype.is_floating_point:
            assert torch.equal(got, ref), k
        else:
            assert torch.allclose(got, ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max() + 1)), (k, float((got - ref).abs().max()))


@pytest.fixture()
def finetune_dataset(tmp_path):
    from surf_amd.datasets import get_loader
    root = tmp_path / "dtu"
    write_finetune_scene(str(root))
    return get_loader(conf.from_dict(dict(FINETUNE_CONF, data_dir=str(root))), "finetune", False)


def test_get_loader_returns_the_finetune_dataset(finetune_dataset):
    from surf_amd.datasets import DATASETS, DTUDatasetFinetune
    assert DATASETS["DTUDatasetFinetune"] is DTUDatasetFinetune and isinstance(finetune_dataset, DTUDatasetFinetune)
    ds = finetune_dataset
    assert [int(v) for v in ds.all_views] == [2, 0, 1] and ds.num_views == 3 and ds.n_rays == 96 and ds.val_res_level == 4
    assert tuple(ds.images.shape) == (3, 48, 64, 3) and tuple(ds.masks.shape) == (3, 48, 64) and tuple(ds.pseudo_depths.shape) == (3, 48, 64)
    assert tuple(ds.pseudo_pts.shape) == (3000, 3)


def test_all_images_equal_the_reference_reader(finetune_dataset):
    from tests.conftest import load_npz
    compare_with_reference_item(finetune_dataset.get_all_images(), load_npz("finetune_items.npz"), "all_images")


@pytest.mark.parametrize("vid", [0, 1, 2])
def test_random_rays_equal_the_reference_reader(finetune_dataset, vid):
    """Same files, same seed, the reference's three draws in the reference's order: the same pixels and pseudo points."""
    from tests.conftest import load_npz
    torch.manual_seed(SEEDS["torch"])
    item = finetune_dataset.get_random_rays(torch.tensor(vid))
    compare_with_reference_item(item, load_npz("finetune_items.npz"), f"random_rays{vid}")
    assert item["view_ids"][0] == vid and tuple(item["pseudo_pts"].shape) == (2048, 3)


def test_rays_at_equal_the_reference_reader(finetune_dataset):
    from tests.conftest import load_npz
    item = finetune_dataset.get_rays_at(0)
    compare_with_reference_item(item, load_npz("finetune_items.npz"), "rays_at0")
    assert item["hw"].tolist() == [12, 16] and tuple(item["rays_d"].shape) == (192, 3)


def test_scale_mat_is_composed_after_the_pseudo_points(finetune_dataset):
    """dtu_finetune.py:128 before :130: the pseudo points are normalised with the un-composed scale_mat (a pure scale + shift in the
    reference view's frame), the exported scale_mat carries the reference pose."""
    ds = finetune_dataset
    back = ds.pseudo_pts[:50].float() @ ds.scale_mat[:3, :3].T + ds.scale_mat[:3, 3]            # unit sphere -> original world
    from surf_amd.datasets import mvs_io
    cloud = torch.from_numpy(mvs_io.read_ply_points(ds.files.pseudo_points(ds.scene)))[:50].float()
    assert torch.allclose(back, cloud, rtol=1e-4, atol=1e-2), float((back - cloud).abs().max())


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_warmup_cosine_lr_reproduces_the_reference_schedule(name):
    from surf_amd.finetune import warmup_cosine_lr
    from tests.conftest import load_npz
    ref = load_npz("finetune_items.npz")[f"schedule/{name}"]
    total, warmup, alpha = SCHEDULES[name]
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sched = warmup_cosine_lr(opt, total, warmup, alpha)
    got = [float(sched.lr_lambdas[0](s)) for s in SCHEDULE_STEPS[name]]
    assert ref.dtype == torch.float64 and len(got) == len(ref)
    for s, g, r in zip(SCHEDULE_STEPS[name], got, ref.tolist()):
        assert abs(g - r) <= 1e-12, (s, g, r)
    # stepped with the step number, as runner.py:323 does: the optimiser's rate follows
    opt.step()
    sched.step(SCHEDULE_STEPS[name][4])
    assert abs(opt.param_groups[0]["lr"] - ref[4].item()) <= 1e-12


def test_ray_sampler_entry_points_are_declared_and_bound():
    """The ABI version stays 41: entry points added, none changed."""
    from surf_amd import _lib
    with open(os.path.join(ROOT, "include", "surf_hip.h")) as f:
        header = f.read()
    declared = set(re.findall(r"^\s*(?:int|int64_t)\s+(surf_\w+)\s*\(", header, flags=re.M))
    assert "#define SURF_ABI_VERSION 41" in header and _lib.ABI_VERSION == 41
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "surf_amd", "csrc", "finetune_rays.hip"))
