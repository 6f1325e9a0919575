#!/usr/bin/env python3
"""Golden items of the REFERENCE's fine-tuning reader and learning-rate schedule: generated in the build container by importing
the reference's datasets/dtu_finetune.py and utils/scheduler.py and running THEIR `DTUDatasetFinetune.get_all_images`,
`get_random_rays` (views 0, 1, 2, each under torch.manual_seed(SEEDS["torch"])), `get_rays_at(0)` on the synthetic scene of
tests/golden/dtu_finetune_scene.py, and THEIR `WarmupCosineLR`'s multiplier at a dozen steps of two schedules.  Only data is
committed (tests/golden/finetune_items.npz).

cv2 and plyfile are absent from this image and stood in for by the stand-ins of tests/golden/make_golden_dataset.py (see there for
what that leaves unpinned).  Python lists of the dictionaries (`view_ids`) are stored as int64 arrays, strings as key names."""
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import dtu_finetune_scene as S  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden.make_golden_dataset import _cv2_stub, _plyfile_stub  # noqa: E402


def main():
    sys.modules["cv2"] = _cv2_stub()
    sys.modules["plyfile"] = _plyfile_stub()
    sys.modules["lmdb"] = types.ModuleType("lmdb")
    sys.path.insert(0, G.REF)
    from datasets.dtu_finetune import DTUDatasetFinetune
    from utils.scheduler import WarmupCosineLR
    out = {}

    def store(tag, item):
        for k, v in item.items():
            if torch.is_tensor(v):
                out[f"{tag}/{k}"] = v
            elif isinstance(v, list):
                out[f"{tag}/{k}"] = torch.tensor([int(x) for x in v], dtype=torch.int64)
            elif isinstance(v, str):
                out[f"{tag}/str/{k}/{v}"] = torch.zeros(1)
            else:
                raise TypeError((k, type(v)))

    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "dtu")
        S.write_finetune_scene(root)
        ds = DTUDatasetFinetune(G.Conf(dict(S.FINETUNE_CONF, data_dir=root)), "finetune")
        assert ds.all_views == [2, 0, 1], ds.all_views
        store("all_images", ds.get_all_images())
        for v in range(3):
            torch.manual_seed(S.SEEDS["torch"])
            store(f"random_rays{v}", ds.get_random_rays(torch.tensor(v)))
        store("rays_at0", ds.get_rays_at(0))
    for name, (total, warmup, alpha) in S.SCHEDULES.items():
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        sched = WarmupCosineLR(opt, total, warmup, alpha)
        out[f"schedule/{name}"] = torch.tensor([float(sched.lr_lambdas[0](s)) for s in S.SCHEDULE_STEPS[name]], dtype=torch.float64)
    G.ONLY.clear()
    G.npz("finetune_items.npz", **out)


if __name__ == "__main__":
    main()
