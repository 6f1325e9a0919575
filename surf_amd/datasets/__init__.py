"""Dataset readers: the `ipts` contract of SuRF.forward from MVSNet-format scenes."""
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, DistributedSampler, RandomSampler, SequentialSampler

from .dtu import DTUDataset, TanksDataset
from .dtu_finetune import DTUDatasetFinetune
from .dtu_resident import DTUDeviceTrainSet

DATASETS = {"DTUDataset": DTUDataset, "TanksDataset": TanksDataset, "DTUDatasetFinetune": DTUDatasetFinetune}


def collect_fn(data):
    return data[0]


def get_loader(conf, mode, distributed, num_workers=8, device=None):
    """datasets/__init__.py:16-43: batch size 1 (one scene + reference view per item), DistributedSampler under DDP;
    mode "finetune": the dataset itself (runner.py:63), whose get_random_rays / get_rays_at make the batches.
    device (a GPU; default None = the host reader as it is): in mode "train" a DTUDataset is wrapped in a DTUDeviceTrainSet -
    the loader then yields device-made batches from the device-resident cache, in this process (num_workers=0), and the third
    value returned is that set (its `dataset` is the host reader, `stats` the cache's counters)."""
    name = conf.get_string("dataset_name")
    if name not in DATASETS:
        raise NotImplementedError(f"dataset_name {name!r}: surf_amd ships {sorted(DATASETS)} "
                                  "(the reference's BlendedMVS / ETH3D readers and its NeuS-format finetune reader are not built)")
    dataset = DATASETS[name](conf, mode)
    if mode == "finetune":
        return dataset
    if device is not None and mode == "train" and isinstance(dataset, DTUDataset):
        dataset, num_workers = DTUDeviceTrainSet(dataset, device), 0
    if distributed:
        sampler = DistributedSampler(dataset, num_replicas=dist.get_world_size(), rank=dist.get_rank())
    else:
        sampler = RandomSampler(dataset) if mode == "train" else SequentialSampler(dataset)
    loader = DataLoader(dataset, 1, sampler=sampler, num_workers=num_workers, drop_last=(mode == "train"), pin_memory=False,
                        collate_fn=collect_fn)
    return loader, sampler, dataset
