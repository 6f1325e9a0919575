#!/usr/bin/env python3
"""What feeding one training item costs, the host reader against the device-resident set, at the size a user trains:
1200 x 1600 files, img_hw 480 x 640, 5 views, 512 rays (confs/surf.conf).

    python scripts/time_train_loader.py [--items 80] [--hits 400] [--workers 8] [--cpus 16] [--step_ms 62] [--out profiles/train_loader.txt]

  host loader   get_loader(conf, "train", False, num_workers=W): items/s through the DataLoader, with and without the upload of
                the dictionary (runner.py's tocuda); one item single-threaded, and what `--cpus` CPUs could make of that
  device path   get_loader(..., device=...): items/s while every item misses the cache (files read, entries uploaded), items/s on
                hits (indices, cameras and pseudo points go up; train_batch.hip makes the batch), bytes uploaded per item each way,
                resident bytes

`--step_ms`: the training step the rates are set against (`training_step.ms_per_step` of `bench.py --full` on the same box): does a
path sustain one item per step?  The scene is synthetic, written in DTU's file formats into a temporary directory
(tests/golden/dtu_scene.write_dtu_scene): the cost depends on the file sizes, the working size and the ray count only.  Its point
cloud is tiny (3000 points, ascii); the host figures are a lower bound on a real scan's."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=80, help="items per host-loader measurement")
    ap.add_argument("--hits", type=int, default=400, help="items of the hit measurement")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--step_ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from surf_amd import conf
    from surf_amd.datasets import get_loader
    from surf_amd.finetune import to_device
    from tests.golden.dtu_scene import write_dtu_scene
    dev = torch.device("cuda:0")
    raw_hw, hw, views, rays = (1200, 1600), (480, 640), 5, 512                      # DTU's files, confs/surf.conf
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit(f"training items, files {raw_hw[0]} x {raw_hw[1]} -> img_hw {hw[0]} x {hw[1]}, {views} views, {rays} rays, "
         f"{len(os.sched_getaffinity(0))} CPUs available")
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "dtu")
        write_dtu_scene(root, n_views=views, hw=raw_hw)
        # the one scan listed often enough for an epoch of --items items: a DataLoader starts its workers once per epoch
        repeat = -(-args.items // views)
        dconf = conf.from_dict({"dataset_name": "DTUDataset", "data_dir": root, "scene": ["scan24"] * repeat, "light_idx": [3],
                                "num_src_view": views - 1, "total_views": views, "factor": 1.0, "interval_scale": 1,
                                "num_interval": 192, "img_hw": list(hw), "n_rays": rays})
        np.random.seed(0)
        torch.manual_seed(0)

        # ---- host reader ----
        _, _, plain = get_loader(dconf, "train", False, num_workers=0)
        t0 = time.perf_counter()
        for i in range(5):
            item = plain[i]
        one = (time.perf_counter() - t0) / 5
        item_bytes = sum(v.numel() * v.element_size() for v in item.values() if torch.is_tensor(v))
        emit(f"host reader, one item single-threaded: {one:.3f} s = {1 / one:.1f} items/s; {args.cpus} CPUs: {args.cpus / one:.1f} items/s; "
             f"the dictionary: {item_bytes / 1e6:.1f} MB")
        for upload in (False, True):                                                # the first pass runs before the GPU is touched
            if upload:
                assert torch.cuda.is_available(), "a timing needs the GPU"
                emit(torch.cuda.get_device_name(0))
                to_device(item, dev)
                torch.cuda.synchronize()
            loader, _, _ = get_loader(dconf, "train", False, num_workers=args.workers)
            it = iter(loader)
            next(it)                                                                # the workers are up
            t0, n = time.perf_counter(), 0
            for item in it:
                if upload:
                    item = to_device(item, dev)
                n += 1
            if upload:
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit(f"host loader, {args.workers} workers{', + upload of the dictionary' if upload else '':34s}: {n / dt:7.1f} items/s "
                 f"({1e3 * dt / n:.1f} ms an item, {n} items)")
            host_rate = n / dt

        # ---- device-resident set ----
        loader, _, ds = get_loader(dconf, "train", False, device=dev)
        n_scan_items = views                                                   # the other list entries are the same scan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_scan_items):
            ds[i]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        miss_bytes = ds.stats.uploaded_bytes / n_scan_items
        emit(f"device path, misses (first touch of every entry): {n_scan_items / dt:7.1f} items/s ({1e3 * dt / n_scan_items:.1f} ms an item), "
             f"{miss_bytes / 1e6:.2f} MB uploaded an item; misses {ds.stats.misses}, resident {ds.stats.resident_bytes / 1e6:.2f} MB "
             f"= {ds.stats.resident_bytes} bytes for {views} views, one light")
        for i in range(20):
            ds[i % n_scan_items]
        before, misses = ds.stats.uploaded_bytes, ds.stats.misses
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.hits):
            ds[i % n_scan_items]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        hit_rate = args.hits / dt
        emit(f"device path, hits                               : {hit_rate:7.1f} items/s ({1e3 * dt / args.hits:.2f} ms an item), "
             f"{(ds.stats.uploaded_bytes - before) / args.hits / 1e3:.1f} KB uploaded an item; new misses {ds.stats.misses - misses}")
        t0, n = time.perf_counter(), 0
        for item in loader:                                                         # the same through the DataLoader (num_workers = 0)
            n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        emit(f"device path, hits, through get_loader's DataLoader: {n / dt:7.1f} items/s ({1e3 * dt / n:.2f} ms an item, {n} items)")
    if args.step_ms:
        need = 1e3 / args.step_ms
        emit(f"a training step of {args.step_ms:.1f} ms consumes {need:.1f} items/s a rank: host loader {host_rate / need:.2f}x, "
             f"device hits {hit_rate / need:.1f}x of one rank; 8 ranks need {8 * need:.0f} items/s against {args.cpus / one:.1f} "
             f"from {args.cpus} CPUs of host reading ({args.cpus / one / (8 * need):.2f}x)")


if __name__ == "__main__":
    main()
