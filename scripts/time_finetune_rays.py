#!/usr/bin/env python3
"""What making the batch of a fine-tuning step costs, the reference's way against the device path, at the size a user runs:
1200 x 1600 images, 512 rays (confs/surf_finetune.conf).

    python scripts/time_finetune_rays.py [--steps 200] [--hw 1200 1600] [--rays 512] [--step_dim 32] [--out profiles/finetune_rays.txt]

  (a) host     DTUDatasetFinetune.get_random_rays on the host + the upload of every tensor of the dictionary (runner.py:310-311):
               `imgs` alone is 3 x 3 x H x W fp32
  (a') host    (a) with `imgs` made NCHW-contiguous on the host first: separates what the model pays for the permuted view the
               reference uploads from what the copy costs
  (b) device   the same reader after .to(device): 12 KB of drawn indices go up, finetune_rays.hip makes the batch

Same process, same device, the ways taking turns call by call after a warm-up; wall time around a device synchronise; median and
quartiles.  Then the whole fine-tuning step (batch + surf_amd.training.finetune_step) each way on a model whose volumes are built
from the same scene (base volume `--step_dim`^3, sphere-concentrated logits as an untrained model needs).  The scene is synthetic
(written in DTU's file formats into a temporary directory): the cost of a batch depends on the image size and the ray count only."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _quartiles(ms):
    q = statistics.quantiles(ms, n=4)
    return f"median {statistics.median(ms):8.3f} ms   quartiles {q[0]:8.3f} .. {q[2]:8.3f}   min {min(ms):8.3f}   n = {len(ms)}"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--hw", type=int, nargs=2, default=[1200, 1600])
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--step_dim", type=int, default=32, help="base volume dim of the whole-step model (0: skip the whole step)")
    ap.add_argument("--step_steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from bench import surf_conf
    from surf_amd import conf, synthetic
    from surf_amd import finetune as FT
    from surf_amd.datasets import get_loader
    from surf_amd.losses import Loss
    from surf_amd.surf import SuRF
    from surf_amd.training import finetune_step
    from tests.golden.dtu_finetune_scene import add_finetune_folders
    from tests.golden.dtu_scene import write_dtu_scene
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    H, W = args.hw
    lines = [f"fine-tuning batch, {H} x {W}, {args.rays} rays, {args.steps} steps each, taking turns, {torch.cuda.get_device_name(0)}"]

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "dtu")
        write_dtu_scene(root, n_views=3, hw=(H, W))
        add_finetune_folders(root, n_views=3, hw=(H, W))
        dconf = conf.from_dict({"dataset_name": "DTUDatasetFinetune", "data_dir": root, "scene": "scan24", "ref_view": 1, "n_rays": args.rays,
                                "val_res_level": 4, "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [H, W]})
        host = get_loader(dconf, "finetune", False)
        device = get_loader(dconf, "finetune", False).to(dev)

    def host_batch(vid):
        return FT.to_device(host.get_random_rays(vid), dev)

    def host_batch_contiguous(vid):
        """(a) with `imgs` laid out NCHW-contiguous on the host before the upload (the reference uploads the permuted view)."""
        b = host.get_random_rays(vid)
        b["imgs"] = b["imgs"].contiguous()
        return FT.to_device(b, dev)

    def device_batch(vid):
        return device.get_random_rays(vid)

    ways = (("host", host_batch), ("host_nchw", host_batch_contiguous), ("device", device_batch))

    def timed(fn, vid):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(vid)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    times = {name: [] for name, _ in ways}
    for i in range(args.warmup + args.steps):
        vid = torch.tensor(i % 3)
        for name, fn in ways[i % 3:] + ways[:i % 3]:                  # rotate the order call by call
            ms, _ = timed(fn, vid)
            if i >= args.warmup:
                times[name].append(ms)
    up = sum(v.numel() * v.element_size() for v in host.get_random_rays(torch.tensor(0)).values() if torch.is_tensor(v))
    emit(f"(a) host batch + upload ({up / 1e6:.1f} MB a step)   {_quartiles(times['host'])}")
    emit(f"(a') the same, imgs NCHW-contiguous on the host   {_quartiles(times['host_nchw'])}")
    emit(f"(b) device batch ({(2 * args.rays + 2048) * 4 / 1e3:.1f} KB a step)      {_quartiles(times['device'])}")
    emit(f"(a) / (b) = {statistics.median(times['host']) / statistics.median(times['device']):.1f}")
    if args.step_dim <= 0:
        return
    # ---- the whole step each way: one model per way from one state, each fed by its own reader ----
    c = conf.from_dict({"model": surf_conf(base_dim=args.step_dim), "train": {"lr_conf": {"mlp_lr": 5e-4, "vol_lr": [1e-1, 1e-2, 1e-2, 1e-3]}}})
    loss_fn = Loss(conf.from_dict({"color_weight": 1.0, "sparse_weight": 0.01, "igr_weight": 0.1, "sparse_scale_factor": 100, "mfc_weight": 1.0,
                                   "smooth_weight": 0.0001, "tv_weight": 0.0, "depth_weight": 0.0, "ptloss_weight": 1.0,
                                   "pseudo_auxi_depth_weight": 1.0, "pseudo_sdf_weight": 1.0, "stage_weights": [0.25, 0.5, 0.75, 1.0],
                                   "pseudo_depth_weight": 1.0})).to(dev)
    runs = {}
    for name, fn in ways:
        torch.manual_seed(0)
        m = SuRF(c["model"]).to(dev).eval()
        m.logit_override = synthetic.sphere_logit
        m.init_volumes(device.get_all_images())
        m.train()
        runs[name] = (m, torch.optim.Adam(m.get_optim_params(lr_conf=c["train.lr_conf"])), fn)
    steps = {name: [] for name, _ in ways}
    for i in range(5 + args.step_steps):
        for name, _ in ways[i % 3:] + ways[:i % 3]:
            m, opt, fn = runs[name]

            def whole(vid, m=m, opt=opt, fn=fn):
                b = fn(vid)
                return finetune_step(m, b, b, loss_fn, opt, 1.0, i)

            ms, _ = timed(whole, torch.tensor(i % 3))
            if i >= 5:
                steps[name].append(ms)
    emit(f"whole step, volumes {args.step_dim}^3 .. {8 * args.step_dim}^3, {[int(v.shape[0]) for v in runs['host'][0].volumes]} voxels:")
    emit(f"    host batch                    {_quartiles(steps['host'])}")
    emit(f"    host batch, imgs contiguous   {_quartiles(steps['host_nchw'])}")
    emit(f"    device batch                  {_quartiles(steps['device'])}")


if __name__ == "__main__":
    main()
