#!/usr/bin/env python3
"""The reference's second stage - per-scene fine-tuning (`python main.py --mode finetune`, runner.py:298-398, README "DTU
fine-tuning") - as ONE command:

    python scripts/finetune.py --conf <surf_finetune.conf> --resume ckpt.pth --scene scan24 --ref_view 23 \
        [--steps 5000 --mesh_resolution 512 --clean_mesh --vertex_colors --out_dir ./outputs] [--eval_dir <DTU eval data> --eval_device gpu]

(the conf is the reference's confs/surf_finetune.conf with its paths filled in: this repository ships no confs/ directory)

reader (surf_amd.datasets.DTUDatasetFinetune, the `finetune_dataset` block of the HOCON conf)
-> SuRF(conf.model).load_state_dict(ckpt["model"])            the generalisation checkpoint (runner.py:78-79)
   or, with --load_vol, SuRF.load_params_vol(ckpt)            a `get_params_vol` file of an earlier fine-tuning (runner.py:75-76)
-> SuRF.init_volumes(dataset.get_all_images())                the scene's volumes, built once (runner.py:86-91)
-> surf_amd.finetune.finetune                                 Adam, warm-up / cosine schedule, checkpoints, validation meshes
-> [evaluation.dtu_eval.evaluate_scan on the final PLY, --eval_dir]
-> one JSON line: {"scene", "ref_view", "steps", "loss" (per step), "psnr", "checkpoints", "meshes", "ms_per_step", ...}.

The batch of a step is made on the device (finetune_rays.hip: 12 KB of drawn indices go up per step); --host_batch makes it on the
host and uploads it whole, as the reference does.  Outputs land in <out_dir>/<scene>/view<ref_view>/ (runner.py:44).
Needs external data (a DTU tree with the pseudo depths / points, a checkpoint): tests/test_finetune_gpu.py runs it on a synthetic
scene written in DTU's file formats.  Measurement harness, not a control plane: no TensorBoard, no progress bar."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--conf", required=True, help="HOCON conf with `model`, `finetune_dataset` and `train` blocks (the reference's confs/surf_finetune.conf)")
    ap.add_argument("--resume", required=True, help="generalisation checkpoint (`model` = state_dict), or with --load_vol a get_params_vol file")
    ap.add_argument("--load_vol", action="store_true", help="--resume holds per-scene volumes (SuRF.get_params_vol): no init_volumes")
    ap.add_argument("--data_dir", default=None, help="overrides finetune_dataset.data_dir")
    ap.add_argument("--scene", default=None, help="overrides finetune_dataset.scene")
    ap.add_argument("--ref_view", type=int, default=None, help="overrides finetune_dataset.ref_view")
    ap.add_argument("--steps", type=int, default=None, help="overrides train.epochs")
    ap.add_argument("--mesh_resolution", type=int, default=512)
    ap.add_argument("--clean_mesh", action="store_true", help="clean the validation meshes with the validation item's masks")
    ap.add_argument("--clean_backend", default="host", choices=["host", "device"])
    ap.add_argument("--vertex_colors", action="store_true",
                    help="also write per-vertex normals and blended colours into the validation PLYs (geometry unchanged)")
    ap.add_argument("--out_dir", default=None, help="overrides general.base_exp_dir")
    ap.add_argument("--host_batch", action="store_true", help="make the batches on the host and upload them (the reference's path)")
    ap.add_argument("--eval_dir", default=None, help="DTU evaluation data: score the final PLY (scripts/dtu_chamfer.py's evaluator)")
    ap.add_argument("--eval_device", default="cpu", choices=["cpu", "gpu"])
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--logit_override", default=None, choices=["sphere"],
                    help="(tests) replace the U-Nets' matching logits by a sphere-concentrated field, as an untrained model needs")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def run(args, state=None):
    """Returns the JSON record.  state (dict, tests): receives the live `model`, `dataset` and the `finetune` result."""
    from surf_amd import conf as C
    from surf_amd import finetune as FT
    from surf_amd import synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.losses import Loss
    from surf_amd.surf import SuRF

    dev = torch.device(args.device)
    cfg = C.parse_file(args.conf)
    dconf = cfg["finetune_dataset"]
    for key in ("data_dir", "scene", "ref_view"):
        if getattr(args, key) is not None:
            dconf[key] = getattr(args, key)
    scene, ref_view = dconf.get_string("scene"), dconf.get_int("ref_view")
    base = args.out_dir if args.out_dir is not None else cfg.get("general.base_exp_dir", "./outputs")
    out_dir = os.path.join(base, scene, f"view{ref_view}")                                      # runner.py:44
    os.makedirs(out_dir, exist_ok=True)

    torch.manual_seed(args.seed)
    dataset = get_loader(dconf, "finetune", False)                                              # runner.py:63
    model = SuRF(cfg["model"])
    if args.load_vol:
        model = model.to(dev)
        model.load_params_vol(args.resume, dev)                                                 # runner.py:75-76
    else:
        ckpt = torch.load(args.resume, map_location="cpu")
        model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt, strict=True)          # runner.py:78-79
        model = model.to(dev)
        if args.logit_override == "sphere":
            model.logit_override = synthetic.sphere_logit
        if not args.host_batch:
            dataset.to(dev)
        model.eval()
        init = dataset.get_all_images()
        model.init_volumes(init if not args.host_batch else FT.to_device(init, dev))            # runner.py:86-91
    isurf0 = [p.detach().clone() for p in model.implicit_surface.parameters()]
    vols0 = [p.detach().clone() for p in model.volumes]
    loss_fn = Loss(cfg["train.loss"]).to(dev)
    res = FT.finetune(model, dataset, loss_fn, cfg, out_dir, steps=args.steps, device=dev, on_device=not args.host_batch,
                      mesh_resolution=args.mesh_resolution, clean_mesh=args.clean_mesh, clean_backend=args.clean_backend,
                      vertex_colors=args.vertex_colors)
    moved = {"implicit_surface": max(float((p.detach() - q).abs().max()) for p, q in zip(model.implicit_surface.parameters(), isurf0)),
             "volumes": max(float((p.detach() - q).abs().max()) for p, q in zip(model.volumes, vols0))}
    rec = {"scene": scene, "ref_view": ref_view, "views": [int(v) for v in dataset.all_views], "steps": res["steps"],
           "loss": res["loss"], "color_loss": res["color_loss"], "psnr": res["psnr"], "val": res["val"],
           "checkpoints": res["checkpoints"], "meshes": res["meshes"], "ms_per_step": res["ms_per_step"],
           "ms_per_batch": res["ms_per_batch"], "batch": "host" if args.host_batch else "device",
           "uploaded_bytes": int(dataset.uploaded_bytes), "max_parameter_change": moved, "resume": args.resume,
           "load_vol": bool(args.load_vol), "voxels": [int(v.shape[0]) for v in model.volumes]}
    if args.eval_dir is not None:
        from surf_amd.evaluation import dtu_eval
        scan = int(scene[4:])
        d2s, s2d, overall = dtu_eval.evaluate_scan(res["meshes"][-1], args.eval_dir, scan, downsample_density=args.downsample_density,
                                                   rng=np.random.default_rng(0), device=args.eval_device)
        rec.update(d2s=d2s, s2d=s2d, chamfer=overall)
    with open(os.path.join(out_dir, "finetune.json"), "w") as f:
        json.dump(rec, f)
    if state is not None:
        state.update(model=model, dataset=dataset, finetune=res, out_dir=out_dir)
    return rec


def main(argv=None):
    print(json.dumps(run(parse_args(argv))))


if __name__ == "__main__":
    main()
