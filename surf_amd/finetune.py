"""Per-scene fine-tuning: the reference's second stage (runner.py:298-398, confs/surf_finetune.conf) as a function.

A model whose volumes are built (`SuRF.init_volumes(dataset.get_all_images())` or `load_params_vol`) is optimised on the three
views of one scene: Adam over `get_optim_params` (the implicit surface + the per-scene feature rows), the reference's warm-up /
cosine schedule, one view per step in a permutation redrawn every `num_views` steps, `training.finetune_step` per step,
checkpoints of `get_params_vol()` and validation renders + world-frame meshes at the conf's frequencies.

The batch comes from `surf_amd.datasets.DTUDatasetFinetune`: with on_device=True (default) the dataset lives on the device and a
step uploads 12 KB of drawn indices (finetune_rays.hip); with on_device=False it is the reference's way - the batch is made on
the host and uploaded whole, three full-size images included - kept for comparison (scripts/time_finetune_rays.py).  Both
consume the CPU generator alike, so a seeded run draws the same pixels either way.

Not here: TensorBoard, progress bars, the runner's code backup.
"""
import os
import time

import numpy as np
import torch
from PIL import Image

from . import mesh_io, training


def warmup_cosine_multiplier(step, total_steps, warmup, alpha):
    """utils/scheduler.py:6, one float64 formula: linear 0.1 -> 1 over `warmup` steps, then half a cosine from 1 down to alpha."""
    if step < warmup:
        return 0.1 + 0.9 * step / warmup
    return (np.cos(np.pi * (step - warmup) / (total_steps - warmup)) + 1.0) * 0.5 * (1 - alpha) + alpha


def warmup_cosine_lr(optimizer, total_steps, warmup=0.2, alpha=0.1):
    """utils/scheduler.py:5-8 `WarmupCosineLR`: a LambdaLR of warmup_cosine_multiplier, stepped with the step number."""
    return torch.optim.lr_scheduler.LambdaLR(optimizer, lambda step: warmup_cosine_multiplier(step, total_steps, warmup, alpha))


def cos_anneal_ratio(step, anneal_end):
    """runner.py:415-419."""
    return 1.0 if anneal_end == 0.0 else float(min(1.0, step / anneal_end))


def to_device(batch, device):
    """runner.py's tocuda: every tensor of the dictionary."""
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}


def psnr(pred, target):
    """runner.py:325."""
    return float(20.0 * torch.log10(1.0 / ((pred - target) ** 2).mean().sqrt()))


def save_checkpoint(path, step, model, optimizer, scheduler):
    """runner.py:346-355: the per-scene parameters (`get_params_vol`), not the state_dict."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"epoch": step, "model": model.get_params_vol(), "optimizer": optimizer.state_dict(),
                "lr_scheduler": scheduler.state_dict()}, path)


def validate(model, dataset, out_dir, step, device, mesh_resolution=512, clean_mesh=False, clean_backend="host", val_vid=0,
             vertex_colors=False):
    """runner.py:357-396: render the validation lattice of view `val_vid`, extract the mesh, write the world-frame PLY and the
    image / normal / depth arrays.  Returns {"mesh", "psnr", "color_loss", "triangles", "outputs"}.  vertex_colors (ours): the
    PLY also carries per-vertex normals and blended colours (SuRF.vertex_attributes on the final - cleaned - vertex set, before
    scale_mat); positions and faces are the same."""
    item = dataset.get_rays_at(val_vid)
    inputs = to_device(item, device)
    inputs["mesh_resolution"] = mesh_resolution
    if vertex_colors:
        inputs["keep_scene"] = True
    was_training = model.training
    with torch.no_grad():
        out = model("val", inputs, cos_anneal_ratio=1.0)
    model.train(was_training)
    v, t = np.asarray(out["vertices"]), np.asarray(out["triangles"])
    if clean_mesh and len(t):
        # the reference passes the TRAINING batch's inputs["masks"] here (runner.py:376), a key that batch does not have; the
        # masks that belong to this mesh's views are the validation item's
        from .evaluation import clean_mesh as CM
        v, t = CM.clean_mesh(v, t, item["masks"], item["intrs"], item["c2ws"], device=str(torch.device(device)), backend=clean_backend)
    mesh_path = os.path.join(out_dir, "meshes", "{}_step{}.ply".format(item["scene"], step))
    os.makedirs(os.path.dirname(mesh_path), exist_ok=True)
    attrs = model.vertex_attributes(v) if vertex_colors and len(v) else {}
    mesh_io.export_mesh(mesh_path, v, t, item["scale_mat"].cpu(), normals=attrs.get("normals"), colors=attrs.get("colors"))
    for sub, arr in (("val_img", out["img_fine"]), ("val_normal", out["normal_img"])):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        Image.fromarray(arr.astype(np.uint8)).save(os.path.join(out_dir, sub, "{}_step{}.png".format(val_vid, step)))
    for sub, arr in (("val_render_depth", out["render_depth"]), ("val_sdf_depth", out["sdf_depth"])):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        np.save(os.path.join(out_dir, sub, "{}_step{}.npy".format(val_vid, step)), arr)       # (the reference colour-maps them)
    color, target = out["color_fine"].cpu(), item["color"].cpu()
    return {"mesh": mesh_path, "psnr": psnr(color, target), "color_loss": float((color - target).abs().mean()),
            "triangles": int(len(t)), "outputs": out}


def finetune(model, dataset, loss_fn, conf, out_dir, steps=None, device="cuda:0", on_device=True, mesh_resolution=512,
             clean_mesh=False, clean_backend="host", validate_mesh=True, vertex_colors=False):
    """runner.py:298-398.  model: a has_vol SuRF on `device`; dataset: DTUDatasetFinetune; conf: the whole conf (its `train`
    block: lr_conf, epochs, anneal_end, warmup, alpha, save_freq, val_freq).  steps overrides train.epochs.  Returns
    {"loss", "color_loss", "psnr" (per step), "checkpoints", "meshes", "val" (per validation: psnr, color_loss), "ms_per_step",
    "ms_per_batch", "steps", "on_device", "optimizer", "lr_scheduler"}.  validate_mesh=False skips the validations (timing runs);
    vertex_colors: the validation PLYs carry normals and colours (validate)."""
    device = torch.device(device)
    tr = conf["train"]
    total = int(steps) if steps is not None else tr.get_int("epochs")
    save_freq, val_freq = tr.get_float("save_freq"), tr.get_float("val_freq")
    anneal_end = tr.get_float("anneal_end", default=0.0)
    if not model.has_vol:
        raise ValueError("finetune: the model has no volumes (SuRF.init_volumes(dataset.get_all_images()) or load_params_vol first)")
    dataset.to(device if on_device else "cpu")
    optimizer = torch.optim.Adam(model.get_optim_params(lr_conf=tr["lr_conf"]))
    scheduler = warmup_cosine_lr(optimizer, total, tr.get_float("warmup"), tr.get_float("alpha"))
    model.train()
    hist = {"loss": [], "color_loss": [], "psnr": []}
    checkpoints, meshes, vals = [], [], []
    t_batch = t_steps = 0.0
    image_perm = torch.randperm(dataset.num_views)
    for step in range(total):
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        inputs = dataset.get_random_rays(image_perm[step % len(image_perm)])
        if not on_device:
            inputs = to_device(inputs, device)
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        scalars, outputs = training.finetune_step(model, inputs, inputs, loss_fn, optimizer, cos_anneal_ratio(step, anneal_end), step,
                                                  return_outputs=True)
        scheduler.step(step)
        hist["loss"].append(scalars["loss"])                     # (float(): the step has finished on the device)
        hist["color_loss"].append(scalars["color_loss"])
        hist["psnr"].append(psnr(outputs["color_fine"].detach(), inputs["color"]))
        t2 = time.perf_counter()
        t_batch += t1 - t0
        t_steps += t2 - t0
        if (step + 1) % len(image_perm) == 0:
            image_perm = torch.randperm(dataset.num_views)
        last = step + 1 >= total
        if (step + 1) % save_freq == 0 or last:
            checkpoints.append(os.path.join(out_dir, "checkpoints", "model_{:0>3}.ckpt".format(step)))
            save_checkpoint(checkpoints[-1], step, model, optimizer, scheduler)
        if validate_mesh and ((step + 1) % val_freq == 0 or last):
            val = validate(model, dataset, out_dir, step, device, mesh_resolution, clean_mesh, clean_backend,
                           vertex_colors=vertex_colors)
            meshes.append(val["mesh"])
            vals.append({"step": step, "psnr": val["psnr"], "color_loss": val["color_loss"], "triangles": val["triangles"]})
    n = max(total, 1)
    return dict(hist, checkpoints=checkpoints, meshes=meshes, val=vals, ms_per_step=1e3 * t_steps / n, ms_per_batch=1e3 * t_batch / n,
                steps=total, on_device=bool(on_device), optimizer=optimizer, lr_scheduler=scheduler)
