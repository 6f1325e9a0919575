"""Dense vs narrow-band mesh extraction (ImplicitSurface.extract_geometry, render.mesh_extraction) on the bench scene: one JSON line.

Per configuration (dense 512 / 1024, band 512 / 1024 / 2048): SDF ms, classify / grow ms (band), marching-cubes ms and total ms
from HIP events (the median of --reps timed calls after one warm-up call), points evaluated, bricks seeded / grown / evaluated,
growth iterations, peak device memory, mesh size.  Also the maximum finite-difference gradient norm of u = -sdf on the dense
512^3 lattice (the evidence for render.mesh_band_margin's default), over the whole box and near the surface.

usage: python scripts/time_mesh_band.py [--reps 3] [--precision bf16x3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def scene_and_model(precision):
    from bench import model_conf
    from surf_amd import synthetic
    from surf_amd.implicit_surface import ImplicitSurface, _LatticeScene
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = ImplicitSurface(model_conf([64, 32, 16, 16], precision)).to(dev)
    vols, tabs, _ = synthetic.sphere_pyramid(88, dev)
    return model, _LatticeScene(vols[::-1], tabs[::-1])


def one(model, scene, res, mode, reps):
    bmin, bmax = torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3)
    rows = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        model.kernel_events = []
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v, t = model.extract_geometry(None, None, bmin, bmax, res, 0.0, scene=scene, mesh_extraction=mode)
        b.record()
        torch.cuda.synchronize()
        ev = model.kernel_events
        model.kernel_events = None
        total = a.elapsed_time(b)
        sdf = sum(x.elapsed_time(y) for n, x, y in ev if n in ("sdf_grid", "band_sdf"))
        mc = sum(x.elapsed_time(y) for n, x, y in ev if n == "band_mc") if mode == "band" else total - sdf
        rows.append({"total_ms": total, "sdf_ms": sdf, "mc_ms": mc, "grow_ms": total - sdf - mc if mode == "band" else 0.0,
                     "peak_mb": (torch.cuda.max_memory_allocated() - base) / 2 ** 20, "vertices": len(v), "triangles": len(t)})
    rows = rows[1:]
    med = {k: sorted(r[k] for r in rows)[len(rows) // 2] for k in rows[0]}
    med["total_ms_all"] = [round(r["total_ms"], 2) for r in rows]
    if mode == "band":
        _, _, stats = model.sdf_band(scene, bmin, bmax, res)
        med.update(stats)
    else:
        med["points_evaluated"] = res ** 3
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in med.items()}


def gradient_bound(model, scene, res=512):
    """max |grad u| by forward differences on the dense lattice: everywhere, and where |u| < 0.05 (near the surface)."""
    bmin, bmax = torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3)
    with torch.no_grad():
        u = model.sdf_grid(scene, bmin, bmax, res)
        h = 2.0 / (res - 1)
        gx = (u[1:, :-1, :-1] - u[:-1, :-1, :-1]) / h
        g2 = gx * gx
        del gx
        gy = (u[:-1, 1:, :-1] - u[:-1, :-1, :-1]) / h
        g2 += gy * gy
        del gy
        gz = (u[:-1, :-1, 1:] - u[:-1, :-1, :-1]) / h
        g2 += gz * gz
        del gz
        g = g2.sqrt_()
        near = u[:-1, :-1, :-1].abs() < 0.05
        return {"grad_max": round(float(g.max()), 4), "grad_max_near_surface": round(float(g[near].max()), 4), "res": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    model, scene = scene_and_model(args.precision)
    out = {"what": "extract_geometry on the bench scene (sphere_pyramid(88), random-init SDF network), HIP events, median of "
                   f"{args.reps} calls after a warm-up", "precision": args.precision,
           "device": torch.cuda.get_device_name(0), "margin": model.mesh_band_margin}
    for mode, res in (("dense", 512), ("band", 512), ("dense", 1024), ("band", 1024), ("band", 2048)):
        out[f"{mode}_{res}"] = one(model, scene, res, mode, args.reps)
    bmin, bmax = torch.tensor([-1.0] * 3), torch.tensor([1.0] * 3)
    out["band_512_margin0"] = model.sdf_band(scene, bmin, bmax, 512, margin=0.0)[2]
    out["gradient"] = gradient_bound(model, scene)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
