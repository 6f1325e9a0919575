"""Per-vertex normals and colours (ImplicitSurface.vertex_attributes) on the bench scene's 512^3 mesh: one JSON line.

The scene is bench.py's scene_timing one (SuRF.forward("val"): FPN, 4-stage volume build, full-resolution render, the 512^3
lattice, marching cubes); `scene_ms` is timed the same way (wall clock, median of the last three of five calls) for scale.  Then
--reps calls of vertex_attributes on that mesh's vertices (numpy in, numpy out, wall clock, after one warm-up call): the median,
and from HIP events of the median call the split between the two new stages (vertex_points, vertex_finish) and the two reused
kernels (the SDF gradient kernel, the blend kernel); the rest of the call is the upload of the vertices and the copy back.

usage: python scripts/time_vertex_attrs.py [--reps 5] [--mesh_resolution 512]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mesh_resolution", type=int, default=512)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--base_dim", type=int, default=88)
    args = ap.parse_args()
    from bench import surf_conf
    from surf_amd import conf, synthetic
    from surf_amd.surf import SuRF
    dev = torch.device("cuda:0")
    H, W, nv = args.height, args.width, args.views
    torch.manual_seed(0)
    model = SuRF(conf.from_dict(surf_conf(args.base_dim))).eval().to(dev)
    model.logit_override = synthetic.sphere_logit
    intrs, c2ws, near_fars = synthetic.ring_cameras(nv, H, W)
    rays_o, rays_d = synthetic.pixel_rays(intrs[0], c2ws[0], H, W, 1, dev)
    ipts = {"imgs": synthetic.procedural_images(nv, H, W, 0, dev), "intrs": intrs.to(dev), "c2ws": c2ws.to(dev),
            "near_fars": near_fars.to(dev), "near": near_fars[0, 0].reshape(1, 1).to(dev), "far": near_fars[0, 1].reshape(1, 1).to(dev),
            "rays_o": rays_o, "rays_d": rays_d, "bound_min": torch.tensor([-1.0] * 3), "bound_max": torch.tensor([1.0] * 3),
            "hw": (H, W), "mesh_resolution": args.mesh_resolution, "keep_scene": True}
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model("val", ipts, 1.0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    v = out["vertices"]
    isurf = model.implicit_surface
    calls = []
    for it in range(args.reps + 1):
        torch.cuda.synchronize()
        isurf.kernel_events = []
        t0 = time.perf_counter()
        attrs = model.vertex_attributes(v)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ev, isurf.kernel_events = isurf.kernel_events, None
        parts = {}
        for name, a, b in ev:
            parts[name] = parts.get(name, 0.0) + a.elapsed_time(b)
        calls.append({"call_ms": wall, **{k + "_ms": x for k, x in parts.items()}})
    calls = sorted(calls[1:], key=lambda r: r["call_ms"])
    med = calls[len(calls) // 2]
    new = med["vertex_points_ms"] + med["vertex_finish_ms"]
    print(json.dumps({
        "what": f"vertex_attributes on the bench scene's {args.mesh_resolution}^3 mesh, numpy in -> numpy out, wall clock; the median "
                f"of {args.reps} calls after a warm-up, its stages by HIP events",
        "device": torch.cuda.get_device_name(0), "vertices": int(len(v)), "chunk_rows": isurf.vertex_chunk_rows(dev, nv),
        "seen_share": round(float((attrs["n_valid"] > 0).mean()), 4),
        **{k: round(x, 3) for k, x in med.items()}, "calls_ms": [round(r["call_ms"], 2) for r in calls],
        "new_stages_ms": round(new, 3), "new_stages_share_of_call": round(new / med["call_ms"], 5),
        "scene_ms": round(sorted(ms[2:])[1], 2), "call_share_of_scene": round(med["call_ms"] / sorted(ms[2:])[1], 4)}))


if __name__ == "__main__":
    main()
