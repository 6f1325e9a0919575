"""CPU (numpy + scikit-learn) against GPU (dtu_eval.hip) time of the DTU Chamfer evaluation's stages on a DTU-scale case.

The mesh: the project's marching cubes (ops.marching_cubes) on an analytic SDF of a ~300 mm bumpy ellipsoid at each lattice
resolution; the "STL" cloud: points on the same analytic surface with 0.2 mm noise.  Per resolution, the stages are timed on
both sides (sample, thin at 0.2 mm, d2s = thinned samples -> STL, s2d = STL -> thinned samples, both capped at 20 mm), the
outputs compared (they must be identical) and one JSON line printed.

    python scripts/time_dtu_eval.py [--resolutions 512 1024] [--stl_points 2500000] [--no_cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surf_amd import ops  # noqa: E402
from surf_amd.evaluation import dtu_eval as E  # noqa: E402

HALF = 160.0                                  # the lattice spans [-HALF, HALF] mm
AXES = np.array([150.0, 120.0, 100.0])


def _sdf(x, y, z):
    """An approximate SDF (unit gradient near the surface) of a bumpy ellipsoid of ~300 mm."""
    r = torch.sqrt((x / AXES[0]) ** 2 + (y / AXES[1]) ** 2 + (z / AXES[2]) ** 2)
    return (r - 1.0 - 0.03 * torch.sin(x / 9.0) * torch.sin(y / 7.0)) * 110.0


def _mesh(res, dev):
    ax = torch.linspace(-HALF, HALF, res, device=dev, dtype=torch.float32)
    u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
    for i in range(res):                                  # slab by slab: 1024^3 temporaries would not fit at once
        y, z = torch.meshgrid(ax, ax, indexing="ij")
        u[i] = -_sdf(ax[i].expand_as(y), y, z)
    v, t = ops.marching_cubes(u, 0.0)
    del u
    v = (v / (res - 1) * (2 * HALF) - HALF).to(torch.float32)          # a written mesh is float32
    return v.cpu().numpy(), t.cpu().numpy()


def _stl(n, seed=0):
    g = np.random.default_rng(seed)
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * AXES[None]
    for _ in range(3):                                    # a few Newton steps onto the bumpy surface
        t = torch.from_numpy(p).requires_grad_(True)
        f = _sdf(t[:, 0], t[:, 1], t[:, 2])
        (gr,) = torch.autograd.grad(f.sum(), t)
        p = (t - (f / (gr * gr).sum(1)).unsqueeze(1) * gr).detach().numpy()
    return (p + g.normal(0, 0.2, p.shape)).astype(np.float32)


def _t(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--stl_points", type=int, default=2_500_000)
    ap.add_argument("--thresh", type=float, default=0.2)
    ap.add_argument("--max_dist", type=float, default=20.0)
    ap.add_argument("--no_cpu", action="store_true", help="GPU stages only")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    stl = _stl(args.stl_points)
    stl_d = torch.from_numpy(stl.astype(np.float64)).to(dev)
    # warm-up: kernel loading and the allocator
    E.downsample_points_gpu(E.sample_mesh_points_gpu(*_mesh(32, dev), 2.0), 2.0, np.random.default_rng(0))
    for res in args.resolutions:
        v, t = _mesh(res, dev)
        gpu, cpu = {}, {}
        samples, gpu["sample"] = _t(lambda: E.sample_mesh_points_gpu(v, t, args.thresh))
        perm = torch.from_numpy(np.random.default_rng(0).permutation(samples.shape[0])).to(dev)

        def thin():
            s = samples[perm].contiguous()
            keep, rounds = ops.thin_points(s, args.thresh)
            return s[keep], rounds
        (down, rounds), gpu["thin"] = _t(thin)
        d2s, gpu["nn_d2s"] = _t(lambda: ops.nearest_dist_capped(down, stl_d, args.max_dist))
        s2d, gpu["nn_s2d"] = _t(lambda: ops.nearest_dist_capped(stl_d, down, args.max_dist))
        gpu["total"] = sum(gpu.values())
        rec = {"resolution": res, "vertices": int(len(v)), "triangles": int(len(t)), "samples": int(samples.shape[0]),
               "kept": int(down.shape[0]), "stl_points": int(len(stl)), "thin_rounds": rounds,
               "gpu_seconds": {k: round(x, 4) for k, x in gpu.items()}}
        if not args.no_cpu:
            import sklearn.neighbors as skln
            t0 = time.perf_counter()
            samples_c = E.sample_mesh_points(v, t, args.thresh)
            cpu["sample"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            down_c = E.downsample_points(samples_c, args.thresh, np.random.default_rng(0))
            cpu["thin"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            d2s_c = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=-1).fit(stl).kneighbors(down_c)[0][:, 0]
            cpu["nn_d2s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            s2d_c = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=-1).fit(down_c).kneighbors(stl)[0][:, 0]
            cpu["nn_s2d"] = time.perf_counter() - t0
            cpu["total"] = sum(cpu.values())
            rec["cpu_seconds"] = {k: round(x, 4) for k, x in cpu.items()}
            rec["speedup_total"] = round(cpu["total"] / gpu["total"], 1)

            def same(g, c):
                g = g.cpu().numpy()
                near = c < args.max_dist
                return bool(np.array_equal(g[near], c[near]) and np.isinf(g[~near]).all())
            rec["identical"] = {"sample": bool(np.array_equal(samples.cpu().numpy(), samples_c)),
                                "thin": bool(np.array_equal(down.cpu().numpy(), down_c)),
                                "nn_d2s": same(d2s, d2s_c), "nn_s2d": same(s2d, s2d_c)}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
