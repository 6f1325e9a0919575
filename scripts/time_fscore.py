"""GPU (fscore.hip) against host (numpy + scikit-learn) time of the Tanks and Temples evaluation's stages on synthetic clouds at
the benchmark's scale, and what the dense nearest-neighbour table costs on a surface-distributed cloud in a 20 m box.

The "scan": n points at random (x, y) on a bumpy surface patch of 20 m x 20 m, about 4 m high; the "reconstruction": the same
number of other points of that surface under a small rigid perturbation (0.3 degrees, 2 cm) with 1 tau / 4 of noise.  tau = 2 x the
mean point spacing, so that the tau / 2 voxels hold about one point each, as the benchmark's scenes do at their own tau.  The crop
volume is an octagon that cuts the corners off the patch.  Per size the stages are timed with HIP events (median of --runs) and,
with --cpu, on the host path (wall time, once); one JSON line per size.

    python scripts/time_fscore.py [--sizes 200000 2000000 20000000] [--cpu_sizes 200000 2000000] [--runs 5]
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
from surf_amd.evaluation import fscore as F  # noqa: E402

SIDE = 20.0


def _surface(x, y):
    return 1.5 * np.sin(0.9 * x + 0.3) * np.cos(0.7 * y) + 0.02 * x * y + 0.3 * np.sin(3.1 * x) * np.sin(2.7 * y)


def _clouds(n, tau, seed=0):
    g = np.random.default_rng(seed)
    x, y = g.uniform(0, SIDE, n), g.uniform(0, SIDE, n)
    gt = np.stack([x, y, _surface(x, y)], axis=1)
    x, y = g.uniform(0, SIDE, n), g.uniform(0, SIDE, n)
    pred = np.stack([x, y, _surface(x, y)], axis=1) + g.normal(0, tau / 4, (n, 3))
    a = np.deg2rad(0.3)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    c = np.array([SIDE / 2, SIDE / 2, 0])
    pred = (pred - c) @ R.T + c + np.array([0.02, -0.01, 0.015])       # the reconstruction's frame: off by a small motion
    return pred, gt


def _crop():
    c, s = SIDE / 2, SIDE / 2 * 0.98
    k = s * 0.6
    poly = [(c - k, c - s), (c + k, c - s), (c + s, c - k), (c + s, c + k), (c + k, c + s), (c - k, c + s), (c - s, c + k), (c - s, c - k)]
    return F.CropVolume("Z", -10.0, 10.0, np.array([[u, v, 0.0] for u, v in poly]))


def _events(fn, runs):
    """Median HIP-event time of fn in ms over `runs` runs after one warm-up, and its last result."""
    out = fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def _wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 2_000_000, 20_000_000])
    ap.add_argument("--cpu_sizes", type=int, nargs="*", default=[200_000, 2_000_000], help="sizes at which the host path is timed too")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--protocol_runs", type=int, default=None, help="runs of the whole protocol (default: --runs)")
    args = ap.parse_args(argv)
    crop = _crop()
    F.evaluate_points(*_clouds(20000, 0.3), 0.3, crop=crop, device="gpu")      # warm-up: kernel loading and the allocator
    for n in args.sizes:
        tau = 2 * SIDE / np.sqrt(n)
        pred, gt = _clouds(n, tau)
        P, G = F._dev(pred), F._dev(gt)
        gpu, cpu = {}, {}
        gpu["crop"], keep = _events(lambda: ops.fscore_crop(G, 2, crop.axis_min, crop.axis_max, F._dev(crop.polygon)[:, :2].contiguous()),
                                    args.runs)
        Gc, Pc = G[keep].contiguous(), P[F.crop_points(P, crop, device="gpu")].contiguous()
        gpu["voxel_mean"], Gv = _events(lambda: ops.fscore_voxel_mean(Gc, tau / 2), args.runs)
        Pv = ops.fscore_voxel_mean(Pc, tau / 2)
        table = ops.NearestTable(Gv)
        cell_scan = (table.cstart[1:] - table.cstart[:-1]).double()
        occupied = cell_scan[cell_scan > 0]
        rec = {"points": n, "tau": tau, "gt_cropped": int(Gc.shape[0]), "gt_voxel": int(Gv.shape[0]), "pred_voxel": int(Pv.shape[0]),
               "table": {"cell": table.cell, "cell_over_tau": table.cell / tau, "dims": table.dims,
                         "cells_per_point": table.cells_per_point, "occupied_share": float(len(occupied) / len(cell_scan)),
                         "points_per_occupied_cell": float(occupied.mean()), "max_points_per_cell": int(occupied.max())}}
        del cell_scan, occupied, table
        gpu["nearest"], (d1, _) = _events(lambda: ops.nearest_capped_index(Pv, Gv, 5 * tau), args.runs)
        src, tgt = ops.fscore_voxel_mean(Pc, tau), ops.fscore_voxel_mean(Gc, tau)
        gpu["icp_round"], icp_gpu = _events(lambda: F.icp(src, tgt, np.eye(4), 80 * tau, 20, device="gpu"), args.runs)
        rec["icp_round"] = {"source": int(src.shape[0]), "target": int(tgt.shape[0]), "iterations": icp_gpu[3], "fitness": icp_gpu[1]}
        del src, tgt
        torch.cuda.empty_cache()
        gpu["protocol"], res = _events(lambda: F.evaluate_points(P, G, tau, crop=crop, device="gpu"),
                                       args.runs if args.protocol_runs is None else args.protocol_runs)
        rec["gpu_ms"] = {k: round(v, 2) for k, v in gpu.items()}
        rec["protocol"] = {k: res[k] for k in ("precision", "recall", "fscore")}
        rec["protocol"]["icp_iterations"] = [r["iterations"] for r in res["icp"]]
        if n in args.cpu_sizes:
            cpu["crop"], keep_c = _wall(lambda: F.crop_points(gt, crop))
            gc, pc = gt[keep_c], pred[F.crop_points(pred, crop)]
            cpu["voxel_mean"], gv = _wall(lambda: F.voxel_mean(gc, tau / 2))
            pv = F.voxel_mean(pc, tau / 2)
            cpu["nearest"], (d1_c, _) = _wall(lambda: F.nearest(pv, gv, 5 * tau))
            s, t = F.voxel_mean(pc, tau), F.voxel_mean(gc, tau)
            cpu["icp_round"], icp_cpu = _wall(lambda: F.icp(s, t, np.eye(4), 80 * tau, 20))
            cpu["protocol"], res_c = _wall(lambda: F.evaluate_points(pred, gt, tau, crop=crop))
            rec["cpu_ms"] = {k: round(v, 1) for k, v in cpu.items()}
            rec["speedup"] = {k: round(cpu[k] / gpu[k], 1) for k in gpu}
            rec["identical"] = {"crop": bool(np.array_equal(keep.cpu().numpy(), keep_c)),
                                "voxel_mean": bool(np.array_equal(Gv.cpu().numpy(), gv)),
                                "nearest": bool(np.array_equal(d1.cpu().numpy(), d1_c)),
                                "icp_iterations": icp_cpu[3] == icp_gpu[3],
                                "tallies": all(res[k] == res_c[k] for k in ("precision", "recall", "curve_precision", "curve_recall"))}
        print(json.dumps(rec), flush=True)
        del P, G, Gc, Pc, Gv, Pv, d1
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
