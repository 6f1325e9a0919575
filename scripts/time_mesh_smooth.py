#!/usr/bin/env python3
"""Times mesh smoothing (surf_amd/mesh_smooth.py; csrc/mesh_smooth.hip) on the GPU and writes profiles/mesh_smooth.txt:

    python scripts/time_mesh_smooth.py [--sides 1000 3162] [--fused_res 1024] [--out profiles/mesh_smooth.txt]
                                       [--kernel_trace <kernel_trace.csv>] [--no_host]

Meshes: noisy height fields of side x side vertices in row-major order (1000 -> 1.0 M vertices, 3162 -> 10.0 M; interior degree 6,
neighbours one row apart, as marching cubes' lattice order leaves them), and with --fused_res R the marching-cubes mesh of
scripts/time_simplify.py's fused sphere at R^3.
Per mesh:
  * ops.smooth_mesh with the defaults (10 Taubin pairs = 20 steps) and normals, stage by stage: device events around each stage
    over --iters repetitions after 2 warm-up ones, mesh resident on the device; total = wall clock of a repetition with its two
    host reads;
  * the step alone: device events around --step_reps launches of surf_smooth_step on the built adjacency after 5 warm-up ones,
    its compulsory bytes (per vertex 16 in + 16 out + 4 row_start + 1 boundary, plus 4 per neighbour entry) and the time those
    bytes take at the 6.29 TB/s this GPU copies at (MI355X measured copy rate); `bound/measured` is that ratio, reported, not
    a pass mark.  With --kernel_trace (the kernel_trace.csv of a `rocprofv3 --kernel-trace --output-format csv` run of this
    command with the same arguments) the step kernel's own time replaces the event time in that ratio;
  * the numpy mirror (smooth_mesh_host, one Taubin pair and normals, one repetition), per stage and per step.
Measurements, not thresholds."""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_TBS = 6.29
STAGES = ("adjacency", "steps", "cap", "normals")
STEP_WARMUP = 5


def height_field(side, seed=0):
    """(vertices (side^2, 3) fp32, faces (2 (side - 1)^2, 3) int32): a unit-spaced grid with noise of 0.2 in z, row-major."""
    g = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(side, dtype=np.float32), np.arange(side, dtype=np.float32), indexing="ij")
    v = np.stack([i.reshape(-1), j.reshape(-1), g.normal(0.0, 0.2, side * side).astype(np.float32)], axis=1)
    a = (np.arange(side - 1, dtype=np.int64)[:, None] * side + np.arange(side - 1, dtype=np.int64)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([a, a + side, a + side + 1], axis=1), np.stack([a, a + side + 1, a + 1], axis=1)])
    return v, f.astype(np.int32)


def step_kernel_ms(path, launches):
    """Per mesh, the mean time in ms of its last `reps` step_kernel launches in a rocprofv3 kernel trace; launches = [(all, reps)]."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "step_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != sum(a for a, _ in launches):
        raise SystemExit(f"{path}: {len(rows)} launches of step_kernel, this command makes {sum(a for a, _ in launches)}")
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    out, at = [], 0
    for count, reps in launches:
        out.append(sum(ns[at + count - reps:at + count]) / reps / 1e6)
        at += count
    return out


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", type=int, nargs="*", default=[1000, 3162])
    ap.add_argument("--fused_res", type=int, nargs="*", default=[1024])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--step_reps", type=int, default=20)
    ap.add_argument("--no_host", action="store_true", help="skip the numpy mirror (a traced run)")
    ap.add_argument("--kernel_trace", default=None)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mesh_smooth.txt"))
    args = ap.parse_args(argv)
    from surf_amd import _lib, ops
    from surf_amd.mesh_smooth import DEFAULTS, schedule, smooth_mesh_host
    assert torch.cuda.is_available(), "time_mesh_smooth.py measures on the GPU"
    dev = torch.device("cuda:0")
    meshes = [(f"height field {s} x {s}", lambda s=s: height_field(s)) for s in args.sides]
    if args.fused_res:
        from time_simplify import fused_mesh
        for res in args.fused_res:
            meshes.append((f"fused sphere {res}^3", lambda res=res: fused_mesh(res, dev)[:2]))
    n_steps = len(schedule(DEFAULTS["iterations"], DEFAULTS["lam"], DEFAULTS["mu"]))
    per_mesh = ((2 + args.iters) * n_steps + STEP_WARMUP + args.step_reps, args.step_reps)
    traced = None if args.kernel_trace is None else step_kernel_ms(args.kernel_trace, [per_mesh] * len(meshes))
    lines = [f"# scripts/time_mesh_smooth.py: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"# device ms: events per stage ({' | '.join(STAGES)}) of ops.smooth_mesh(defaults: {n_steps} steps, normals=True) over "
             f"{args.iters} repetitions after 2 warm-up ones; total = wall clock with the two host reads, mesh resident on the device",
             f"# step: ms per surf_smooth_step launch, device events around {args.step_reps} launches after {STEP_WARMUP} warm-up ones; "
             + ("kernel ms: the step kernel alone, mean of the same launches in a rocprofv3 --kernel-trace run of this command"
                if traced else "kernel ms: not measured (no --kernel_trace)"),
             f"# bytes = n (16 + 16 + 4 + 1) + 4 nnz per step; bound = bytes at {COPY_TBS} TB/s (the measured copy rate); "
             "bound/measured against the kernel ms when traced, else against the event ms.  Reported, not a pass mark.",
             "# host ms: smooth_mesh_host, ONE Taubin pair (2 steps) and normals, one repetition (numpy, one thread)"]
    for k, (name, make) in enumerate(meshes):
        v, f = make()
        v32, f32 = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
        n, m = len(v32), len(f32)
        dv, df = torch.from_numpy(v32).to(dev), torch.from_numpy(f32).to(dev)
        sums, totals = dict.fromkeys(STAGES, 0.0), []
        for it in range(2 + args.iters):
            st = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ops.smooth_mesh(dv, df, normals=True, stages=st)
            torch.cuda.synchronize()
            if it >= 2:
                totals.append(1e3 * (time.perf_counter() - t0))
                for sname, a, b in st:
                    sums[sname] += a.elapsed_time(b) / args.iters
        info = out[2]
        del out
        # the step alone
        row_start, nbr, boundary, _ = ops.smooth_adjacency(df, n)
        nnz = int(nbr.shape[0])
        a = torch.zeros(n, 4, dtype=torch.float32, device=dev)
        a[:, :3] = dv
        b = torch.empty_like(a)
        L, s = _lib.lib(), ops._stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(STEP_WARMUP + args.step_reps):
            if r == STEP_WARMUP:
                torch.cuda.synchronize()
                e0.record()
            L.surf_smooth_step(ops._p(a), ops._p(b), n, ops._p(row_start), ops._p(nbr), nnz, ops._p(boundary), 1,
                               0.5 if r % 2 == 0 else -0.53, s)
            a, b = b, a
        e1.record()
        torch.cuda.synchronize()
        step_ms = e0.elapsed_time(e1) / args.step_reps
        nbytes = n * (16 + 16 + 4 + 1) + 4 * nnz
        bound_ms = nbytes / (COPY_TBS * 1e12) * 1e3
        kms = traced[k] if traced else None
        lines += [f"{name}: {n} vertices, {m} faces, {nnz} neighbour entries (mean degree {nnz / max(n, 1):.2f}), "
                  f"{info['boundary_vertices']} boundary, moved_rms {info['moved_rms']:.4g}",
                  f"  device  {' | '.join(f'{sums[x]:8.3f}' for x in STAGES)}   total {np.mean(totals):9.3f}   "
                  f"per step in the run {sums['steps'] / n_steps:7.4f}",
                  f"  step    {step_ms:8.4f} ms/launch   kernel ms {f'{kms:8.4f}' if kms is not None else 'not measured'}   "
                  f"bytes {nbytes / 1e6:9.1f} MB   bound {bound_ms:7.4f} ms   bound/measured {bound_ms / (kms or step_ms):5.2f}   "
                  f"({nbytes / 1e9 / (kms or step_ms):5.2f} TB/s of compulsory bytes)"]
        del a, b, row_start, nbr, boundary, dv, df
        if not args.no_host:
            st = []
            t0 = time.perf_counter()
            smooth_mesh_host(v32, f32, iterations=1, normals=True, stages=st)
            h_total = 1e3 * (time.perf_counter() - t0)
            h = dict(st)
            lines.append(f"  host    {' | '.join(f'{h.get(x, 0.0):8.1f}' for x in STAGES)}   total {h_total:9.1f}   "
                         f"per step {h['steps'] / 2:9.1f}")
        for line in lines[-(3 if args.no_host else 4):]:
            print(line, flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
