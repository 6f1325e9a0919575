#!/usr/bin/env python3
"""Times mesh denoising (surf_amd/mesh_denoise.py; csrc/mesh_denoise.hip) on the GPU and writes profiles/mesh_denoise.txt:

    python scripts/time_mesh_denoise.py [--sides 1000 3162] [--host_side 1000] [--out profiles/mesh_denoise.txt]

Meshes: the noisy height fields of scripts/time_mesh_smooth.py, side x side vertices in row-major order (1000 -> 1.0 M vertices,
3162 -> 10.0 M; interior vertices have 6 faces, interior faces 13 face neighbours).
Per mesh:
  * ops.denoise_mesh with the defaults (10 normal and 10 vertex iterations) and normals, stage by stage: device events around each
    stage over --iters repetitions after 1 warm-up one, mesh resident on the device; total = wall clock of a repetition with its
    three host reads;
  * each step alone: device events around --step_reps launches of surf_denoise_normal_step and of surf_denoise_vertex_step on the
    built lists after 3 warm-up ones, the step's compulsory bytes and the time those bytes take at the 6.29 TB/s this GPU copies
    at (MI355X measured copy rate); `bound/measured` is that ratio, reported, not a pass mark.  Compulsory bytes: a normal step
    reads per face its 32-byte record and 4 bytes of row_start, 4 bytes per neighbour entry, and writes 16 bytes; a vertex step
    reads per vertex its 16-byte row, 8 bytes of corner_start and the boundary byte, 8 bytes per corner, every face's indices
    and normal once (12 + 16 bytes), and writes 16 bytes.  The gathered rows are re-reads of rows counted once;
  * for the mesh of --host_side, the numpy mirror (denoise_mesh_host, ONE normal and ONE vertex iteration and normals, one
    repetition), per stage.
Measurements, not thresholds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_TBS = 6.29
STAGES = ("adjacency", "records", "neighbours", "normal_steps", "vertex_steps", "cap", "normals")
HOST_STAGES = ("records", "neighbours", "normal_steps", "vertex_steps", "cap", "normals")
STEP_WARMUP = 3


def timed_launches(launch, reps):
    """ms per call of launch(r), device events around `reps` calls after STEP_WARMUP warm-up ones."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(STEP_WARMUP + reps):
        if r == STEP_WARMUP:
            torch.cuda.synchronize()
            e0.record()
        launch(r)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sides", type=int, nargs="*", default=[1000, 3162])
    ap.add_argument("--host_side", type=int, default=1000, help="the side whose mesh the numpy mirror is timed on (0: none)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--step_reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mesh_denoise.txt"))
    args = ap.parse_args(argv)
    from surf_amd import _lib, ops
    from surf_amd.mesh_denoise import DEFAULTS, denoise_mesh_host, inverse_supports
    from time_mesh_smooth import height_field
    assert torch.cuda.is_available(), "time_mesh_denoise.py measures on the GPU"
    dev = torch.device("cuda:0")
    n_normal, n_vertex = DEFAULTS["normal_iterations"], DEFAULTS["vertex_iterations"]
    lines = [f"# scripts/time_mesh_denoise.py: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"# device ms: events per stage ({' | '.join(STAGES)}) of ops.denoise_mesh(defaults: {n_normal} normal and {n_vertex} "
             f"vertex iterations, normals=True) over {args.iters} repetitions after 1 warm-up one; total = wall clock with the "
             "three host reads, mesh resident on the device",
             f"# steps: ms per launch, device events around {args.step_reps} launches after {STEP_WARMUP} warm-up ones; bytes = the "
             f"step's compulsory bytes (see the script), bound = bytes at {COPY_TBS} TB/s (the measured copy rate).  Reported, not a "
             "pass mark.",
             "# host ms: denoise_mesh_host, ONE normal and ONE vertex iteration and normals, one repetition (numpy, one thread)"]
    for side in args.sides:
        v32, f32 = height_field(side)
        n, m = len(v32), len(f32)
        dv, df = torch.from_numpy(v32).to(dev), torch.from_numpy(f32).to(dev)
        sums, totals = dict.fromkeys(STAGES, 0.0), []
        for it in range(1 + args.iters):
            st, keep = [], {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ops.denoise_mesh(dv, df, normals=True, stages=st, keep=keep)
            torch.cuda.synchronize()
            if it >= 1:
                totals.append(1e3 * (time.perf_counter() - t0))
                for sname, a, b in st:
                    sums[sname] += a.elapsed_time(b) / args.iters
        info = out[2]
        del out
        # the steps alone, on the lists and records of the last run
        rows, nbr, records = keep["face_row_start"], keep["face_neighbours"], keep["records"]
        total = int(nbr.shape[0])
        L, s = _lib.lib(), ops._stream()
        inv_s, inv_r = inverse_supports(info["sigma_s"], info["sigma_r"])
        bufs = [records.clone(), records.clone()]
        normal_ms = timed_launches(lambda r: L.surf_denoise_normal_step(ops._p(bufs[r % 2]), ops._p(bufs[1 - r % 2]), m, ops._p(rows),
                                                                        ops._p(nbr), total, inv_s, inv_r, s), args.step_reps)
        corder, cstart = ops.denoise_corners(df, n)
        boundary = ops.smooth_adjacency(df, n)[2]
        pos = [torch.zeros(n, 4, dtype=torch.float32, device=dev) for _ in range(2)]
        pos[0][:, :3] = dv
        vertex_ms = timed_launches(lambda r: L.surf_denoise_vertex_step(ops._p(pos[r % 2]), ops._p(pos[1 - r % 2]), n, ops._p(df), m,
                                                                        ops._p(records), ops._p(corder), ops._p(cstart),
                                                                        ops._p(boundary), 1, s), args.step_reps)
        normal_bytes = m * (32 + 4 + 16) + 4 * total
        vertex_bytes = n * (16 + 8 + 1 + 16) + 8 * 3 * m + m * (12 + 16)
        lines += [f"height field {side} x {side}: {n} vertices, {m} faces, {total} face neighbour entries (mean row "
                  f"{total / max(m, 1):.2f}), {info['boundary_vertices']} boundary, sigma_s {info['sigma_s']:.4g}, moved_rms "
                  f"{info['moved_rms']:.4g}",
                  f"  device  {' | '.join(f'{sums[x]:8.3f}' for x in STAGES)}   total {np.mean(totals):9.3f}   per normal step in "
                  f"the run {sums['normal_steps'] / n_normal:7.4f}   per vertex step {sums['vertex_steps'] / n_vertex:7.4f}"]
        for what, ms, nbytes in (("normal step", normal_ms, normal_bytes), ("vertex step", vertex_ms, vertex_bytes)):
            bound = nbytes / (COPY_TBS * 1e12) * 1e3
            lines.append(f"  {what} {ms:8.4f} ms/launch   bytes {nbytes / 1e6:9.1f} MB   bound {bound:7.4f} ms   bound/measured "
                         f"{bound / ms:5.2f}   ({nbytes / 1e9 / ms:5.2f} TB/s of compulsory bytes)")
        del rows, nbr, records, bufs, pos, corder, cstart, boundary, keep, dv, df
        shown = 4
        if side == args.host_side:
            st = []
            t0 = time.perf_counter()
            denoise_mesh_host(v32, f32, normal_iterations=1, vertex_iterations=1, normals=True, stages=st)
            h_total = 1e3 * (time.perf_counter() - t0)
            h = dict(st)
            lines.append(f"  host    ({' | '.join(HOST_STAGES)}) {' | '.join(f'{h.get(x, 0.0):8.1f}' for x in HOST_STAGES)}   total "
                         f"{h_total:9.1f}")
            shown = 5
        for line in lines[-shown:]:
            print(line, flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
