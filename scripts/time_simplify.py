#!/usr/bin/env python3
"""Times mesh simplification (surf_amd/mesh_simplify.py; csrc/mesh_simplify.hip) on the GPU and writes profiles/simplify.txt:

    python scripts/time_simplify.py [--res 512 2048] [--steps 2 4 8] [--out profiles/simplify.txt]

The meshes are those of scripts/time_fuse.py --sparse: a sphere of radius 0.5 in [-1, 1]^3, 16 ring views of 576 x 800 with colours
fused into a brick-sparse lattice of res^3.  Per lattice and per cell of 2, 4 and 8 lattice steps: triangles and vertices in and
out, the host path and the device path stage by stage, and mesh_io.write_ply of the mesh before and after.
Device: events around each stage, 5 repetitions after 2 warm-up ones, the mesh resident on the device; total = wall clock of a
repetition with its two host reads.  Host: one repetition (numpy, one thread).  Measurements, not thresholds."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEVICE_STAGES = ("keys+sort", "faces", "corner sort", "cells", "compact")
HOST_STAGES = ("keys+sort", "faces", "cells")


def fused_mesh(res, dev):
    from surf_amd.fusion import FusionVolume
    from time_fuse import sphere_views
    axes = [np.linspace(-1, 1, res).astype(np.float32) for _ in range(3)]
    vol = FusionVolume(axes, trunc=4 * 2.0 / (res - 1), colors=True, backend="device", device=dev, sparse=True)
    vol.integrate(sphere_views(16, 576, 800, dev))
    return vol.extract_mesh()


def write_ms(v, t, c, tmp):
    from surf_amd import mesh_io
    path = os.path.join(tmp, "m.ply")
    t0 = time.perf_counter()
    mesh_io.write_ply(path, v, t, colors=c)
    ms = 1e3 * (time.perf_counter() - t0)
    size = os.path.getsize(path)
    os.remove(path)
    return ms, size


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--steps", type=int, nargs="+", default=[2, 4, 8], help="cell sizes in lattice steps")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "simplify.txt"))
    args = ap.parse_args(argv)
    from surf_amd import ops
    from surf_amd.mesh_simplify import simplify_mesh_host
    dev = torch.device("cuda:0")
    lines = [f"# scripts/time_simplify.py --res {' '.join(map(str, args.res))} --steps {' '.join(map(str, args.steps))}: "
             f"{torch.cuda.get_device_name(0)}; the meshes of time_fuse.py --sparse (16 views of 576 x 800, colours)",
             f"# ms.  device: events per stage over {args.iters} repetitions after 2 warm-up ones ({' | '.join(DEVICE_STAGES)}), total = wall "
             "clock with the two host reads, mesh resident on the device.  host: one repetition of the numpy path "
             f"({' | '.join(HOST_STAGES)}).  write_ply: the coloured mesh before -> after, with the file's size in MB.",
             "res   cell  path    tri in    tri out   vert in   vert out  stages" + " " * 44 + "total      write_ply ms        PLY MB"]
    with tempfile.TemporaryDirectory() as tmp:
        for res in args.res:
            v, t, c = fused_mesh(res, dev)
            v32, t32 = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
            w_in, mb_in = write_ms(v32, t32, c, tmp)
            dv, dt, dc = (torch.from_numpy(x).to(dev) for x in (v32, t32, c))
            for k in args.steps:
                cell = k * 2.0 / (res - 1)
                st = []
                t0 = time.perf_counter()
                hv, hf, _, hc, _ = simplify_mesh_host(v32, t32, cell, colors=c, stages=st)
                h_total = 1e3 * (time.perf_counter() - t0)
                h_st = dict(st)
                w_out, mb_out = write_ms(hv, hf, hc, tmp)
                sums, totals = dict.fromkeys(DEVICE_STAGES, 0.0), []
                for it in range(2 + args.iters):
                    st = []
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = ops.simplify_mesh(dv, dt, cell, colors=dc, stages=st)
                    torch.cuda.synchronize()
                    if it >= 2:
                        totals.append(1e3 * (time.perf_counter() - t0))
                        for name, a, b in st:
                            sums[name] += a.elapsed_time(b) / args.iters
                assert np.array_equal(out[0].cpu().numpy(), hv) and np.array_equal(out[1].cpu().numpy(), hf)
                head = f"{res:4d}  {k:4d}  "
                tail = f"{len(t32):8d}  {len(hf):8d}  {len(v32):8d}  {len(hv):8d}  "
                lines.append(head + "host    " + tail + f"{' | '.join(f'{h_st.get(s, 0.0):9.1f}' for s in HOST_STAGES):50s}  {h_total:9.1f}  "
                             f"{w_in:8.1f} -> {w_out:6.1f}  {mb_in / 1e6:7.1f} -> {mb_out / 1e6:5.1f}")
                lines.append(head + "device  " + tail + f"{' | '.join(f'{sums[s]:7.3f}' for s in DEVICE_STAGES):50s}  {np.mean(totals):9.3f}")
                print(lines[-2]), print(lines[-1])
            del dv, dt, dc
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
