#!/usr/bin/env python3
"""Times the point-set surface (surf_amd/point_surface.py; csrc/point_surface.hip) on the GPU and writes profiles/point_surface.txt:

    python scripts/time_point_surface.py [--sizes 1000000 10000000] [--out profiles/point_surface.txt] [--remarks FILE]

  * scripts/time_point_filter.py's cloud (a sphere of radius 0.5 with radial noise of a third of the point spacing, 1 % uniform
    outliers in [-1, 1]^3) with radial normals; voxel = the point spacing, R = 3 voxels, min_points = 4, no colours unless
    --colors; the lattice is the box of the cloud padded by R.  HIP events around: keys + sort (the key kernel, torch's sort, the
    gathers), mark + assign (rule 6, surf_compact, surf_band_assign), the field kernel, and extract_mesh (marching cubes over the
    bricks and the copy of the mesh to the host).  Mean of --iters repetitions after 2 warm-up ones, the cloud resident on the device;
  * counted by this script: pair evaluations = 512 x the candidates every brick staged, admitted pairs = the sum of the node counts
    of a run with min_points = 1 (there weight == count at every node), the minimal allocation of rule 6 = the bricks of that run
    that hold a node with count >= 1;
  * the field kernel against ITS OWN ISSUE BOUND: pair evaluations x vector instructions per pair, counted in the inner loop of the
    build's assembly (--instr_per_pair; the default is this tree's count), over CUs x 4 SIMDs x 16 lanes x the clock.  That is
    the time the kernel's own instruction stream needs at one wave-instruction per SIMD every 4 cycles with nothing else in the
    way - not a share of the chip's 157 TFLOP/s, which counts packed fused multiply-adds;
  * the numpy mirror (field_bricks_host) at --host_points points, wall clock, and that its arrays equal the device's;
  * the compiler's resource remarks of the field kernel from --remarks FILE (a build with -Rpass-analysis=kernel-resource-usage).
Measurements, not thresholds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# vector instructions of cloud_field_kernel's inner loop per (node, candidate) pair: the loop body handles 2 candidates x 2 nodes
# in 78 VALU instructions (32 of them packed v_pk_*_f32) without colours and 83 (36 packed) with them
INSTR_PER_PAIR = {False: 78 / 4, True: 83 / 4}


def oriented_cloud(n, seed=0):
    from time_point_filter import surface_cloud
    P, spacing = surface_cloud(n, seed)
    N = P / np.maximum(np.linalg.norm(P, axis=1, keepdims=True), 1e-12)
    return P, N.astype(np.float32), spacing


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--colors", action="store_true")
    ap.add_argument("--radius_voxels", type=float, default=3.0)
    ap.add_argument("--host_points", type=int, default=20000)
    ap.add_argument("--instr_per_pair", type=float, default=None)
    ap.add_argument("--clock_mhz", type=float, default=2400.0, help="the clock the issue bound is taken at (MI355X: 2400 MHz at most)")
    ap.add_argument("--remarks", default=None, help="compiler output of a build with -Rpass-analysis=kernel-resource-usage")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "point_surface.txt"))
    args = ap.parse_args(argv)
    from surf_amd import ops, point_surface as PS
    from surf_amd.fusion import PointCloud
    from time_point_filter import event_ms
    assert torch.cuda.is_available(), "time_point_surface.py measures on the GPU"
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    clock = args.clock_mhz * 1e6                       # Hz
    ipp = args.instr_per_pair if args.instr_per_pair is not None else INSTR_PER_PAIR[args.colors]
    lanes = props.multi_processor_count * 4 * 16
    rv = args.radius_voxels
    lines = [f"# scripts/time_point_surface.py --sizes {' '.join(map(str, args.sizes))}{' --colors' if args.colors else ''}: "
             f"{torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs; bound taken at {clock / 1e6:.0f} MHz)",
             f"# noisy sphere + 1 % outliers, voxel = point spacing, R = {rv} voxels, min_points 4.  HIP events, mean of {args.iters} "
             "repetitions after 2 warm-up ones, ms.  issue bound = pairs x "
             f"{ipp:.2f} vector instructions per pair / ({props.multi_processor_count} CUs x 4 SIMDs x 16 lanes x clock).",
             "points      lattice           bricks  alloc %  / minimal  cand max  keys+sort  mark+assign    field  extract ms |  "
             "pairs        admitted     adm %  | bound ms  bound / field  Gpair/s | vertices  faces"]
    for n in args.sizes:
        P, N, spacing = oriented_cloud(n)
        col = np.random.default_rng(1).integers(0, 256, P.shape).astype(np.uint8) if args.colors else None
        voxel, R = spacing, rv * spacing
        lo, hi = PS.cloud_bounds(P, N, R)
        vol = PS.PointSetVolume((lo, hi, voxel), R, colors=args.colors, device=dev).set_cloud(PointCloud(P, col, None), N)
        pts, nrm, cols = vol._cloud
        lat_lo, lat_voxel = vol._lattice
        ms_sort, cloud = event_ms(lambda: ops.cloud_sort(pts, nrm, cols, vol.axes, lat_lo, lat_voxel, vol.reach), args.iters)

        def allocate():
            mark = torch.zeros(vol.nbp ** 3, dtype=torch.uint8, device=dev)
            ops.cloud_mark_bricks(mark, cloud[1], vol.axes, lat_lo, lat_voxel, vol.reach)
            return ops.fuse_assign_bricks(mark)

        ms_mark, (table, bricks) = event_ms(allocate, args.iters)
        field = lambda mp: ops.cloud_field_bricks(cloud, bricks, vol.axes, lat_lo, lat_voxel, vol.reach, float(vol.radius), mp, staged=True)
        ms_field, (tsdf, weight, color, staged) = event_ms(lambda: field(4), args.iters)
        pairs = 512 * int(staged.long().sum())
        cand_max = int(staged.max())
        count = field(1)[1]                                         # min_points = 1: weight is the node's count everywhere
        admitted = int(count.double().sum())
        minimal = int((count.reshape(-1, 512) > 0).any(dim=1).sum())
        del count
        vol._state, vol._staged, vol.stats = (bricks, table, tsdf, weight, color), staged, {"points": int(cloud[0].shape[0])}
        ms_mesh, mesh = event_ms(lambda: vol.extract_mesh(), args.iters)
        bound = 1e3 * pairs * ipp / (lanes * clock)
        shape = "x".join(map(str, vol.shape))
        lines.append(f"{n:9d}  {shape:16s}  {vol.n_bricks:6d}  {100 * vol.allocated_share():7.3f}  {vol.n_bricks / max(minimal, 1):9.3f}  "
                     f"{cand_max:8d}  {ms_sort:9.2f}  {ms_mark:11.2f}  {ms_field:7.2f}  {ms_mesh:10.2f} |  {pairs:11.4g}  {admitted:11.4g}  "
                     f"{100 * admitted / max(pairs, 1):6.2f}  | {bound:8.2f}  {bound / ms_field:13.3f}  {pairs / ms_field / 1e6:7.1f} | "
                     f"{len(mesh[0]):8d}  {len(mesh[1]):8d}")
        print(lines[-1], flush=True)
        del vol, cloud, table, bricks, tsdf, weight, color, staged, mesh
        torch.cuda.empty_cache()
    # the numpy mirror at a size it can finish, and that the device returns its arrays
    n = args.host_points
    P, N, spacing = oriented_cloud(n)
    lo, hi = PS.cloud_bounds(P, N, rv * spacing)
    dvol = PS.PointSetVolume((lo, hi, spacing), rv * spacing, device=dev).set_cloud(P, N).finalize()
    t0 = time.perf_counter()
    hvol = PS.PointSetVolume((lo, hi, spacing), rv * spacing, backend="host").set_cloud(P, N).finalize()
    ms_host = 1e3 * (time.perf_counter() - t0)
    same = all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dvol._state[:4], hvol._state[:4]))
    lines += ["#", f"# numpy mirror (field_bricks_host) at {n} points, lattice {'x'.join(map(str, hvol.shape))}, {hvol.n_bricks} bricks: "
              f"{ms_host:.0f} ms wall clock; its arrays equal the device's: {same}"]
    print(lines[-1], flush=True)
    lines += ["#", "# compiler resource remarks (-Rpass-analysis=kernel-resource-usage, gfx950) of the field kernel (256 threads):"]
    if args.remarks and os.path.exists(args.remarks):
        on = False
        for l in open(args.remarks):
            if "Function Name" in l:
                on = "cloud_field_kernel" in l
                if on:
                    lines.append("# cloud_field_kernel<" + ("colours" if "ILb1E" in l else "no colours") + ">")
            elif on and "remark:" in l and any(w in l for w in ("VGPRs:", "AGPRs:", "TotalSGPRs:", "ScratchSize", "Occupancy", "LDS Size", "Spill")):
                lines.append("#   " + l.split("remark:")[-1].split("[-Rpass")[0].strip().split(":0: ")[-1].strip())
    else:
        lines.append("#   (not collected in this run: SURF_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage bash surf_amd/csrc/build.sh)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
