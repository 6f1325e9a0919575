#!/usr/bin/env python3
"""Times the point-cloud clean-up (surf_amd/point_filter.py; csrc/point_knn.hip) on the GPU and writes profiles/point_filter.txt:

    python scripts/time_point_filter.py [--sizes 1000000 10000000] [--k 16] [--out profiles/point_filter.txt]

  * synthetic surface-like clouds (a sphere of radius 0.5 with radial noise of a third of the point spacing, plus 1 % uniform
    outliers in [-1, 1]^3; max_dist = 10 spacings), k = 16.  HIP events around: the table build (key kernel, torch sort, bincount,
    cumsum, the permutation), the fused search with the statistic, the fused search with statistic and normals, and the
    list-writing search (up to --lists_up_to points).  Mean of --iters repetitions after 2 warm-up ones, points resident on the device;
  * the host path's k-d tree on the same cloud: scipy's cKDTree build and its query of the k + 1 nearest with workers = --workers
    (the 16 CPUs a job may use), one repetition, and point_filter.knn_host as a whole up to --lists_up_to points;
  * one real cloud: fusion.fuse_points over 49 ring views of 576 x 800 against their 4 nearest views (scripts/time_points.py's
    scene), wall clock, then remove_outliers + estimate_normals on that cloud (wall clock, host copies included): the clean-up's
    share of the merge that made the cloud;
  * the compiler's resource remarks for the two search kernels are appended from --remarks FILE when given (a build with
    -Rpass-analysis=kernel-resource-usage), else the file says where to get them.
Measurements, not thresholds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def surface_cloud(n, seed=0):
    """(points (n, 3) fp32, spacing): 99 % on a noisy sphere of radius 0.5, 1 % uniform in [-1, 1]^3, shuffled."""
    g = np.random.default_rng(seed)
    n_out = n // 100
    n_surf = n - n_out
    spacing = float(np.sqrt(4 * np.pi * 0.25 / n_surf))
    d = g.normal(size=(n_surf, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    surf = d * (0.5 + g.normal(0.0, spacing / 3, (n_surf, 1)))
    pts = np.concatenate([surf, g.uniform(-1, 1, (n_out, 3))]).astype(np.float32)
    return pts[g.permutation(n)], spacing


def event_ms(fn, iters, warmup=2):
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
    return total / iters, out


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--lists_up_to", type=int, default=1000000)
    ap.add_argument("--no_fuse", action="store_true", help="skip the fuse_points comparison")
    ap.add_argument("--remarks", default=None, help="compiler output of a build with -Rpass-analysis=kernel-resource-usage")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "point_filter.txt"))
    args = ap.parse_args(argv)
    from scipy.spatial import cKDTree
    from surf_amd import fusion, ops, point_filter as PF
    assert torch.cuda.is_available(), "time_point_filter.py measures on the GPU"
    dev = torch.device("cuda:0")
    props = torch.cuda.get_device_properties(0)
    k = args.k
    lines = [f"# scripts/time_point_filter.py --sizes {' '.join(map(str, args.sizes))} --k {k}: {torch.cuda.get_device_name(0)} "
             f"({props.gcnArchName}, {props.multi_processor_count} CUs)",
             f"# device: HIP events, mean of {args.iters} repetitions after 2 warm-up ones, ms; Mpts/s of the fused search with the statistic. "
             f"host: scipy cKDTree, float64, build + query of the k + 1 nearest with workers = {args.workers}, one repetition, ms; "
             "knn_host = the whole numpy mirror (tree, ball query, fp32 recomputation, ordering).",
             "points      max_dist   cells/pt  pts/cell(occ)  table ms  search+stat ms  +normals ms  lists ms   Mpts/s  starved  | "
             "tree build ms  tree query ms  knn_host ms  | tree query / search+stat"]
    for n in args.sizes:
        P, spacing = surface_cloud(n)
        md = 10 * spacing
        pts = torch.from_numpy(P).to(dev)
        ms_table, table = event_ms(lambda: ops.PointKnnTable(pts, md), args.iters)
        occ = int((table.cstart[1:] > table.cstart[:-1]).sum())
        cells_per_point = table.cells_per_point
        ms_stat, (stat, count, _) = event_ms(lambda: ops.points_knn_reduce(table, k, md), args.iters)
        ms_nrm, _ = event_ms(lambda: ops.points_knn_reduce(table, k, md, normals=True), args.iters)
        ms_lists = event_ms(lambda: ops.points_knn(table, k, md), args.iters)[0] if n <= args.lists_up_to else float("nan")
        starved = int((count < k).sum())
        del table
        t0 = time.perf_counter()
        tree = cKDTree(P.astype(np.float64))
        t1 = time.perf_counter()
        tree.query(P.astype(np.float64), k=k + 1, distance_upper_bound=md, workers=args.workers)
        t2 = time.perf_counter()
        del tree
        ms_host = float("nan")
        if n <= args.lists_up_to:
            t3 = time.perf_counter()
            hi, hd, hc = PF.knn_host(P, k, md, workers=args.workers)
            ms_host = 1e3 * (time.perf_counter() - t3)
            assert np.array_equal(PF.stat_host(hd, hc), stat.cpu().numpy()) and np.array_equal(hc, count.cpu().numpy())
        lines.append(f"{n:9d}  {md:9.5f}  {cells_per_point:8.2f}  {n / max(occ, 1):13.1f}  {ms_table:8.2f}  {ms_stat:14.2f}  "
                     f"{ms_nrm:11.2f}  {ms_lists:8.2f}  {n / ms_stat / 1e3:7.1f}  {starved:7d}  | {1e3 * (t1 - t0):13.0f}  "
                     f"{1e3 * (t2 - t1):13.0f}  {ms_host:11.0f}  | {1e3 * (t2 - t1) / ms_stat:8.1f} x")
        print(lines[-1], flush=True)
        del pts, stat, count
    if not args.no_fuse:
        from surf_amd.fusion import DepthView
        from time_fuse import sphere_views
        views = [DepthView(*v) for v in sphere_views(49, 576, 800, dev)]
        near = fusion.nearest_sources(views, 4)
        fusion.fuse_points(views, 2, sources=near, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cloud = fusion.fuse_points(views, 2, sources=near, device=dev)
        torch.cuda.synchronize()
        ms_fuse = 1e3 * (time.perf_counter() - t0)
        ext = cloud.points.max(0) - cloud.points.min(0)
        md = 10 * float(np.sqrt(np.pi * 0.25 * 2 / len(cloud.points)))        # ten spacings of the visible part of the sphere
        centres = PF.camera_centres(views)
        st = {}
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept_cloud, _ = PF.remove_outliers(cloud, k=k, max_dist=md, device=dev, stats=st)
            t1 = time.perf_counter()
            nrm = PF.estimate_normals(kept_cloud, centres, k=k, max_dist=md, device=dev)
            t2 = time.perf_counter()
        lines += ["#", f"# one real cloud: fuse_points over 49 ring views of 576 x 800, 4 nearest sources, min_consistent 2 (wall clock, second call): "
                  f"{len(cloud.points)} points (extent {ext.max():.2f}) in {ms_fuse:.1f} ms",
                  f"# remove_outliers(k={k}, max_dist={md:.5f}) {1e3 * (t1 - t0):.1f} ms -> {st['points_out']} points ({st['starved']} starved), "
                  f"estimate_normals {1e3 * (t2 - t1):.1f} ms ({int((~nrm.any(1)).sum())} zero); wall clock with the host copies of the "
                  f"arrays; together {100 * 1e3 * (t2 - t0) / ms_fuse:.0f} % of the merge's time"]
        print("\n".join(lines[-2:]), flush=True)
    lines += ["#", "# compiler resource remarks (-Rpass-analysis=kernel-resource-usage, gfx950) of the two search kernels:"]
    if args.remarks and os.path.exists(args.remarks):
        keep, on = [], False
        for l in open(args.remarks):
            if "Function Name" in l:
                on = "knn_lists_kernel" in l or "knn_reduce_kernel" in l
                if on:
                    keep.append("# " + ("knn_lists_kernel" if "knn_lists_kernel" in l else "knn_reduce_kernel") + " (64 threads; dynamic LDS k * 512 B)")
            elif on and "remark:" in l and any(w in l for w in ("VGPRs:", "AGPRs:", "TotalSGPRs:", "ScratchSize", "Occupancy", "LDS Size", "Spill")):
                keep.append("#   " + l.split("remark:")[-1].split("[-Rpass")[0].strip().split(":0: ")[-1].strip())
        lines += keep
    else:
        lines.append("#   (not collected in this run: SURF_EXTRA_FLAGS=-Rpass-analysis=kernel-resource-usage bash surf_amd/csrc/build.sh)")
    lines += ["# scratch 0: the k-slot list is not a per-thread array (a run-time index would put it in scratch) but a column of LDS, one 8-byte "
              "word per slot (d2's bits above the index).  The compiler's LDS figure is the static part, 0: the launch adds k * 512 B per "
              f"64-thread workgroup ({k * 512} B at k = {k}, 16384 B at k = 32), so the 160 KB of a CU hold {min(32, 163840 // (k * 512))} such "
              f"wavefronts at k = {k} and 10 at k = 32 - LDS, not the 54 VGPRs (32 wavefronts), bounds the occupancy from k = 11 on."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
