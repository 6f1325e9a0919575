#!/usr/bin/env python3
"""Times the depth-map consistency kernel (csrc/depth_filter.hip) on the GPU and writes profiles/depth_filter.txt:

    python scripts/time_depth_filter.py [--out profiles/depth_filter.txt] [--kernel_trace <kernel_trace.csv>]

  * ms per surf_depth_consistency launch for one reference map of 144 x 200, 576 x 800 and 1080 x 1920 against 1, 4 and 16 sources
    of the same size, for each thread-to-pixel mapping (a wavefront covers 64 pixels of the flat index, a 16 x 4 tile or an 8 x 8
    tile), the time per (pixel, source) pair and the bytes of the reference-side streams the launch moves per second (depth read
    at every pixel, count + zsum read at the measured pixels and written where a source agreed, once per launch whatever the
    number of sources: they are looped inside the kernel; the four taps per pair in the source maps come through the caches);
  * ms of surf_depth_consistency_finish, and of the host mirror (fusion.consistency_host) on the smallest case, for scale.
ms/launch is what a caller of ops.depth_consistency waits for: where the kernel is short that is the host's work per launch (the
source table, the ctypes call), not the kernel.  --kernel_trace takes the kernel trace of an earlier run of this very command
under `rocprofv3 --kernel-trace --output-format csv` and reports the kernel's own time per launch; the per-pair time and the
rate are then taken from it.
Scene: a sphere of radius 0.5 seen by 17 ring cameras (scripts/time_fuse.py's), analytic depth maps; the sources are the
reference's nearest neighbours on the ring.  Device events around 10 launches after 3 warm-up launches; count and zsum are reset
before every series."""
import argparse
import csv
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = ((144, 200), (576, 800), (1080, 1920))
MAPPINGS = ((64, "64 x 1 (flat)"), (16, "16 x 4"), (8, "8 x 8"))
SOURCES = (1, 4, 16)
WARMUP = 3


def kernel_ms(path, iters):
    """Per series (in the order this script runs them) the mean kernel time in ms of its timed launches, from the rows of a
    rocprofv3 kernel trace whose kernel is depth_consistency_kernel: a series is 1 + WARMUP + iters launches, the last iters count."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if "depth_consistency_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per, n_series = 1 + WARMUP + iters, len(SIZES) * len(MAPPINGS) * len(SOURCES)
    if len(rows) != per * n_series:
        raise SystemExit(f"{path}: {len(rows)} launches of depth_consistency_kernel, this command makes {per * n_series}")
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows]
    return [sum(ns[i * per + per - iters:(i + 1) * per]) / iters / 1e6 for i in range(n_series)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "depth_filter.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel_trace", default=None, help="kernel_trace.csv of a rocprofv3 run of this command with the same --iters")
    args = ap.parse_args(argv)
    from surf_amd import fusion, ops
    from surf_amd.fusion import DepthView
    from time_fuse import sphere_views
    assert torch.cuda.is_available(), "time_depth_filter.py measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    traced = None if args.kernel_trace is None else kernel_ms(args.kernel_trace, args.iters)
    lines = [f"# scripts/time_depth_filter.py: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}, "
             f"{torch.cuda.get_device_properties(0).multi_processor_count} CUs), one reference map against 1, 4, 16 sources of its size "
             "per launch",
             f"# ms/launch: device events around {args.iters} launches of ops.depth_consistency after {WARMUP} warm-up launches (host "
             "work per launch included: it is the larger part where the kernel is short)",
             "# kernel ms: the kernel alone, mean of the same launches in a rocprofv3 --kernel-trace run of this command"
             if traced else "# kernel ms: not measured (no --kernel_trace); per-pair time and rate are taken from ms/launch",
             "# ref-side bytes of a launch = depth read at every pixel + (count + zsum) read at the measured pixels + written at the "
             "pixels a source agreed with; ns/(pixel source) and GB/s from the kernel time",
             "# surf_depth_consistency",
             "wavefront      map          sources  ms/launch  kernel ms  ns/(pixel source)  measured  agreed  ref-side MB  ref-side GB/s"]

    def timed(fn, iters):
        for _ in range(WARMUP):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    host_line, finish_lines, series = None, [], 0
    for H, W in SIZES:
        views = [DepthView(P, depth, dscale) for P, depth, dscale, _ in sphere_views(17, H, W, dev)]
        order = fusion.nearest_sources(views, 16)[0]
        ref = (views[0].depth, 1.0)
        count = torch.zeros(H, W, dtype=torch.int32, device=dev)
        zsum = torch.zeros(H, W, device=dev)
        measured = float((views[0].depth > 0).sum()) / (H * W)
        for tile_w, name in MAPPINGS:
            for ns in SOURCES:
                sources = [(fusion.pair_transforms(views[0], views[s]), views[s].depth, 1.0) for s in order[:ns]]
                count.zero_(), zsum.zero_()
                ops.depth_consistency(ref, sources, count, zsum, tile_w=tile_w)
                agreed = float((count > 0).sum()) / (H * W)          # every launch of the series writes exactly these pixels
                ms = timed(lambda: ops.depth_consistency(ref, sources, count, zsum, tile_w=tile_w), args.iters)
                kms = traced[series] if traced else ms
                series += 1
                mb = H * W * (4 + 8 * measured + 8 * agreed) / 1e6
                lines.append(f"{name:13s}  {H:4d} x {W:4d}  {ns:7d}  {ms:9.4f}  {f'{kms:9.4f}' if traced else '        -'}  "
                             f"{1e6 * kms / (H * W * ns):17.4f}  {measured:8.3f}  {agreed:6.3f}  {mb:11.3f}  {mb / kms:13.2f}")
        ms = timed(lambda: ops.depth_consistency_finish(ref, count, zsum, 2), args.iters)
        finish_lines.append(f"finish         {H:4d} x {W:4d}  {ms:9.4f} ms per call   (13 B read, 5 B written per pixel; the two output "
                            "allocations included)")
        if host_line is None:
            host = [v._replace(depth=v.depth.cpu().numpy()) for v in views]
            t0 = time.perf_counter()
            fusion.consistency_host(host, 0, order[:1])
            host_line = (f"host mirror    {H:4d} x {W:4d}  1 source: {1e3 * (time.perf_counter() - t0):9.3f} ms   "
                         "(fusion.consistency_host, numpy fp32)")
    lines += ["# surf_depth_consistency_finish (min_consistent 2)"] + finish_lines + ["# for scale", host_line]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
