#!/usr/bin/env python3
"""Times the point-cloud merge (fusion.fuse_points, csrc/point_cloud.hip) on the GPU and writes profiles/points.txt:

    python scripts/time_points.py [--out profiles/points.txt]

  * ms per reference view of fusion.fuse_points for 49 views of 144 x 200 and 576 x 800, each tested against its 4, 16 and 48
    nearest views (min_consistent 2, average on): candidates, the consistency launches (16 sources each), the accept map, the
    mark launches, the ordered list of kept pixels (one host read of its length per view) and the lift, plus the one copy of the
    cloud to the host at the end;
  * beside it ms per reference view of fusion.filter_views on the same views with the same sources - the consistency launches
    and the finish alone, the only comparable number the tree had before the merge existed.
Scene: a sphere of radius 0.5 seen by 49 ring cameras (scripts/time_fuse.py's), analytic depth maps, random images.  Wall clock
around one call after one warm-up call, the device synchronised on either side."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = ((144, 200), (576, 800))
SOURCES = (4, 16, 48)
N_VIEWS = 49
MIN_CONSISTENT = 2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "points.txt"))
    args = ap.parse_args(argv)
    from surf_amd import fusion
    from surf_amd.fusion import DepthView
    from time_fuse import sphere_views
    assert torch.cuda.is_available(), "time_points.py measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    props = torch.cuda.get_device_properties(0)
    lines = [f"# scripts/time_points.py: {torch.cuda.get_device_name(0)} ({props.gcnArchName}, {props.multi_processor_count} CUs), "
             f"{N_VIEWS} ring views of a sphere, each against its nearest views, min_consistent {MIN_CONSISTENT}",
             "# ms/view: wall clock of one call (after one warm-up call, device synchronised) / number of views; fuse_points includes "
             "its copy of the cloud to the host, filter_views leaves its depth maps on the device",
             "map          sources  fuse_points ms/view  filter_views ms/view  points  kept by filter_views  measured"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / N_VIEWS, out

    for H, W in SIZES:
        views = [DepthView(P, depth, dscale, image) for P, depth, dscale, image in sphere_views(N_VIEWS, H, W, dev)]
        for ns in SOURCES:
            near = fusion.nearest_sources(views, ns)
            stats = {}
            ms_points, cloud = timed(lambda: fusion.fuse_points(views, MIN_CONSISTENT, sources=near, device=dev))
            ms_filter, _ = timed(lambda: fusion.filter_views(views, MIN_CONSISTENT, sources=near, average=True, device=dev))
            fusion.filter_views(views, MIN_CONSISTENT, sources=near, average=True, device=dev, stats=stats)
            lines.append(f"{H:4d} x {W:4d}  {ns:7d}  {ms_points:19.3f}  {ms_filter:20.3f}  {len(cloud.points):6d}  "
                         f"{sum(stats['kept']):20d}  {sum(stats['measured']):8d}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
