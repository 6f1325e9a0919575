#!/usr/bin/env python3
"""Times the depth-map fusion kernels (csrc/fuse.hip) on the GPU and writes profiles/fuse.txt:

    python scripts/time_fuse.py [--res 512] [--out profiles/fuse.txt]

  * ms per surf_fuse_integrate launch at res^3 for 1, 4 and 16 views of 144 x 200 and 576 x 800, with and without colours, and the
    state bytes the launch moves per ms (tsdf + weight, + 3 colour channels: read at every point, written at the points its views
    observe, once per launch whatever the number of views: the views are looped inside the kernel);
  * ms of fuse_lattice + marching_cubes(observed_only) on the fused lattice.
Scene: a sphere of radius 0.5 in [-1, 1]^3 seen by ring cameras, analytic depth maps.  Device events around 10 launches after 3
warm-up launches; the state is reset before every series, so every launch updates a lattice of the same occupancy."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sphere_views(n, H, W, dev, radius=0.5, dist=2.5):
    """n ring cameras looking at the origin with the analytic z-depth of the sphere |p| = radius (0 off the sphere)."""
    views = []
    f = 0.9 * W / (2 * 1.0 / dist)                      # the unit box about fills the image width
    for i in range(n):
        a = 2 * np.pi * i / max(n, 1)
        c = np.array([dist * np.sin(a), 0.3 * np.sin(2 * a), -dist * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.stack([x, y, z], axis=1), c
        K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
        yy, xx = np.mgrid[:H, :W].astype(np.float64)
        d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
        b, cc, aa = (d @ c), c @ c - radius * radius, (d * d).sum(-1)
        disc = b * b - aa * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / aa, 0.0)
        depth = torch.from_numpy(np.where(t > 0, t, 0.0).astype(np.float32)).to(dev)
        image = torch.rand(H, W, 3, device=dev)
        views.append(((K @ np.linalg.inv(c2w)[:3, :4]).astype(np.float32), depth, 1.0, image))
    return views


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fuse.txt"))
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args(argv)
    from surf_amd import ops
    assert torch.cuda.is_available(), "time_fuse.py measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = args.res
    n = res ** 3
    axes = [torch.linspace(-1, 1, res, device=dev) for _ in range(3)]
    trunc = 4 * 2.0 / (res - 1)
    tsdf, weight = torch.zeros(res, res, res, device=dev), torch.zeros(res, res, res, device=dev)
    color = torch.zeros(res, res, res, 3, device=dev)
    lines = [f"# scripts/time_fuse.py --res {res}: {torch.cuda.get_device_name(0)}, lattice {res}^3 = {n} points, trunc = 4 steps",
             f"# device events around {args.iters} launches after 3 warm-up launches; state bytes of a launch = (tsdf + weight [+ 3 colour "
             "channels]) read at every point + written at the points the launch's views observe (the others are not written)",
             "# surf_fuse_integrate",
             "views  map        colours  ms/launch  ms/view  observed  state GB  state GB per ms (= TB/s)"]

    def timed(fn, iters):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for H, W in ((144, 200), (576, 800)):
        all_views = sphere_views(16, H, W, dev)
        for nv in (1, 4, 16):
            for col in (False, True):
                tsdf.zero_(), weight.zero_(), color.zero_()
                views = all_views[::16 // nv][:nv]
                ms = timed(lambda: ops.fuse_integrate(tsdf, weight, color if col else None, axes, views, trunc), args.iters)
                share = float((weight > 0).sum()) / n           # every launch of the series updates exactly these points
                gb = n * (8 + (12 if col else 0)) * (1.0 + share) / 1e9
                lines.append(f"{nv:5d}  {H:3d} x {W:3d}  {'yes' if col else 'no ':7s}  {ms:9.3f}  {ms / nv:7.3f}  {share:8.3f}  {gb:8.3f}  "
                             f"{gb / ms:8.3f}")
    # ---- the mesh step on a lattice fused from 16 views ----
    tsdf.zero_(), weight.zero_()
    ops.fuse_integrate(tsdf, weight, None, axes, sphere_views(16, 144, 200, dev), trunc)
    ms_lat = timed(lambda: ops.fuse_lattice(tsdf, weight), args.iters)
    u = ops.fuse_lattice(tsdf, weight)
    ms_mc = timed(lambda: ops.marching_cubes(u, 0.0, observed_only=True), args.iters)
    v, t = ops.marching_cubes(u, 0.0, observed_only=True)
    share = float((weight > 0).sum()) / n
    lines += ["# mesh step on the lattice fused from 16 views of 144 x 200 "
              f"(observed share {share:.3f}, {len(v)} vertices, {len(t)} triangles)",
              f"fuse_lattice                    {ms_lat:9.3f} ms   ({n * 12 / 1e9 / ms_lat:.3f} GB per ms)",
              f"marching_cubes(observed_only)   {ms_mc:9.3f} ms   (classify, compact, count, emit, drop of unreferenced vertices; "
              "host syncs included)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
