#!/usr/bin/env python3
"""Times the depth-map fusion kernels (csrc/fuse.hip) on the GPU and writes profiles/fuse.txt:

    python scripts/time_fuse.py [--res 512] [--out profiles/fuse.txt]

  * ms per surf_fuse_integrate launch at res^3 for 1, 4 and 16 views of 144 x 200 and 576 x 800, with and without colours, and the
    state bytes the launch moves per ms (tsdf + weight, + 3 colour channels: read at every point, written at the points its views
    observe, once per launch whatever the number of views: the views are looped inside the kernel);
  * ms of fuse_lattice + marching_cubes(observed_only) on the fused lattice.
Scene: a sphere of radius 0.5 in [-1, 1]^3 seen by ring cameras, analytic depth maps.  Device events around 10 launches after 3
warm-up launches; the state is reset before every series, so every launch updates a lattice of the same occupancy.

    python scripts/time_fuse.py --sparse [--res 512] [--big_res 2048] [--out profiles/fuse_sparse.txt]

times the brick-sparse path (csrc/fuse_sparse.hip) on the same scene, view counts and map sizes, stage by stage - mark, assign,
integrate, values, mesh - with bricks, allocated share and state bytes per row, at --res beside the dense path's stages measured in
the same run, and at --big_res, a lattice the dense path cannot hold."""
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


def device_timer(iters):
    def timed(fn):
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
    return timed


def sparse_main(args, dev):
    """--sparse: the brick-sparse path (csrc/fuse_sparse.hip) stage by stage at --res and at --big_res (a lattice the dense path
    cannot hold), and at --res the dense path's stages measured in the same run."""
    from surf_amd import fusion, ops
    timed = device_timer(args.iters)
    lines = [f"# scripts/time_fuse.py --sparse --res {args.res} --big_res {args.big_res}: {torch.cuda.get_device_name(0)}, trunc = 4 steps",
             f"# device events around {args.iters} repetitions after 3 warm-up ones, per stage; ms.  mark: surf_fuse_mark_bricks of all views; "
             "assign: surf_compact + surf_band_assign (one host read); integrate: ONE surf_fuse_integrate_bricks launch; values: "
             "surf_fuse_lattice on the band; mesh: marching_cubes_band(observed_only), host syncs included.  total = their sum.",
             "# dense rows (sparse = no): integrate = ONE surf_fuse_integrate launch, values = fuse_lattice, mesh = "
             "marching_cubes(observed_only) - the dense code path, measured in this run",
             "res   views  map        colours  sparse  mark     assign   integrate  values   mesh      total     bricks   alloc share  "
             "state bytes   triangles"]
    for res in (args.res, args.big_res):
        axes = [torch.linspace(-1, 1, res, device=dev) for _ in range(3)]
        trunc = 4 * 2.0 / (res - 1)
        shape = (res, res, res)
        nbp = ops.fuse_brick_dims(shape)[1]
        dense_ok = res == args.res and res ** 3 < 2 ** 31
        if dense_ok:
            d_tsdf, d_weight = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
            d_color = torch.zeros(shape + (3,), device=dev)
        for H, W in ((144, 200), (576, 800)):
            all_views = sphere_views(16, H, W, dev)
            for nv in (1, 4, 16):
                views = all_views[::16 // nv][:nv]
                lifts = [fusion.lift_transform(fusion.DepthView(v[0], None, 1.0)) for v in views]
                mark = torch.zeros(nbp ** 3, dtype=torch.uint8, device=dev)

                def do_mark():
                    for v, lift in zip(views, lifts):
                        ops.fuse_mark_bricks(mark, axes, lift, v[1], v[2], trunc)
                ms_mark = timed(do_mark)

                def do_assign():
                    do_mark()                                     # fuse_assign_bricks clears the marks
                    return ops.fuse_assign_bricks(mark)
                ms_assign = max(timed(do_assign) - ms_mark, 0.0)
                table, bricks = do_assign()
                m = int(bricks.shape[0])
                for col in (False, True):
                    tsdf, weight = torch.zeros(m * 512, device=dev), torch.zeros(m * 512, device=dev)
                    color = torch.zeros(m * 512, 3, device=dev) if col else None
                    ms_int = timed(lambda: ops.fuse_integrate_bricks(tsdf, weight, color, bricks, axes, views, trunc))
                    ms_val = timed(lambda: ops.fuse_band_values(tsdf, weight))
                    band = ops.Band(res, table, None, bricks, ops.fuse_band_values(tsdf, weight), {}, shape=shape)
                    ms_mesh = timed(lambda: ops.marching_cubes_band(band, 0.0, observed_only=True))
                    n_tri = len(ops.marching_cubes_band(band, 0.0, observed_only=True)[1])
                    state = m * (512 * (20 if col else 8) + 4) + 4 * nbp ** 3
                    total = ms_mark + ms_assign + ms_int + ms_val + ms_mesh
                    lines.append(f"{res:4d}  {nv:5d}  {H:3d} x {W:3d}  {'yes' if col else 'no ':7s}  yes     {ms_mark:7.3f}  {ms_assign:7.3f}  "
                                 f"{ms_int:9.3f}  {ms_val:7.3f}  {ms_mesh:8.3f}  {total:8.3f}  {m:7d}  {m / float(nbp ** 3):11.4f}  "
                                 f"{state:12d}  {n_tri:10d}")
                    del tsdf, weight, color, band
                    if dense_ok:
                        d_tsdf.zero_(), d_weight.zero_(), d_color.zero_()
                        ms_int = timed(lambda: ops.fuse_integrate(d_tsdf, d_weight, d_color if col else None, axes, views, trunc))
                        ms_val = timed(lambda: ops.fuse_lattice(d_tsdf, d_weight))
                        u = ops.fuse_lattice(d_tsdf, d_weight)
                        ms_mesh = timed(lambda: ops.marching_cubes(u, 0.0, observed_only=True))
                        n_tri = len(ops.marching_cubes(u, 0.0, observed_only=True)[1])
                        del u
                        lines.append(f"{res:4d}  {nv:5d}  {H:3d} x {W:3d}  {'yes' if col else 'no ':7s}  no      {0.0:7.3f}  {0.0:7.3f}  "
                                     f"{ms_int:9.3f}  {ms_val:7.3f}  {ms_mesh:8.3f}  {ms_int + ms_val + ms_mesh:8.3f}  {0:7d}  {1.0:11.4f}  "
                                     f"{res ** 3 * (20 if col else 8):12d}  {n_tri:10d}")
                del table, bricks, mark
        if dense_ok:
            del d_tsdf, d_weight, d_color
    return "\n".join(lines) + "\n"


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--out", default=None, help="default profiles/fuse.txt, with --sparse profiles/fuse_sparse.txt")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sparse", action="store_true", help="time the brick-sparse path beside the dense one (profiles/fuse_sparse.txt)")
    ap.add_argument("--big_res", type=int, default=2048, help="--sparse: a second lattice, one the dense path cannot hold")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(root, "profiles", "fuse_sparse.txt" if args.sparse else "fuse.txt")
    from surf_amd import ops
    assert torch.cuda.is_available(), "time_fuse.py measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.sparse:
        text = sparse_main(args, dev)
        print(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
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
