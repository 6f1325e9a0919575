#!/usr/bin/env python3
"""Times ray casting of the fused TSDF (csrc/ray_cast.hip) on the GPU and writes profiles/raycast.txt:

    python scripts/time_raycast.py [--res 512] [--big_res 2048] [--out profiles/raycast.txt]

ms per 576 x 800 view (depth + normal + colour, device tensors: FusionVolume.ray_cast(return_tensors=True)) of
  * the dense path at res^3 and the brick-sparse path at res^3 and at big_res^3 (a lattice the dense volume cannot hold),
    from the camera of a fused view and from a camera none of the views had, with z_min = 0 and with z_min just in front of the
    surface (the difference is the walk through free space in front of the model);
  * today's only alternative for the same view on the same state: FusionVolume.extract_mesh() followed by ops.raster_first_hit
    (upload of the mesh as fp32 / int32 included; it yields face ids - depth, normal and colour would still have to be
    interpolated from them).
Scene: a sphere of radius 0.5 in [-1, 1]^3 fused from 16 ring cameras' analytic 576 x 800 depth maps with colours, trunc = 4
steps.  Device events around --iters calls after 3 warm-up calls; the mesh path, which ends on the host, by a host clock around
calls that end in a device synchronise."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 576, 800
RADIUS, DIST = 0.5, 2.5


def ring_camera(a, dist=DIST, lift=0.3):
    """(K (3, 3), c2w (4, 4)) of a camera on the ring at angle a looking at the origin; the unit box about fills the width."""
    f = 0.9 * W / (2 * 1.0 / dist)
    c = np.array([dist * np.sin(a), lift * np.sin(2 * a), -dist * np.cos(a)])
    z = -c / np.linalg.norm(c)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), c
    return np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]]), c2w


def sphere_view(K, c2w, dev):
    from surf_amd.fusion import DepthView
    c = c2w[:3, 3]
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    b, cc, aa = d @ c, c @ c - RADIUS * RADIUS, (d * d).sum(-1)
    disc = b * b - aa * cc
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / aa, 0.0)
    depth = torch.from_numpy(np.where(t > 0, t, 0.0).astype(np.float32)).to(dev)
    return DepthView((K @ np.linalg.inv(c2w)[:3, :4]).astype(np.float32), depth, 1.0, torch.rand(H, W, 3, device=dev))


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--big_res", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "raycast.txt"))
    args = ap.parse_args(argv)
    from surf_amd import ops
    from surf_amd.fusion import FusionVolume
    assert torch.cuda.is_available(), "time_raycast.py measures on the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def wall(fn, iters=3):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / iters, out

    cams = [ring_camera(2 * np.pi * i / 16) for i in range(16)]
    views = [sphere_view(K, c2w, dev) for K, c2w in cams]
    novel = ring_camera(2 * np.pi * 0.5 / 16, dist=1.6, lift=0.8)            # between two views, closer, higher
    targets = [("fused view 0", cams[0], DIST), ("novel camera", novel, 1.6)]
    lines = [f"# scripts/time_raycast.py --res {args.res} --big_res {args.big_res}: {torch.cuda.get_device_name(0)}; {H} x {W} rays per view; "
             "state fused from 16 views with colours, trunc = 4 steps",
             f"# ray cast: device events around {args.iters} calls of FusionVolume.ray_cast(return_tensors=True) (depth + normal + colour) "
             "after 3 warm-up calls, ms per view.  z_min 'near' = 2 x trunc in front of the sphere: what remains is the walk through "
             "the band; the rest of the z_min = 0 time is the walk through cells in front of it.",
             "# mesh path: host clock around 3 calls (after one warm-up call) that end in a device synchronise, ms: extract_mesh() as "
             "the public interface returns it (host arrays), then upload as fp32 / int32 + ops.raster_first_hit (face ids only).",
             "res   state   camera        hits     ray cast z_min=0  z_min near   extract_mesh  raster_first_hit  mesh path   triangles  bricks"]
    for res, sparse in ((args.res, False), (args.res, True), (args.big_res, True)):
        voxel = 2.0 / (res - 1)
        vol = FusionVolume((np.full(3, -1.0), np.full(3, 1.0), voxel), trunc=4 * voxel, colors=True, device=dev, sparse=sparse)
        assert vol.shape == (res, res, res)
        vol.integrate(views)
        if sparse:
            vol.finalize()
        torch.cuda.synchronize()
        ms_extract, mesh = wall(vol.extract_mesh)
        v32, t32 = mesh[0].astype(np.float32), mesh[1].astype(np.int32)
        for name, (K, c2w), dist in targets:
            P = (K @ np.linalg.inv(c2w)[:3, :4]).astype(np.float32)
            near = max(dist - RADIUS - 8 * voxel, 0.0)
            ms0 = timed(lambda: vol.ray_cast(P, (H, W), return_tensors=True))
            ms1 = timed(lambda: vol.ray_cast(P, (H, W), z_min=near, return_tensors=True))
            hits = int((vol.ray_cast(P, (H, W), return_tensors=True)["depth"] > 0).sum())
            K4 = np.eye(4)
            K4[:3, :3] = K
            intr, pose = torch.from_numpy(K4).float(), torch.from_numpy(c2w).float()
            ms_raster, _ = wall(lambda: ops.raster_first_hit(torch.from_numpy(v32).to(dev), torch.from_numpy(t32).to(dev), intr, pose, (H, W)))
            lines.append(f"{res:4d}  {'sparse' if sparse else 'dense ':6s}  {name:12s}  {hits:7d}  {ms0:16.3f}  {ms1:10.3f}  {ms_extract:13.3f}  "
                         f"{ms_raster:16.3f}  {ms_extract + ms_raster:9.3f}  {len(t32):10d}  {vol.n_bricks if sparse else 0:6d}")
        del vol, mesh, v32, t32
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
