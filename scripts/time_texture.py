#!/usr/bin/env python3
"""Times texture baking (surf_amd/mesh_texture.py; csrc/mesh_texture.hip) on the GPU and writes profiles/texture.txt:

    python scripts/time_texture.py [--side 708] [--views 49] [--hw 1200 1600] [--texels 8] [--host_faces 20000]

Scene: a unit sphere of 2 side^2 faces (708 -> 1.0 M) seen by --views synthetic cameras on three rings around it, each with a
procedural photograph of --hw pixels that the sphere fills; mesh, photographs and depth maps are resident on the device.
  * rasterise: mesh_depth_maps, one surf_raster_first_hit launch per view; device events around all of them.
  * pack | bake | finish: the stages of ops.bake_texture, wall clock between device synchronisations, summed over its launches
    (16 views each), mean of --iters repetitions after 1 warm-up one.
  * bake against its compulsory bytes at the 6.29 TB/s this GPU copies at (MI355X measured copy rate): per launch the accumulators
    are written (16 B a texel) and, but for the first launch, read; every view's packed records are read once (16 B a pixel; the
    four taps of a texel and those of its neighbours share lines); faces and vertices once (12 B each).  `bound/measured` is that
    ratio, reported, not a pass mark.
  * bake against the numpy mirror: mesh_texture.bake_host, one repetition, on the first --host_faces faces and all views with the
    depth maps of the whole mesh, and the device's bake stage on the same faces.
Measurements, not thresholds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29


def sphere(side):
    """A unit sphere as a side x side grid of split cells between the poles' caps: (vertices fp32, faces int32, 2 side^2 of them)."""
    th = np.linspace(0.02, np.pi - 0.02, side + 1)
    ph = np.linspace(0.0, 2.0 * np.pi, side + 1)
    t, p = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)], axis=-1).reshape(-1, 3).astype(np.float32)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(side), np.arange(side), indexing="ij"))
    p00, p10, p11, p01 = i * (side + 1) + j, (i + 1) * (side + 1) + j, (i + 1) * (side + 1) + j + 1, i * (side + 1) + j + 1
    return v, np.concatenate([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)]).astype(np.int32)


def cameras(count, H, W):
    """count projections (3, 4) fp32 looking at the origin from distance 3, on rings 0, 30 and 60 degrees above the XY plane."""
    out = []
    for k in range(count):
        az, el = 0.4 + 2.399963 * k, np.radians((0.0, 30.0, 60.0)[k % 3])
        c = 3.0 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        f = 0.9 * (min(H, W) / 2) * np.sqrt(8.0)                  # the sphere's silhouette has tan = 1 / sqrt(8): it fills 90 %
        K = np.array([[f, 0.0, (W - 1) / 2], [0.0, f, (H - 1) / 2], [0.0, 0.0, 1.0]])
        out.append((K @ np.concatenate([R, (-R @ c)[:, None]], axis=1)).astype(np.float32))
    return out


def photograph(k, H, W, dev):
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    return torch.stack([0.5 + 0.4 * torch.sin(0.05 * x + k), 0.5 + 0.4 * torch.cos(0.04 * y - k), 0.5 + 0.4 * torch.sin(0.03 * (x + y))],
                       dim=-1).contiguous()


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--side", type=int, default=708)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--hw", type=int, nargs=2, default=[1200, 1600])
    ap.add_argument("--texels", type=int, default=8)
    ap.add_argument("--host_faces", type=int, default=20000, help="faces the numpy mirror is timed on (0: none)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "texture.txt"))
    args = ap.parse_args(argv)
    from surf_amd import mesh_texture as MT
    from surf_amd import ops
    assert torch.cuda.is_available(), "time_texture.py measures on the GPU"
    dev = torch.device("cuda:0")
    H, W = args.hw
    T, K = args.texels, args.views
    depth_tol, min_cos = 0.02, 0.2
    v32, f32 = sphere(args.side)
    n, m = len(v32), len(f32)
    _, cols, rows, Ha, Wa = MT.atlas_layout(m, T)
    dv, df = torch.from_numpy(v32).to(dev), torch.from_numpy(f32).to(dev)
    Ps = cameras(K, H, W)
    images = [photograph(k, H, W, dev) for k in range(K)]

    raster_ms = []
    for it in range(1 + args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        depths = [ops.raster_depth(dv, df, P, (H, W)) for P in Ps]                  # what mesh_depth_maps launches per view
        e1.record()
        torch.cuda.synchronize()
        if it >= 1:
            raster_ms.append(e0.elapsed_time(e1))
    packed = [(P.reshape(12), MT.view_centre(P), image, depth) for P, image, depth in zip(Ps, images, depths)]

    def device_stages(faces, layout):
        sums = {}
        for it in range(1 + args.iters):
            st = []
            out = ops.bake_texture(dv, faces, packed, T, layout[1], layout[2], depth_tol, min_cos, stages=st)
            if it >= 1:
                for name, ms in st:
                    sums[name] = sums.get(name, 0.0) + ms / args.iters
        return sums, out

    stages, (atlas, acc, _) = device_stages(df, (None, cols, rows))
    seen = float((acc[..., 3] > 0).sum()) / (m * T * (T + 1) // 2)
    launches = -(-K // ops.FUSE_MAX_VIEWS)
    texels = Ha * Wa
    nbytes = texels * 16 * (2 * launches - 1) + K * H * W * 16 + 12 * m + 12 * n
    bound = nbytes / (COPY_TBS * 1e12) * 1e3
    lines = [f"# scripts/time_texture.py: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"# rasterise: device events around the {K} launches of mesh_depth_maps; pack | bake | finish: wall clock between device "
             f"synchronisations inside ops.bake_texture, summed over its {launches} launches; means of {args.iters} repetitions "
             "after 1 warm-up one; everything resident on the device",
             f"# bound = the bake's compulsory bytes (see the script) at {COPY_TBS} TB/s (the measured copy rate).  Reported, not a pass mark.",
             f"sphere {args.side} x {args.side}: {n} vertices, {m} faces, T = {T}: atlas {Ha} x {Wa} = {texels} texels, "
             f"{K} views of {H} x {W}, seen share {seen:.3f}",
             f"  device  rasterise {np.mean(raster_ms):9.3f} | pack {stages['pack']:8.3f} | bake {stages['bake']:9.3f} | finish "
             f"{stages['finish']:7.3f}   ms",
             f"  bake    {stages['bake']:9.3f} ms   bytes {nbytes / 1e6:9.1f} MB   bound {bound:7.3f} ms   bound/measured "
             f"{bound / stages['bake']:5.2f}   ({nbytes / 1e9 / stages['bake']:5.2f} TB/s of compulsory bytes)"]
    if args.host_faces:
        sub = np.ascontiguousarray(f32[:args.host_faces])
        layout = MT.atlas_layout(len(sub), T)
        dsub, _ = device_stages(torch.from_numpy(sub).to(dev), layout)
        host_views = [(P.reshape(12), MT.view_centre(P), image.cpu().numpy(), depth.cpu().numpy()) for P, image, depth in zip(Ps, images, depths)]
        t0 = time.perf_counter()
        MT.bake_host(v32, sub, T, host_views, depth_tol, min_cos, 4, False, 0.0, np.empty((layout[3], layout[4], 4), np.float32))
        host_ms = 1e3 * (time.perf_counter() - t0)
        lines.append(f"  first {len(sub)} faces ({layout[3] * layout[4]} texels), all {K} views: device bake {dsub['bake']:8.3f} ms   "
                     f"numpy mirror (bake_host, one thread, one repetition) {host_ms:10.1f} ms   ratio {host_ms / dsub['bake']:8.0f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
