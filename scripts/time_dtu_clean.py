"""Host (numpy / scipy + raster.hip) against device (dtu_clean.hip, mesh_clean.hip) time of the DTU protocol's mesh cleaner
(surf_amd.evaluation.clean_dtu), stage by stage.

The mesh: the project's marching cubes on a sphere lattice, scaled to millimetres (radius ~70 mm around the origin), plus a few
hundred sub-500-face blobs scattered around it so that every stage removes something.  Three ring cameras about 600 mm away with
DTU's intrinsics and three synthetic 1200 x 1600 masks (ellipse, rectangle on two borders, blob with a hole).  Per mesh size:
every stage on both sides, outputs compared (they must be EQUAL, else the script stops before printing a time), one warm-up,
`--host_repeats` / `--repeats` timed runs, median and spread (min .. max), device time between two synchronisations.  One JSON
line per size.

    python scripts/time_dtu_clean.py [--resolutions 512 1280] [--radii 0.39 0.45] [--repeats 5] [--host_repeats 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surf_amd import ops  # noqa: E402
from surf_amd.evaluation import clean_dtu as D  # noqa: E402
from surf_amd.evaluation import clean_mesh as C  # noqa: E402

H, W = 1200, 1600
K = np.array([[2892.33, 0.0, 823.2], [0.0, 2883.18, 619.07], [0.0, 0.0, 1.0]])
MM = 150.0                                                 # lattice box [-0.6, 0.6] -> +-90 mm


def _projections(n=3, radius=600.0):
    out = []
    K4 = np.eye(4, dtype=np.float32)
    K4[:3, :3] = K
    for i in range(n):
        a = 0.35 * (i - n // 2)
        o = np.array([radius * np.sin(a), 25.0 * i - 20.0, -radius * np.cos(a)])
        z = -o / np.linalg.norm(o)
        x = np.cross([0, 1.0, 0], z)
        x /= np.linalg.norm(x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, o
        out.append(K4 @ np.linalg.inv(c2w).astype(np.float32))
    return out


def _masks():
    yy, xx = np.mgrid[:H, :W].astype(np.int64)
    a, b = (5 * W) // 16, (5 * H) // 24
    m0 = ((xx - W // 2) ** 2) * b * b + ((yy - H // 2) ** 2) * a * a <= a * a * b * b
    m1 = (yy < (7 * H) // 10) & (xx >= (4 * W) // 10)
    r = H // 5
    m2 = ((xx - W // 2) ** 2 + (yy - H // 2) ** 2 <= r * r) | ((xx - W // 2 - r) ** 2 + (yy - H // 2 + r // 2) ** 2 <= (3 * r // 4) ** 2)
    m2 &= (xx - W // 2) ** 2 + (yy - H // 2) ** 2 > (r // 3) ** 2
    return [m.astype(np.uint8) * 255 for m in (m0, m1, m2)]


def _sphere(res, radius, dev, half=0.6):
    ax = torch.linspace(-half, half, res, device=dev)
    u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
    y, z = torch.meshgrid(ax, ax, indexing="ij")
    for i in range(res):                                   # slab by slab: no res^3 temporaries
        u[i] = radius - torch.sqrt(ax[i] * ax[i] + y * y + z * z)
    v, t = ops.marching_cubes(u, 0.0)
    del u
    return (v / (res - 1) * (2 * half) - half).double().cpu().numpy(), t.long().cpu().numpy()


def _mesh(res, radius, dev, n_floaters=300, seed=0):
    v, t = _sphere(res, radius, dev)
    bv, bt = _sphere(8, 0.5, dev)
    assert len(bt) < 500
    g = np.random.default_rng(seed)
    d = g.standard_normal((n_floaters, 3))
    centres = d / np.linalg.norm(d, axis=1, keepdims=True) * g.uniform(0.5, 0.7, (n_floaters, 1))
    vs, ts, off = [v], [t], len(v)
    for c in centres:
        vs.append(bv * 0.03 + c[None])
        ts.append(bt + off)
        off += len(bv)
    return np.concatenate(vs) * MM, np.concatenate(ts)


def _timed(fn, repeats):
    """Median, min, max in ms of `repeats` runs after one warm-up, synchronised on both sides; and the last result."""
    out = fn()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "repeats": repeats}


def _same(a, b, what):
    a = [x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a if isinstance(a, tuple) else (a,))]
    b = [x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (b if isinstance(b, tuple) else (b,))]
    if len(a) != len(b) or not all(np.array_equal(x, y) for x, y in zip(a, b)):
        raise SystemExit(f"time_dtu_clean: host and device disagree in stage {what}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1280])
    ap.add_argument("--radii", type=float, nargs="+", default=[0.39, 0.45],
                    help="sphere radius per lattice, in a [-0.6, 0.6] box (512 / 0.39: ~1 M faces, 1280 / 0.45: ~8.7 M)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_repeats", type=int, default=3)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    P_list, masks = _projections(), _masks()
    dmasks = torch.from_numpy(np.stack(masks)).to(dev)
    assert len(args.radii) == len(args.resolutions)
    for res, radius in zip(args.resolutions, args.radii):
        v, f = _mesh(res, radius, dev)
        dv, df = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        R, HR = args.repeats, args.host_repeats
        host, devi = {}, {}
        dil_h, host["dilate"] = _timed(lambda: np.stack([D.dilate_ellipse(m, 11) for m in masks]), HR)
        dil_d, devi["dilate"] = _timed(lambda: D.dilate_ellipse_device(dmasks, 11), R)
        _same(dil_h, dil_d, "dilate")
        c_h, host["points_in_masks"] = _timed(lambda: D.points_in_masks(v, P_list, dil_h, None), HR)
        c_d, devi["points_in_masks"] = _timed(lambda: D.points_in_masks_device(dv, P_list, dil_d, None), R)
        _same(c_h, c_d, "points_in_masks")
        m1_h, host["remove_vertices"] = _timed(lambda: D.clean_faces_by_mask(v, f, c_h, 1), HR)
        m1_d, devi["remove_vertices"] = _timed(lambda: D.clean_faces_by_mask_device(dv, df, c_d, 1), R)
        _same(m1_h, m1_d, "remove_vertices")
        m2_h, host["outside_frustum"] = _timed(lambda: D.clean_faces_outside_frustum(m1_h[0], m1_h[1], P_list, dil_h, None), HR)
        m2_d, devi["outside_frustum"] = _timed(lambda: D.clean_faces_outside_frustum_device(m1_d[0], m1_d[1], P_list, dil_d, None), R)
        _same(m2_h, m2_d, "outside_frustum")
        out_h, host["clean_dtu"] = _timed(lambda: D.clean_dtu(v, f, P_list, masks), HR)
        out_d, devi["clean_dtu"] = _timed(lambda: D.clean_dtu(dv, df, P_list, dmasks, backend="device", return_tensors=True), R)
        _same(out_h, out_d, "clean_dtu")
        _same(out_h, m2_h, "clean_dtu against its stages")
        _, devi["clean_dtu_numpy_io"] = _timed(lambda: D.clean_dtu(v, f, P_list, masks, backend="device"), R)
        print(json.dumps({"lattice": res, "vertices": int(len(v)), "faces": int(len(f)), "views": len(P_list), "hw": [H, W],
                          "faces_after": {"remove_vertices": int(len(m1_h[1])), "clean_dtu": int(len(out_h[1]))},
                          "components_of_500": int(C.face_components(out_h[1], 500).sum()),
                          "identical": True, "host": host, "device": devi,
                          "speedup_clean_dtu": round(host["clean_dtu"]["median_ms"] / devi["clean_dtu"]["median_ms"], 1)}), flush=True)


if __name__ == "__main__":
    main()
