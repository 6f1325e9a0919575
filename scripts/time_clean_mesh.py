"""Host (numpy / scipy / torch-CPU + raster.hip) against device (mesh_clean.hip) time of the mesh cleaner, stage by stage.

The mesh: the project's marching cubes (ops.marching_cubes) on a sphere lattice, plus a few hundred copies of a sub-500-face
marching-cubes blob scattered around it (inside and outside the views), so that every stage removes something.  Five ring
cameras at 576x800 with masks that have a margin, a hole and specks.  Vertices within 1e-3 px of a pixel line in some view are
nudged off it first (the host hull test's matmul has no fixed summation order, so equality cannot be demanded on that band;
tests/test_clean_mesh_gpu.py), then per mesh size: every stage on both sides, outputs compared (they must be equal, else the
script stops before printing a time), warm-up, `--repeats` timed runs each, median and spread (min .. max), device time between
two synchronisations.  One JSON line per size.

    python scripts/time_clean_mesh.py [--resolutions 512 1280] [--radii 0.39 0.45] [--repeats 5] [--host_repeats 3]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surf_amd import ops  # noqa: E402
from surf_amd.evaluation import clean_mesh as C  # noqa: E402

H, W, NV = 576, 800, 5
AZIMUTHS = [0.0, 0.25, -0.25, 0.5, -0.5]


def _ring(azimuths, radius=2.5):
    c2ws, intrs = [], []
    for a in azimuths:
        o = torch.tensor([radius * math.sin(a), 0.0, -radius * math.cos(a)], dtype=torch.float32)
        z = -o / o.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, o
        K = torch.eye(4)
        K[0, 0] = K[1, 1] = 1.6 * W
        K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
        c2ws.append(c2w)
        intrs.append(K)
    return torch.stack(intrs), torch.stack(c2ws)


def _sphere(res, radius, dev, half=0.6):
    ax = torch.linspace(-half, half, res, device=dev)
    u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
    y, z = torch.meshgrid(ax, ax, indexing="ij")
    for i in range(res):                                   # slab by slab: no res^3 temporaries
        u[i] = radius - torch.sqrt(ax[i] * ax[i] + y * y + z * z)
    v, t = ops.marching_cubes(u, 0.0)
    del u
    return (v / (res - 1) * (2 * half) - half).cpu().numpy(), t.long().cpu().numpy()


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
    return np.concatenate(vs), np.concatenate(ts)


def _masks(seed=0):
    g = np.random.default_rng(seed)
    m = np.zeros((NV, H, W), dtype=bool)
    for i in range(NV):
        m[i, H // 12 + i:H - H // 10 - i, W // 14 + 2 * i:W - W // 16 - i] = True
        y0, x0 = int(g.integers(H // 4, H // 2)), int(g.integers(W // 4, W // 2))
        m[i, y0:y0 + H // 8, x0:x0 + W // 9] = False
        m[i][g.random((H, W)) < 0.002] ^= True
    return torch.from_numpy(m).float()


def _near(v, intrs, c2ws, eps=1e-3):
    xyz1 = np.concatenate([v, np.ones((len(v), 1))], axis=1)
    near = np.zeros(len(v), dtype=bool)
    for K, c2w in zip(intrs, c2ws):
        uvw = (xyz1 @ np.linalg.inv(c2w.double().numpy()).T)[:, :3] @ K.double().numpy()[:3, :3].T
        px, py = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        close = (px >= -1) & (px <= W) & (py >= -1) & (py <= H)
        near |= (close & ((np.abs(px - np.rint(px)) < eps) | (np.abs(py - np.rint(py)) < eps))) | (np.abs(uvw[:, 2]) < eps)
    return near


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
    if not all(np.array_equal(x, y) for x, y in zip(a, b)):
        raise SystemExit(f"time_clean_mesh: host and device disagree in stage {what}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1280],
                    help="sphere lattices (the dense marching cubes takes up to 2^31 lattice points, 1290 per axis)")
    ap.add_argument("--radii", type=float, nargs="+", default=[0.39, 0.45],
                    help="sphere radius per lattice, in a [-0.6, 0.6] box (512 / 0.39: ~1.04 M faces, 1280 / 0.45: ~8.7 M)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_repeats", type=int, default=3)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    intrs, c2ws = _ring(AZIMUTHS)
    masks = _masks()
    kw = dict(dilation_radius=11, min_nb_visible=1, upscale=2, min_component=500)
    assert len(args.radii) == len(args.resolutions)
    for res, radius in zip(args.resolutions, args.radii):
        v, f = _mesh(res, radius, dev)
        g = np.random.default_rng(1)
        for _ in range(50):
            near = _near(v, intrs, c2ws)
            if not near.any():
                break
            v[near] += g.normal(0.0, 1e-5, (int(near.sum()), 3))
        assert not _near(v, intrs, c2ws).any()
        dv, df, dm = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), masks.to(dev)
        bm = (masks > 0.5).numpy()
        R, HR = args.repeats, args.host_repeats
        host, devi = {}, {}
        dil_h, host["dilate"] = _timed(lambda: np.stack([C.dilate_disk(m, 11) for m in bm]), HR)
        dil_d, devi["dilate"] = _timed(lambda: C.dilate_disk_device(dm > 0.5, 11), R)
        _same(dil_h, dil_d, "dilate")
        dil_t = torch.from_numpy(dil_h)
        k1_h, host["visual_hull"] = _timed(lambda: C.clean_mesh_by_mask(v, f, dil_t, intrs, c2ws, 1), HR)
        k1_d, devi["visual_hull"] = _timed(lambda: C.clean_mesh_by_mask_device(dv, df, dil_d, intrs, c2ws, 1), R)
        _same(k1_h, k1_d, "visual_hull")
        f1 = f[k1_h]
        df1 = torch.from_numpy(f1).to(dev)
        k2_h, host["visible_faces"] = _timed(lambda: C.visible_faces(v, f1, masks, intrs, c2ws, 2, "cuda"), HR)
        k2_d, devi["visible_faces"] = _timed(lambda: C.visible_faces_device(dv, df1, dm, intrs, c2ws, 2), R)
        _same(k2_h, k2_d, "visible_faces")
        m2_h, host["update_faces"] = _timed(lambda: C.update_faces(v, f1, k2_h), HR)
        m2_d, devi["update_faces"] = _timed(lambda: C.update_faces_device(dv, df1, k2_d), R)
        _same(m2_h, m2_d, "update_faces")
        k3_h, host["components"] = _timed(lambda: C.face_components(m2_h[1], 500), HR)
        k3_d, devi["components"] = _timed(lambda: C.face_components_device(m2_d[1], 500), R)
        _same(k3_h, k3_d, "components")
        out_h, host["clean_mesh"] = _timed(lambda: C.clean_mesh(v, f, masks, intrs, c2ws, **kw), HR)
        out_d, devi["clean_mesh"] = _timed(lambda: C.clean_mesh(dv, df, dm, intrs, c2ws, backend="device", return_tensors=True, **kw), R)
        _same(out_h, out_d, "clean_mesh")
        _, devi["clean_mesh_numpy_io"] = _timed(lambda: C.clean_mesh(v, f, masks, intrs, c2ws, backend="device", **kw), R)
        print(json.dumps({"lattice": res, "vertices": int(len(v)), "faces": int(len(f)), "views": NV, "hw": [H, W],
                          "faces_after": {"visual_hull": int(k1_h.sum()), "visible_faces": int(k2_h.sum()),
                                          "components": int(k3_h.sum()), "clean_mesh": int(len(out_h[1]))},
                          "identical": True, "host": host, "device": devi,
                          "speedup_clean_mesh": round(host["clean_mesh"]["median_ms"] / devi["clean_mesh"]["median_ms"], 1)}), flush=True)


if __name__ == "__main__":
    main()
