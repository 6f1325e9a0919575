"""Tanks and Temples evaluation (the protocol of the benchmark's published Python toolbox), which is also ETH3D's accuracy /
completeness / F1 at a list of tolerances: align the reconstruction to the laser scan (one 4x4, refined by three rounds of
point-to-point ICP), crop both clouds to the scene's polygon volume, voxel-down-sample both at tau / 2, then

    precision = share of reconstructed points nearer than tau to the scan, recall = share of scan points nearer than tau to the
    reconstruction, fscore = 2 P R / (P + R), and the cumulative curves of both up to 5 tau.

    python -m surf_amd.evaluation.fscore --pred fused.ply --gt_dir <T&T ground truth> --scene Barn [--mode mesh] [--tau X]
        [--device gpu] [--no_refine] [--taus 0.01 0.02 ...]          -> one JSON line

<gt_dir>/<scene>/ holds <scene>.ply (the scan), <scene>.json (the crop volume, Open3D's SelectionPolygonVolume) and
<scene>_trans.txt (a 4x4 from the reconstruction's frame to the scan's).  The toolbox derives its initial alignment from the
camera trajectory logs; here the caller supplies ONE 4x4 (default: <scene>_trans.txt) and ICP refines it.

Two paths that give the same arrays stage by stage: numpy + scikit-learn's kd-tree (device="cpu") and surf_amd/csrc/fscore.hip
(device="gpu").  The rules both follow, all in float64:
  transform   p' = ((R[k,0]*x + R[k,1]*y) + R[k,2]*z) + t[k], separate multiplies and adds.
  crop        orthogonal axis a, (u, v) the two other axes in increasing order; kept iff axis_min <= p[a] <= axis_max and the
              crossing number over the polygon's edges (i, j = i - 1) is odd:
              ((v_i > v) != (v_j > v)) and u < (u_j - u_i) * (v - v_i) / (v_j - v_i) + u_i.
  voxel mean  Open3D's voxel_down_sample: origin = min(points) - voxel / 2, cell = floor((p - origin) / voxel), one output point
              per occupied cell in ascending (x << 42) | (y << 21) | z order (at most 2^21 cells per axis), each coordinate the
              sum of the members IN INPUT ORDER over their number.
  nearest     min of (dx*dx + dy*dy) + dz*dz, one sqrt; +inf / -1 where that is >= max_dist.  The device breaks exact ties to
              the smallest index, the kd-tree to whichever it meets.
  icp         point-to-point, rigid, no scale: per iteration transform, nearest, keep d < max_dist; fitness = kept / n, rmse =
              sqrt(mean d^2); stop when |dfitness| and |drmse| are both below rel_tol (Open3D's criterion) or after max_iter
              updates; else centroids, then the CENTRED cross-covariance in a second pass, Kabsch by a host 3x3 SVD.
The crop's edge rule, the voxel origin, the ICP convergence test and the three-round schedule are restated from the published
toolbox / Open3D; Open3D is not a dependency and they are not checked against it."""
import argparse
import json
import time
from collections import namedtuple

import numpy as np

from .dtu_eval import _check_device, sample_mesh_points, sample_mesh_points_gpu

# the benchmark's per-scene distance threshold tau, in the scan's units (metres)
SCENE_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
             "Truck": 0.005}
AXIS_CELLS = 1 << 21             # cells per axis of the voxel grid (63-bit keys)
ICP_ROUND_POINTS = 4_000_000     # the last ICP round strides the clouds down to this many points

CropVolume = namedtuple("CropVolume", "axis axis_min axis_max polygon")     # axis "X"|"Y"|"Z", polygon (k, 3) float64


def read_crop_volume(json_path):
    """Open3D's SelectionPolygonVolume JSON: orthogonal_axis, axis_min, axis_max, bounding_polygon [[x, y, z], ...]."""
    with open(json_path) as f:
        d = json.load(f)
    axis = str(d["orthogonal_axis"]).upper()
    if axis not in ("X", "Y", "Z"):
        raise ValueError(f"{json_path}: orthogonal_axis must be X, Y or Z, got {d['orthogonal_axis']!r}")
    poly = np.asarray(d["bounding_polygon"], dtype=np.float64).reshape(-1, 3)
    if len(poly) < 3:
        raise ValueError(f"{json_path}: bounding_polygon needs at least three vertices")
    return CropVolume(axis, float(d["axis_min"]), float(d["axis_max"]), poly)


def _crop_axes(crop):
    a = "XYZ".index(crop.axis)
    u, v = [k for k in range(3) if k != a]
    return a, u, v


# ---- host / device dispatch: a cloud is a numpy array on the host path and a cuda tensor on the device path ----

def _is_tensor(a):
    return type(a).__module__.startswith("torch")


def _dev(a):
    """(n, 3) float64 cuda tensor of a numpy array or a tensor."""
    import torch
    if not _is_tensor(a):
        a = torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1, 3))          # a copy: the caller's array may be read-only
    return a.to("cuda", torch.float64).contiguous()


def _host(a):
    if _is_tensor(a):
        a = a.cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 3))


def _back(out, like):
    """Results go back as what the caller gave: numpy for numpy, tensors for tensors."""
    return out if _is_tensor(like) else out.cpu().numpy()


def transform_points(points, T, device="cpu"):
    """R p + t with the rule above; T a 4x4 whose last row is not read."""
    _check_device(device)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    if device == "gpu":
        from .. import ops
        return _back(ops.fscore_transform(_dev(points), T), points)
    p = _host(points)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(3)], axis=1)


def crop_points(points, crop, device="cpu"):
    """keep (n,) bool: the points inside the polygon volume, by the rule above."""
    _check_device(device)
    a, ua, va = _crop_axes(crop)
    poly = np.ascontiguousarray(np.asarray(crop.polygon, dtype=np.float64)[:, [ua, va]])
    if device == "gpu":
        import torch
        from .. import ops
        return _back(ops.fscore_crop(_dev(points), a, crop.axis_min, crop.axis_max, torch.from_numpy(poly).to("cuda")), points)
    p = _host(points)
    u, v = p[:, ua], p[:, va]
    inside = np.zeros(len(p), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):           # a horizontal edge divides by zero where the first test fails
        for i in range(len(poly)):
            (ui, vi), (uj, vj) = poly[i], poly[i - 1]
            inside ^= ((vi > v) != (vj > v)) & (u < (uj - ui) * (v - vi) / (vj - vi) + ui)
    return (crop.axis_min <= p[:, a]) & (p[:, a] <= crop.axis_max) & inside


def voxel_mean(points, voxel, device="cpu"):
    """(m, 3) float64: one point per occupied voxel, by the rule above."""
    _check_device(device)
    if not (voxel > 0 and np.isfinite(voxel)):
        raise ValueError(f"voxel_mean: voxel must be finite and > 0, got {voxel}")
    if device == "gpu":
        from .. import ops
        return _back(ops.fscore_voxel_mean(_dev(points), float(voxel)), points)
    p = _host(points)
    if len(p) == 0:
        return np.zeros((0, 3))
    origin = p.min(axis=0) - voxel / 2
    cell = np.floor((p - origin) / voxel).astype(np.int64)
    if cell.max() >= AXIS_CELLS:
        raise ValueError(f"voxel_mean: the cloud spans {int(cell.max()) + 1} voxels of {voxel} along an axis, the limit is {AXIS_CELLS}")
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    _, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    # bincount adds its weights one after the other in index order: the sum the device forms per segment
    return np.stack([np.bincount(inv, weights=p[:, k], minlength=len(counts)) / counts for k in range(3)], axis=1)


def _nearest_host(q, ref, max_dist):
    import sklearn.neighbors as skln
    if len(q) == 0 or len(ref) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, dtype=np.int64)
    nn = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=-1).fit(ref)
    return _cap(*nn.kneighbors(q, n_neighbors=1, return_distance=True), max_dist)


def _cap(dist, index, max_dist):
    dist, index = dist.reshape(-1).astype(np.float64), index.reshape(-1).astype(np.int64)
    far = ~(dist < max_dist)
    dist[far] = np.inf
    index[far] = -1
    return dist, index


def nearest(queries, ref, max_dist, device="cpu"):
    """(dist (n,) float64, +inf where >= max_dist; index (n,) int64 into ref, -1 there)."""
    _check_device(device)
    if not (max_dist > 0 and np.isfinite(max_dist)):
        raise ValueError(f"nearest: max_dist must be finite and > 0, got {max_dist}")
    if device == "gpu":
        from .. import ops
        d, i = ops.nearest_capped_index(_dev(queries), _dev(ref), float(max_dist))
        return _back(d, queries), _back(i, queries)
    return _nearest_host(_host(queries), _host(ref), max_dist)


def _kabsch(cs, ct, H):
    """The rotation and translation that take the centred source onto the centred target: H = sum (s - cs)(t - ct)^T."""
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])       # a reflection is turned back
    R = Vt.T @ D @ U.T
    upd = np.eye(4)
    upd[:3, :3] = R
    upd[:3, 3] = ct - R @ cs
    return upd


def icp(source, target, init, max_dist, max_iter=20, rel_tol=1e-6, device="cpu"):
    """Point-to-point rigid ICP by the rule above.  Returns (T (4, 4) float64, fitness, rmse, iterations): T takes `source` onto
    `target`, starting at `init`; iterations counts the updates applied."""
    _check_device(device)
    T = np.array(init, dtype=np.float64).reshape(4, 4)
    gpu = device == "gpu"
    if gpu:
        from .. import ops
        src0, tgt = _dev(source), _dev(target)
        table = ops.NearestTable(tgt) if tgt.shape[0] else None
    else:
        import sklearn.neighbors as skln
        src0, tgt = _host(source), _host(target)
        tree = skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=-1).fit(tgt) if len(tgt) else None
    n = src0.shape[0]
    if n == 0 or tgt.shape[0] == 0:
        raise ValueError("icp: empty cloud")
    prev, it = None, 0
    while True:
        if gpu:
            src = ops.fscore_transform(src0, T)
            dist, index = table.query(src, float(max_dist))
            s = ops.fscore_icp_sums(src, tgt, index, dist).cpu().numpy()
            kept = int(s[0])
        else:
            src = transform_points(src0, T)
            dist, index = _cap(*tree.kneighbors(src, n_neighbors=1, return_distance=True), max_dist)
            pair = index >= 0
            kept = int(pair.sum())
            ps, pt = src[pair], tgt[index[pair]]
            s = np.concatenate([[kept], ps.sum(axis=0), pt.sum(axis=0), [(dist[pair] ** 2).sum()]])
        fitness = kept / n
        rmse = float(np.sqrt(s[7] / kept)) if kept else 0.0
        if prev is not None and abs(fitness - prev[0]) < rel_tol and abs(rmse - prev[1]) < rel_tol:
            break
        if it >= max_iter or kept < 3:
            break
        prev = (fitness, rmse)
        cs, ct = s[1:4] / kept, s[4:7] / kept
        if gpu:
            H = ops.fscore_icp_cov(src, tgt, index, cs, ct).cpu().numpy()
        else:
            H = (ps - cs).T @ (pt - ct)
        T = _kabsch(cs, ct, H) @ T
        it += 1
    return T, fitness, rmse, it


def fscore(dist_pred_to_gt, dist_gt_to_pred, tau):
    """(precision, recall, fscore) at tau: shares of distances strictly below tau; fscore 0 when both are 0."""
    d1, d2 = np.asarray(dist_pred_to_gt).reshape(-1), np.asarray(dist_gt_to_pred).reshape(-1)
    if len(d1) == 0 or len(d2) == 0:
        raise ValueError("fscore: empty distance list")
    p = float(np.count_nonzero(d1 < tau)) / len(d1)
    r = float(np.count_nonzero(d2 < tau)) / len(d2)
    return p, r, (2 * p * r / (p + r) if p + r > 0 else 0.0)


def cumulative_curve(dist, tau):
    """The toolbox's curve: the share of distances below each edge of np.arange(0, 5 tau, tau / 100) after the first."""
    d = np.asarray(dist).reshape(-1)
    hist, _ = np.histogram(d[np.isfinite(d)], np.arange(0, 5 * tau, tau / 100))
    return np.cumsum(hist) / len(d)


def default_schedule(tau):
    """The published toolbox's three ICP rounds: (down-sampling, max_dist, max_iter)."""
    return [(("voxel", tau), 80 * tau, 20), (("voxel", tau / 2), 20 * tau, 20), (("stride_to", ICP_ROUND_POINTS), 2 * tau, 20)]


def _down(points, spec, device):
    kind, value = spec
    if kind == "voxel":
        return voxel_mean(points, value, device)
    if kind == "stride_to":
        k = max(1, -(-points.shape[0] // int(value)))                   # every k-th point: at most `value` remain
        return points[::k] if k > 1 else points
    raise ValueError(f"schedule: down-sampling must be ('voxel', v) or ('stride_to', n), got {spec!r}")


def _cropped(points, crop, device, stage):
    if crop is not None:
        points = points[crop_points(points, crop, device)]
    if points.shape[0] == 0:
        raise ValueError(f"evaluate_points: no point left after the crop ({stage})")
    return points


def evaluate_points(pred, gt, tau, transform=None, crop=None, voxel=None, refine=True, schedule=None, taus=(), device="cpu"):
    """The protocol on two clouds (n, 3): `transform` (4x4, default identity) takes pred into gt's frame and is refined by the ICP
    schedule (refine=False: used as it is); both clouds are cropped, voxel-down-sampled at `voxel` (default tau / 2) and measured
    against each other up to 5 max(tau, *taus).  Returns a dict: precision, recall, fscore; taus (one dict per extra tolerance);
    curve_precision, curve_recall; transform; icp (per round fitness, rmse, iterations); counts; ms per stage."""
    _check_device(device)
    if not (tau > 0 and np.isfinite(tau)):
        raise ValueError(f"evaluate_points: tau must be finite and > 0, got {tau}")
    taus = [float(t) for t in taus]
    voxel = tau / 2 if voxel is None else float(voxel)
    to = _dev if device == "gpu" else _host
    pred, gt = to(pred), to(gt)
    T = np.eye(4) if transform is None else np.array(transform, dtype=np.float64).reshape(4, 4)
    ms, rounds = {}, []
    counts = {"pred": int(pred.shape[0]), "gt": int(gt.shape[0])}
    if counts["pred"] == 0 or counts["gt"] == 0:
        raise ValueError("evaluate_points: empty cloud (input)")

    def sync():
        if device == "gpu":
            import torch
            torch.cuda.synchronize()

    t0 = time.perf_counter()
    gt_c = _cropped(gt, crop, device, "ground truth")
    sync()
    ms["crop_gt"] = 1e3 * (time.perf_counter() - t0)
    counts["gt_cropped"] = int(gt_c.shape[0])
    if refine:
        t0 = time.perf_counter()
        for r, (spec, max_dist, max_iter) in enumerate(default_schedule(tau) if schedule is None else schedule):
            src = _down(_cropped(transform_points(pred, T, device), crop, device, f"prediction, ICP round {r + 1}"), spec, device)
            tgt = _down(gt_c, spec, device)
            upd, fit, rmse, its = icp(src, tgt, np.eye(4), max_dist, max_iter, device=device)
            T = upd @ T
            rounds.append({"source": int(src.shape[0]), "target": int(tgt.shape[0]), "max_dist": float(max_dist), "fitness": fit,
                           "rmse": rmse, "iterations": its})
        sync()
        ms["icp"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    pred_c = _cropped(transform_points(pred, T, device), crop, device, "prediction")
    counts["pred_cropped"] = int(pred_c.shape[0])
    pred_v, gt_v = voxel_mean(pred_c, voxel, device), voxel_mean(gt_c, voxel, device)
    sync()
    ms["crop_voxel"] = 1e3 * (time.perf_counter() - t0)
    counts.update(pred_voxel=int(pred_v.shape[0]), gt_voxel=int(gt_v.shape[0]))
    t0 = time.perf_counter()
    max_dist = 5 * max([tau] + taus)
    d1, _ = nearest(pred_v, gt_v, max_dist, device)
    d2, _ = nearest(gt_v, pred_v, max_dist, device)
    if device == "gpu":
        d1, d2 = d1.cpu().numpy(), d2.cpu().numpy()
    ms["nearest"] = 1e3 * (time.perf_counter() - t0)
    p, r, f = fscore(d1, d2, tau)
    extra = []
    for t in taus:
        pt, rt, ft = fscore(d1, d2, t)
        extra.append({"tau": t, "precision": pt, "recall": rt, "fscore": ft})
    return {"tau": float(tau), "precision": p, "recall": r, "fscore": f, "taus": extra,
            "curve_precision": cumulative_curve(d1, tau).tolist(), "curve_recall": cumulative_curve(d2, tau).tolist(),
            "transform": T.tolist(), "icp": rounds, "counts": counts, "ms": ms, "device": device}


def evaluate_scene(pred_file, gt_dir, scene, mode="pcd", tau=None, transform=None, voxel=None, device="cpu", **kw):
    """One scene in the T&T layout: <gt_dir>/<scene>/<scene>.ply, <scene>.json, <scene>_trans.txt.  mode "pcd": pred_file is a
    point cloud taken as it is; "mesh": a triangle mesh, sampled to points at thresh = voxel first.  tau defaults to the
    benchmark's value for the scene, voxel to tau / 2, transform to <scene>_trans.txt.  kw: refine, schedule, taus."""
    from .. import mesh_io
    from ..datasets import mvs_io
    _check_device(device)
    if mode not in ("mesh", "pcd"):
        raise ValueError(f"mode must be 'mesh' or 'pcd', got {mode!r}")
    if tau is None:
        if scene not in SCENE_TAU:
            raise ValueError(f"no default tau for the scene {scene!r} (known: {', '.join(sorted(SCENE_TAU))}): pass tau")
        tau = SCENE_TAU[scene]
    voxel = tau / 2 if voxel is None else voxel
    base = f"{gt_dir}/{scene}/{scene}"
    if mode == "pcd":
        pred = mvs_io.read_ply_points(pred_file)
    else:
        vertices, triangles = mesh_io.read_ply(pred_file)
        pred = (sample_mesh_points_gpu if device == "gpu" else sample_mesh_points)(vertices, triangles, voxel)
    if transform is None:
        transform = np.loadtxt(base + "_trans.txt", dtype=np.float64).reshape(4, 4)
    out = evaluate_points(pred, mvs_io.read_ply_points(base + ".ply"), tau, transform=transform, crop=read_crop_volume(base + ".json"),
                          voxel=voxel, device=device, **kw)
    out.update(scene=scene, mode=mode)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Tanks and Temples precision / recall / F-score of one reconstruction")
    ap.add_argument("--pred", required=True, help="the reconstruction: a PLY point cloud, or a triangle mesh with --mode mesh")
    ap.add_argument("--gt_dir", required=True, help="<gt_dir>/<scene>/<scene>.ply, <scene>.json, <scene>_trans.txt")
    ap.add_argument("--scene", required=True)
    ap.add_argument("--mode", default="pcd", choices=["pcd", "mesh"])
    ap.add_argument("--tau", type=float, default=None, help="distance threshold (default: the benchmark's value for the scene)")
    ap.add_argument("--taus", type=float, nargs="*", default=[], help="extra tolerances scored from the same distances (ETH3D's table)")
    ap.add_argument("--no_refine", action="store_true", help="use the 4x4 as it is: no ICP")
    ap.add_argument("--device", default="cpu", choices=["cpu", "gpu"],
                    help="gpu: crop, down-sample, align and measure with the HIP kernels (the same numbers as the numpy / scikit-learn path)")
    args = ap.parse_args(argv)
    rec = evaluate_scene(args.pred, args.gt_dir, args.scene, mode=args.mode, tau=args.tau, device=args.device,
                         refine=not args.no_refine, taus=args.taus)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
