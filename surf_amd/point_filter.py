"""Clean-up of a fused point cloud (fusion.fuse_points): outlier removal on the cloud itself and normals, both from ONE primitive,
the k nearest neighbours of every point of the cloud within the cloud.

    cloud = fusion.fuse_points(views, 2)
    cloud, kept = remove_outliers(cloud, k=16, std_ratio=2.0, max_dist=10 * voxel)           # or method="radius"
    normals = estimate_normals(cloud, camera_centres(views), k=16, max_dist=10 * voxel)
    mesh_io.write_ply_points(path, cloud.points, cloud.colors, normals=normals)

THE RULE (rules 1-5: neighbours, statistic, statistical rule, radius rule, normals) is written once, in include/surf_hip.h above
the surf_points_knn* entry points.  backend="device" runs csrc/point_knn.hip through surf_amd.ops (a dense cell table, one thread
per query, the k-slot list in LDS) and has no host fall-back.  backend="host" is the numpy mirror below and returns equal arrays:
it takes its CANDIDATES from scipy's cKDTree in float64 (the k + 1 nearest give a radius; every point within that radius times
1 + 1e-5 - fp32 squared distances are good to 3e-7 relative - is a candidate), then recomputes d2 in fp32 by the rule, orders by
(d2, j) and keeps the first k; the sums, the covariance and the Jacobi sweeps repeat the kernel's operations one by one.
The one exception is the statistical rule's threshold: its three sums are added in the device's own fixed order there and by np.sum
here, so mu, sd and the threshold may differ in their last bits, and a mask differs only where a statistic lies within ~1e-15
relative of the threshold.

How this relates to the libraries that do the same jobs (from recollection, NOT pinned against either: neither is a dependency):
Open3D's remove_statistical_outlier(nb_neighbors, std_ratio) queries nb_neighbors points INCLUDING the query itself at distance 0
and averages over all of them, so it is believed to correspond to k = nb_neighbors - 1 with the mean rescaled by k / (k + 1) (the
threshold rule is invariant under that scaling); it has no max_dist, so no point is starved there.  PCL's StatisticalOutlierRemoval
uses the sample standard deviation; this rule uses the population's.  remove_radius_outlier(nb_points, radius) keeps a point with
at least nb_points neighbours inside the radius (whether the point itself counts there is likewise unpinned): method="radius" with
k = min_neighbours excludes the point itself and includes the boundary, d2 <= md2.

max_dist is in world units and required: it bounds the search (an isolated outlier costs a bounded walk) and makes a point with
fewer than k neighbours within it STARVED - its statistic is +inf, the statistical rule drops it, its count says why.
"""
import time

import numpy as np
import torch

from .fusion import PointCloud, _split_P

KNN_MAX_K = 32                       # SURF_POINTS_KNN_MAX_K
NORMAL_SWEEPS = 8                    # SURF_POINTS_NORMAL_SWEEPS
_CANDIDATE_MARGIN = 1.0 + 1e-5


def _check(k, max_dist, what):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"{what}: k must be an integer in [1, {KNN_MAX_K}], got {k}")
    if max_dist is None:
        raise ValueError(f"{what}: max_dist (world units) is required")
    md = np.float32(max_dist)
    with np.errstate(all="ignore"):
        md2 = md * md
    if not (md > 0 and np.isfinite(md) and md2 > 0 and np.isfinite(md2)):
        raise ValueError(f"{what}: max_dist must be finite and > 0 (and so must its fp32 square), got {max_dist}")
    return int(k), md, md2


def _points(points):
    p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    p = np.ascontiguousarray(p, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points: expected (n, 3), got {p.shape}")
    if len(p) > 2 ** 31 - 1:
        raise ValueError(f"points: {len(p)} points exceed int32 indexing")
    return p


def _device(backend, device, what):
    if backend not in ("device", "host"):
        raise ValueError(f"{what}: backend {backend!r} (device or host)")
    if backend == "host":
        return None
    if not torch.cuda.is_available() or (device is not None and torch.device(device).type == "cpu"):
        raise RuntimeError(f"{what}(backend='device') needs a GPU (the SuRF hot path has no CPU fallback)")
    return torch.device("cuda" if device is None else device)


# ---- the host mirror ----

def knn_host(points, k, max_dist, workers=1):
    """Rule 1 in numpy: (index (n, k) int32 padded with -1, d2 (n, k) fp32 padded with +inf, count (n,) int32)."""
    from scipy.spatial import cKDTree
    k, md, md2 = _check(k, max_dist, "knn")
    P = _points(points)
    n = len(P)
    index = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf, np.float32)
    count = np.zeros(n, np.int32)
    fin = np.flatnonzero(np.isfinite(P).all(axis=1))
    if len(fin) < 2:
        return index, d2, count
    Q = P[fin].astype(np.float64)
    tree = cKDTree(Q)
    cap = float(md) * _CANDIDATE_MARGIN
    kk = min(k + 1, len(fin))                          # the query itself is among them
    dist = tree.query(Q, k=kk, workers=workers)[0].reshape(len(fin), kk)
    # the k-th other point's float64 distance bounds every fp32-rule neighbour (up to the margin); fewer than k + 1 points: the cap
    radius = np.minimum(dist[:, -1] * _CANDIDATE_MARGIN, cap) if kk == k + 1 else np.full(len(fin), cap)
    radius = np.where(np.isfinite(radius), radius, cap)
    balls = tree.query_ball_point(Q, radius, workers=workers)
    lens = np.fromiter((len(b) for b in balls), np.int64, len(fin))
    row = np.repeat(np.arange(len(fin)), lens)
    col = np.fromiter((j for b in balls for j in b), np.int64, int(lens.sum()))
    keep = row != col                                  # only the index itself is excluded
    row, col = row[keep], col[keep]
    a, b = P[fin[col]], P[fin[row]]
    dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
    dd = (dx * dx + dy * dy) + dz * dz                 # fp32, one operation per operator
    keep = dd <= md2
    row, col, dd = row[keep], fin[col[keep]], dd[keep]
    order = np.lexsort((col, dd, row))                 # by query, then (d2, j)
    row, col, dd = row[order], col[order], dd[order]
    first = np.searchsorted(row, np.arange(len(fin)))
    rank = np.arange(len(row)) - first[row]
    keep = rank < k
    row, col, dd, rank = row[keep], col[keep], dd[keep], rank[keep]
    index[fin[row], rank] = col
    d2[fin[row], rank] = dd
    count[fin] = np.minimum(np.bincount(row, minlength=len(fin)), k)
    return index, d2, count


def stat_host(d2, count):
    """Rule 2 from the lists: stat (n,) fp32."""
    n, k = d2.shape
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2.astype(np.float32))
        s = np.zeros(n, np.float32)
        for m in range(k):
            s = s + dist[:, m]
        return np.where(count == k, s / np.float32(k), np.float32(np.inf)).astype(np.float32)


def threshold_host(stat, std_ratio):
    """Rule 3: (mu, sd, thr, number of finite statistics); thr is -inf when none is finite (nothing is kept)."""
    x = stat[np.isfinite(stat)].astype(np.float64)
    return _threshold(float(len(x)), float(np.sum(x)), float(np.sum(x * x)), std_ratio)


def _threshold(N, S, Q, std_ratio):
    if N == 0:
        return float("nan"), float("nan"), float("-inf"), 0
    mu = S / N
    sd = float(np.sqrt(max(Q / N - mu * mu, 0.0)))
    return mu, sd, mu + float(std_ratio) * sd, int(N)


def _rotate(A, V, p, q, r):
    """One Jacobi rotation of rule 5 on the rows where A[pq] != 0.  A: dict of (n,) arrays keyed by sorted index pairs; V: (3, 3)
    list of (n,) arrays."""
    key = lambda i, j: (min(i, j), max(i, j))
    app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[key(p, q)], A[key(r, p)], A[key(r, q)]
    on = apq != 0.0
    safe = np.where(on, apq, 1.0)
    theta = (aqq - app) / (2.0 * safe)
    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(theta < 0.0, -t, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[(p, p)] = np.where(on, app - h, app)
    A[(q, q)] = np.where(on, aqq + h, aqq)
    A[key(p, q)] = np.where(on, 0.0, apq)
    A[key(r, p)] = np.where(on, c * arp - s * arq, arp)
    A[key(r, q)] = np.where(on, s * arp + c * arq, arq)
    for i in range(3):
        vp, vq = V[i][p], V[i][q]
        V[i][p] = np.where(on, c * vp - s * vq, vp)
        V[i][q] = np.where(on, s * vp + c * vq, vq)


def normals_host(points, index, count, view=None, centres=None):
    """Rule 5 from the lists: (n, 3) fp32.  view (n,) integers and centres (n_views, 3) float64 orient the normals."""
    P = _points(points)
    n, k = index.shape
    out = np.zeros((n, 3), np.float32)
    rows = np.flatnonzero(count >= 2)
    if not len(rows):
        return out
    idx, cnt, p = index[rows], count[rows], P[rows]
    with np.errstate(all="ignore"):
        S1 = [np.zeros(len(rows)) for _ in range(3)]
        S2 = {(a, b): np.zeros(len(rows)) for a in range(3) for b in range(a, 3)}
        for m in range(k):
            on = m < cnt
            e = (P[np.where(on, idx[:, m], 0)] - p).astype(np.float64)          # the fp32 difference, then widened
            for a in range(3):
                S1[a] = np.where(on, S1[a] + e[:, a], S1[a])
                for b in range(a, 3):
                    S2[(a, b)] = np.where(on, S2[(a, b)] + e[:, a] * e[:, b], S2[(a, b)])
        mm = (cnt + 1).astype(np.float64)
        M = [S1[a] / mm for a in range(3)]
        A = {(a, b): S2[(a, b)] / mm - M[a] * M[b] for a in range(3) for b in range(a, 3)}
        one, zero = np.ones(len(rows)), np.zeros(len(rows))
        V = [[one if i == j else zero for j in range(3)] for i in range(3)]
        for _ in range(NORMAL_SWEEPS):
            _rotate(A, V, 0, 1, 2)
            _rotate(A, V, 0, 2, 1)
            _rotate(A, V, 1, 2, 0)
        g1 = A[(1, 1)] < A[(0, 0)]
        g2 = A[(2, 2)] < np.where(g1, A[(1, 1)], A[(0, 0)])
        x, y, z = (np.where(g2, V[i][2], np.where(g1, V[i][1], V[i][0])) for i in range(3))
        ln = np.sqrt((x * x + y * y) + z * z)
        x, y, z = x / ln, y / ln, z / ln
        d = np.zeros(len(rows))
        if centres is not None:
            centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
            v = np.asarray(view)[rows].astype(np.int64)
            ok = (v >= 0) & (v < len(centres))
            c = centres[np.where(ok, v, 0)]
            pd = p.astype(np.float64)
            d = np.where(ok, (x * (c[:, 0] - pd[:, 0]) + y * (c[:, 1] - pd[:, 1])) + z * (c[:, 2] - pd[:, 2]), 0.0)
        big = x
        big = np.where(np.abs(y) > np.abs(big), y, big)
        big = np.where(np.abs(z) > np.abs(big), z, big)
        flip = np.where(d == 0.0, big < 0.0, d < 0.0)
        x, y, z = (np.where(flip, -c, c) for c in (x, y, z))
        good = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~np.isnan(d)
        out[rows] = np.where(good[:, None], np.stack([x, y, z], axis=1), 0.0).astype(np.float32)
    return out


# ---- the public surface ----

def _to_dev(points, dev):
    t = points if torch.is_tensor(points) else torch.from_numpy(_points(points))
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"points: expected (n, 3), got {tuple(t.shape)}")
    return t


@torch.no_grad()
def knn(points, k, max_dist, backend="device", device=None, cell=None):
    """The k nearest neighbours of every point of `points` (n, 3) (used as fp32) within the cloud, by rule 1: (index (n, k) int32
    padded with -1, d2 (n, k) fp32 squared distances padded with +inf, count (n,) int32), numpy arrays.  Neighbours lie within
    max_dist (d2 <= fp32(max_dist)^2), in ascending (d2, index) order; a point is not its own neighbour, its duplicates are.
    cell (tests only) overrides the device path's cell size; the result does not depend on it."""
    k, md, _ = _check(k, max_dist, "knn")
    dev = _device(backend, device, "knn")
    if dev is None:
        return knn_host(points, k, md)
    from . import ops
    return tuple(t.cpu().numpy() for t in ops.points_knn(_to_dev(points, dev), k, float(md), cell=cell))


@torch.no_grad()
def outlier_stats(points, k, max_dist, backend="device", device=None, cell=None):
    """(stat (n,) fp32, count (n,) int32) by rule 2: the mean distance to the k nearest neighbours within max_dist, +inf for a
    starved point (count < k).  The device path never forms the lists."""
    k, md, _ = _check(k, max_dist, "outlier_stats")
    dev = _device(backend, device, "outlier_stats")
    if dev is None:
        _, d2, count = knn_host(points, k, md)
        return stat_host(d2, count), count
    from . import ops
    stat, count, _ = ops.points_knn_reduce(_to_dev(points, dev), k, float(md), cell=cell)
    return stat.cpu().numpy(), count.cpu().numpy()


@torch.no_grad()
def remove_outliers(cloud, k=16, std_ratio=2.0, max_dist=None, method="statistical", backend="device", device=None, stats=None):
    """(PointCloud, kept_index): the cloud without its outliers; kept_index (ascending int64) filters points, colors and origin.
    method="statistical" (rule 3): a point stays iff its statistic is <= mu + std_ratio * sd over the finite statistics; starved
    points (fewer than k neighbours within max_dist) go.  method="radius" (rule 4): a point stays iff it has k neighbours within
    max_dist (k = min_neighbours, max_dist = radius; std_ratio is not read).  max_dist is required, in world units.
    stats (dict, optional): receives points_in, points_out, starved, mu, sd, threshold (None for "radius")."""
    if method not in ("statistical", "radius"):
        raise ValueError(f"remove_outliers: method {method!r} (statistical or radius)")
    k, md, _ = _check(k, max_dist, "remove_outliers")
    if method == "statistical" and not np.isfinite(float(std_ratio)):
        raise ValueError(f"remove_outliers: std_ratio must be finite, got {std_ratio}")
    dev = _device(backend, device, "remove_outliers")
    cloud = cloud if isinstance(cloud, PointCloud) else PointCloud(*cloud)
    n = len(cloud.points)
    mu = sd = thr = None
    if dev is None:
        _, d2, count = knn_host(cloud.points, k, md)
        if method == "statistical":
            stat = stat_host(d2, count)
            mu, sd, thr, _ = threshold_host(stat, std_ratio)
            keep = stat.astype(np.float64) <= thr
        else:
            keep = count == k
        starved = int((count < k).sum())
    else:
        from . import ops
        stat, count, _ = ops.points_knn_reduce(_to_dev(cloud.points, dev), k, float(md))
        if method == "statistical":
            N, S, Q = (ops.points_stat_sums(stat).tolist() if n else (0.0, 0.0, 0.0))
            mu, sd, thr, _ = _threshold(N, S, Q, std_ratio)
            keep = (stat.double() <= thr).cpu().numpy()
        else:
            keep = (count == k).cpu().numpy()
        starved = int((count < k).sum())
    kept = np.flatnonzero(keep).astype(np.int64)
    out = PointCloud(np.ascontiguousarray(np.asarray(cloud.points)[kept]),
                     None if cloud.colors is None else np.ascontiguousarray(np.asarray(cloud.colors)[kept]),
                     None if cloud.origin is None else np.ascontiguousarray(np.asarray(cloud.origin)[kept]))
    if stats is not None:
        stats.update(points_in=n, points_out=int(len(kept)), starved=starved, mu=mu, sd=sd, threshold=thr)
    return out, kept


@torch.no_grad()
def estimate_normals(cloud, centres=None, k=16, max_dist=None, backend="device", device=None):
    """(n, 3) fp32 unit normals by rule 5: the direction of least variance of a point and its k nearest neighbours within max_dist,
    (0, 0, 0) where a point has fewer than two.  centres (n_views, 3) float64 (camera_centres(views)): a normal is turned towards
    the camera that saw its point (cloud.origin[:, 0] names the view); None: its largest component is made positive.
    cloud: a PointCloud, or (n, 3) points when centres is None."""
    k, md, _ = _check(k, max_dist, "estimate_normals")
    dev = _device(backend, device, "estimate_normals")
    if isinstance(cloud, PointCloud):
        points, origin = cloud.points, cloud.origin
    else:
        points, origin = cloud, None
    view = None
    if centres is not None:
        if origin is None:
            raise ValueError("estimate_normals: centres need a PointCloud with its origin")
        centres = np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(-1, 3))
        view = np.ascontiguousarray(np.asarray(origin)[:, 0], dtype=np.int32)
        if len(view) != len(points):
            raise ValueError("estimate_normals: origin has one row per point")
        if len(view) and (view.min() < 0 or view.max() >= len(centres)):
            raise ValueError(f"estimate_normals: origin names views {view.min()}..{view.max()}, centres has {len(centres)}")
        if not len(centres):
            raise ValueError("estimate_normals: centres is empty")
    if dev is None:
        index, _, count = knn_host(points, k, md)
        return normals_host(points, index, count, view, centres)
    from . import ops
    normal = ops.points_knn_reduce(_to_dev(points, dev), k, float(md), normals=True,
                                   view=None if view is None else torch.from_numpy(view).to(dev),
                                   centres=None if centres is None else torch.from_numpy(centres).to(dev))[2]
    return normal.cpu().numpy()


def camera_centres(views):
    """(n_views, 3) float64: the centre -M^-1 t of every DepthView's P = [M | t], as fusion.lift_transform forms it."""
    out = np.zeros((len(views), 3), np.float64)
    for i, v in enumerate(views):
        _, t, M_inv = _split_P(v)
        out[i] = -(M_inv @ t)
    return out


def clean_step(cloud, views, outliers=None, radius_outliers=None, normals_k=None, max_dist=None, backend="device", device=None):
    """scripts/fuse_scene.py's cloud steps, outliers first and normals on what is left: (cloud, normals or None, records) with
    records = {"cloud_filter": {method, k, std_ratio, max_dist, points_in, points_out, starved, threshold, ms}, "cloud_normals":
    {k, zero, ms}}, each present when its step ran.  outliers: (k, std_ratio); radius_outliers: min_neighbours."""
    records, normals = {}, None
    if outliers is not None and radius_outliers is not None:
        raise ValueError("clean_step: one of outliers and radius_outliers")
    if outliers is not None or radius_outliers is not None:
        method = "statistical" if outliers is not None else "radius"
        k, ratio = (int(outliers[0]), float(outliers[1])) if outliers is not None else (int(radius_outliers), None)
        st = {}
        t0 = time.perf_counter()
        cloud, _ = remove_outliers(cloud, k=k, std_ratio=2.0 if ratio is None else ratio, max_dist=max_dist, method=method,
                                   backend=backend, device=device, stats=st)
        records["cloud_filter"] = {"method": method, "k": k, "std_ratio": ratio, "max_dist": float(max_dist),
                                   "points_in": st["points_in"], "points_out": st["points_out"], "starved": st["starved"],
                                   "threshold": st["threshold"] if st["threshold"] is not None and np.isfinite(st["threshold"]) else None,
                                   "ms": 1e3 * (time.perf_counter() - t0)}       # no finite statistic: no threshold (JSON has no -inf)
    if normals_k is not None:
        t0 = time.perf_counter()
        normals = estimate_normals(cloud, camera_centres(views), k=int(normals_k), max_dist=max_dist, backend=backend, device=device)
        records["cloud_normals"] = {"k": int(normals_k), "zero": int((~normals.any(axis=1)).sum()),
                                    "ms": 1e3 * (time.perf_counter() - t0)}
    return cloud, normals, records
