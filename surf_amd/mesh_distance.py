"""Mesh deviation: the exact distance from a point to a triangle mesh, and from it how far one mesh lies from another - what
smoothing (surf_amd/mesh_smooth.py) and simplification (surf_amd/mesh_simplify.py) cost in geometry.

point_to_mesh gives, per query point, the least point-to-triangle distance over ALL faces, the smallest face index that attains
it and the closest point on that face.  mesh_deviation queries the vertices of each mesh against the other (Metro-style: Cignoni,
Rocchini, Scopigno 1998) and reports count, beyond, max, mean and rms per direction and the Hausdorff estimate, the larger of the
two max.  Only VERTICES are sampled, so that estimate is a LOWER bound of the true Hausdorff distance between the surfaces: a
coarse mesh can leave the fine one farthest in the middle of a large face.  Not attempted: signed distances, samples inside
faces or on edges, normals.

THE RULE is written once, in include/surf_hip.h above the surf_meshdist_* entry points.  backend="host" (the default) is its
numpy mirror below: fp64 on fp32 coordinates, one operation per operator in the header's order, the same kind of cell table walked
shell by shell over the queries still open.  backend="device" runs csrc/mesh_distance.hip through surf_amd.ops.point_to_mesh and
returns the same arrays; it has no host fall-back.  point_to_mesh_all_faces evaluates every (query, face) pair without any table:
the value is a minimum over all faces, so all three agree to the bit.

    python -m surf_amd.mesh_distance A.ply B.ply [--max_dist X] [--device gpu]

prints the deviation of two PLY meshes as one JSON line."""
import math
import time

import numpy as np
import torch

from .mesh_simplify import _as_device
from .mesh_smooth import sum256_host

_FAR_CELLS = 2.0 ** 40               # cell coordinates are kept within this many cells of the table (mesh_distance.hip, kFar)
_CHUNK = 1 << 20                     # (query, face) pairs the host path evaluates at once


def check_max_dist(max_dist):
    """max_dist as a float, or None for the default; ValueError unless it is finite and > 0."""
    if max_dist is None:
        return None
    try:
        value = float(max_dist)
    except (TypeError, ValueError):
        value = float("nan")
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"point_to_mesh: max_dist must be finite and > 0, got {max_dist!r} (None: the joint box's diagonal)")
    return value


def diagonal(lo, hi):
    """The default max_dist: the diagonal of the box [lo, hi] (three Python floats each), or 1.0 for a box without extent."""
    d = [float(b) - float(a) for a, b in zip(lo, hi)]
    diag = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return diag if diag > 0.0 and math.isfinite(diag) else 1.0


def joint_diagonal(*clouds):
    """diagonal() of the joint bounding box of (n, 3) fp32 arrays; the empty ones do not count."""
    clouds = [np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]
    clouds = [c for c in clouds if len(c)]
    if not clouds:
        return 1.0
    lo = np.min([c.min(axis=0) for c in clouds], axis=0)
    hi = np.max([c.max(axis=0) for c in clouds], axis=0)
    return diagonal(lo.tolist(), hi.tolist())


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def pair_rule(p, a, b, c):
    """The pair value of the rule for N (point, face) pairs, all (N, 3) fp64: (q (N,), c* (N, 3), region (N,) int8).  Every
    region's quotient is formed for every pair and only the taken one is used: the others are not part of the value."""
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    with np.errstate(all="ignore"):
        vc, vb, va, e1, e2 = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 > d3),
                 (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
        region = np.select(tests, list(range(6)), 6).astype(np.int8)
        den = 1.0 / ((va + vb) + vc)
        candidates = [a, b, a + ab * (d1 / (d1 - d3))[:, None], c, a + ac * (d2 / (d2 - d6))[:, None],
                      b + (c - b) * (e1 / (e1 + e2))[:, None], (a + ab * (vb * den)[:, None]) + ac * (vc * den)[:, None]]
        cs = candidates[6]
        for r in range(6):
            cs = np.where((region == r)[:, None], candidates[r], cs)
        e = p - cs
        q = _dot(e, e)
    return q, cs, region


def _as_np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def _inputs(points, vertices, faces, what="point_to_mesh"):
    """(points (k, 3) fp32, vertices (n, 3) fp32, faces (m, 3)) as contiguous host arrays, checked as the rule asks."""
    as_np = _as_np
    p32 = np.ascontiguousarray(as_np(points), dtype=np.float32).reshape(-1, 3)
    v32 = np.ascontiguousarray(as_np(vertices), dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(as_np(faces)).reshape(-1, 3)
    n = len(v32)
    if len(faces) and (faces.min() < 0 or faces.max() >= n):
        raise ValueError(f"face indices span [{faces.min()}, {faces.max()}], the mesh has {n} vertices")
    for arr, name in ((v32, "vertex"), (p32, "point")):
        bad = np.flatnonzero(~np.isfinite(arr).all(axis=1))
        if len(bad):
            raise ValueError(f"{what}: {name} {bad[0]} is not finite: {arr[bad[0]].tolist()}")
    return p32, v32, faces


def _finish(best, face, closest, max_dist):
    """Per query: distance = sqrt(Q), and +inf / -1 / +inf where distance < max_dist does not hold."""
    distance = np.sqrt(best)
    near = distance < max_dist
    return (np.where(near, distance, np.inf), np.where(near, face, -1).astype(np.int64),
            np.where(near[:, None], closest, np.inf))


def _corners(v32, faces):
    v = v32.astype(np.float64)
    f = faces.astype(np.int64)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def point_to_mesh_all_faces(points, vertices, faces, max_dist=None, chunk=_CHUNK):
    """The rule by brute force: every query against every face, `chunk` pairs at a time.  The yardstick of the tests."""
    max_dist = check_max_dist(max_dist)
    p32, v32, faces = _inputs(points, vertices, faces)
    if max_dist is None:
        max_dist = joint_diagonal(p32, v32)
    k, m = len(p32), len(faces)
    best, face, closest = np.full(k, np.inf), np.full(k, -1, np.int64), np.full((k, 3), np.inf)
    if k and m:
        a, b, c = _corners(v32, faces)
        p = p32.astype(np.float64)
        step = max(1, chunk // m)
        for s in range(0, k, step):
            nq = len(p[s:s + step])
            q, cs, _ = pair_rule(np.repeat(p[s:s + step], m, axis=0), np.tile(a, (nq, 1)), np.tile(b, (nq, 1)), np.tile(c, (nq, 1)))
            q = np.where(np.isnan(q), np.inf, q).reshape(nq, m)          # a NaN pair is ignored
            j = np.argmin(q, axis=1)                                      # the first, hence the smallest, index of the minimum
            best[s:s + nq], face[s:s + nq] = q[np.arange(nq), j], j
            closest[s:s + nq] = cs.reshape(nq, m, 3)[np.arange(nq), j]
    return _finish(best, face, closest, max_dist)


class HostTable:
    """The cell table of the rule's search over a mesh: lo, cell, dims, cell_start (cells + 1) and the face of every (cell, face)
    pair in cell order.  cell: the cell size to use, not grown for the pair budget (tests)."""

    def __init__(self, v32, faces, cell=None):
        from . import ops
        f = faces.astype(np.int64)
        m = len(f)
        named = v32[f.reshape(-1)]
        lo, hi = named.min(axis=0).astype(np.float64), named.max(axis=0).astype(np.float64)
        ext = (hi - lo).tolist()
        corners = np.stack([v32[f[:, 0]], v32[f[:, 1]], v32[f[:, 2]]])
        mn, mx = corners.min(axis=0).astype(np.float64), corners.max(axis=0).astype(np.float64)
        c, dims = ops.meshdist_cell_dims(ext, m, start_cell=cell)
        while True:
            top = np.array(dims, np.float64) - 1.0
            c0 = np.minimum(np.maximum(np.floor((mn - lo) / c), 0.0), top).astype(np.int64)
            c1 = np.minimum(np.maximum(np.floor((mx - lo) / c), 0.0), top).astype(np.int64)
            span = c1 - c0 + 1
            per = span[:, 0] * span[:, 1] * span[:, 2]
            pairs = int(per.sum())
            if cell is not None or pairs <= ops.meshdist_pair_budget(m):
                break
            c, dims = ops.meshdist_cell_dims(ext, m, start_cell=1.25 * c)
        if pairs > 2 ** 31 - 1:
            raise ValueError(f"point_to_mesh: {pairs} (cell, face) pairs at the cell size {c}")
        pair_face = np.repeat(np.arange(m), per)
        i = np.arange(pairs) - np.repeat(np.cumsum(per) - per, per)
        sy, sz, first = np.repeat(span[:, 1], per), np.repeat(span[:, 2], per), np.repeat(c0, per, axis=0)
        x, y, z = first[:, 0] + i // (sy * sz), first[:, 1] + (i // sz) % sy, first[:, 2] + i % sz
        pair_cell = (x * dims[1] + y) * dims[2] + z
        ncell = dims[0] * dims[1] * dims[2]
        self.faces = pair_face[np.argsort(pair_cell, kind="stable")]
        self.cell_start = np.zeros(ncell + 1, np.int64)
        self.cell_start[1:] = np.cumsum(np.bincount(pair_cell, minlength=ncell))
        self.lo, self.cell, self.dims, self.pairs = lo, float(c), np.array(dims, np.int64), pairs
        self.listed = np.flatnonzero(self.cell_start[1:] > self.cell_start[:-1])          # the cells that list a face
        self.listed_xyz = np.stack([self.listed // (dims[1] * dims[2]), (self.listed // dims[2]) % dims[1], self.listed % dims[2]], axis=1)
        self.per_listed_cell = pairs / max(1, len(self.listed))


def _shell_offsets(k, lo, hi):
    """The cell offsets of Chebyshev length k whose axis a lies in [lo[a], hi[a]], (S, 3) int64."""
    if k == 0:
        return np.zeros((1, 3), np.int64) if all(lo[a] <= 0 <= hi[a] for a in range(3)) else np.zeros((0, 3), np.int64)
    full = [np.arange(max(-k, lo[a]), min(k, hi[a]) + 1) for a in range(3)]
    inner = [np.arange(max(-k + 1, lo[a]), min(k - 1, hi[a]) + 1) for a in range(3)]
    parts = []
    for s in (-k, k):                                  # the two x faces whole, the y faces without them, the z faces without both
        for axes in (([s], full[1], full[2]) if lo[0] <= s <= hi[0] else None,
                     (inner[0], [s], full[2]) if lo[1] <= s <= hi[1] else None,
                     (inner[0], inner[1], [s]) if lo[2] <= s <= hi[2] else None):
            if axes is not None:
                parts.append(np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3))
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros((0, 3), np.int64)


def _walk(p, table, corners, max_dist, stats=None):
    """The shell walk of the rule for queries p (k, 3) fp64 over a HostTable: (Q (k,), face (k,), c* (k, 3)).  Shell after shell
    over the queries still open: a query is closed once its best is STRICTLY within the visited reach, the reach is max_dist, or
    the shell took in the last cell of the table."""
    a, b, c = corners
    k = len(p)
    best, face = np.full(k, np.inf), np.full(k, np.iinfo(np.int64).max, np.int64)
    top = table.dims - 1
    f = np.floor((p - table.lo) / table.cell)
    away = np.where(f < 0, -f, f - top)
    kmaxd = math.ceil(max_dist / (table.cell * (1.0 - 1e-6))) + 1.0
    open_ = (away <= kmaxd).all(axis=1)                # the others are far outside: nothing within max_dist
    cq = np.clip(f, -_FAR_CELLS, _FAR_CELLS).astype(np.int64)
    nxt = np.where(cq < 0, -cq, np.maximum(cq - top, 0)).max(axis=1)       # the first shell that touches the table
    last = np.minimum(np.maximum(cq, top - cq).max(axis=1), int(min(kmaxd, 4.0 * _FAR_CELLS)))
    evaluated = 0
    while open_.any():
        shell = int(nxt[open_].min())
        idx = np.flatnonzero(open_ & (nxt == shell))
        reach = float(shell - 1 if shell > 0 else 0) * table.cell * (1.0 - 1e-6)
        done = (best[idx] < reach * reach) | (reach >= max_dist) | (shell > last[idx])
        open_[idx[done]] = False
        idx = idx[~done]
        nxt[idx] += 1
        if not len(idx):
            continue
        # the shell's cells per query: by the shell's offsets, or, where those outnumber the cells that list a face (a query far
        # outside the table), by the Chebyshev distance from the query's cell to each of those
        lo_off, hi_off = (-cq[idx]).min(axis=0), (top - cq[idx]).max(axis=0)
        box = [max(0, int(min(shell, hi_off[a]) - max(-shell, lo_off[a])) + 1) for a in range(3)]
        by_listed = box[0] * box[1] * box[2] > 4 * len(table.listed)
        off = table.listed_xyz if by_listed else _shell_offsets(shell, lo_off, hi_off)
        if not len(off):
            continue
        step = max(1, int(_CHUNK // (len(off) * max(1.0, table.per_listed_cell))))
        for s in range(0, len(idx), step):
            part = idx[s:s + step]
            if by_listed:
                qi, si = np.nonzero(np.abs(off[None, :, :] - cq[part][:, None, :]).max(axis=2) == shell)
                cid = table.listed[si]
            else:
                cells = cq[part][:, None, :] + off[None, :, :]
                qi, si = np.nonzero(((cells >= 0) & (cells <= top)).all(axis=2))
                cid = (cells[qi, si, 0] * table.dims[1] + cells[qi, si, 1]) * table.dims[2] + cells[qi, si, 2]
            begin = table.cell_start[cid]
            count = table.cell_start[cid + 1] - begin
            total = int(count.sum())
            if total == 0:
                continue
            evaluated += total
            pq = np.repeat(part[qi], count)
            slot = np.repeat(begin, count) + (np.arange(total) - np.repeat(np.cumsum(count) - count, count))
            pf = table.faces[slot]
            q = pair_rule(p[pq], a[pf], b[pf], c[pf])[0]
            keep = ~np.isnan(q)                                            # a NaN pair is ignored
            pq, pf, q = pq[keep], pf[keep], q[keep]
            order = np.lexsort((pf, q, pq))                                # per query: the least q, then the smallest face
            pq, pf, q = pq[order], pf[order], q[order]
            head = np.ones(len(pq), bool)
            head[1:] = pq[1:] != pq[:-1]
            pq, pf, q = pq[head], pf[head], q[head]
            better = (q < best[pq]) | ((q == best[pq]) & (pf < face[pq]))
            best[pq[better]], face[pq[better]] = q[better], pf[better]
    closest = np.full((k, 3), np.inf)
    hit = np.flatnonzero(np.isfinite(best))
    if len(hit):
        closest[hit] = pair_rule(p[hit], a[face[hit]], b[face[hit]], c[face[hit]])[1]
    if stats is not None:
        stats.update(cell=table.cell, dims=table.dims.tolist(), pairs=table.pairs, evaluated=evaluated, max_dist=max_dist)
    return best, face, closest


def point_to_mesh_host(points, vertices, faces, max_dist=None, _cell=None, stats=None):
    """The rule in numpy through the cell table: (distance (k,) fp64, face (k,) int64, closest (k, 3) fp64).  _cell: the cell size
    to use (tests); stats: a dict that receives cell, dims, pairs, evaluated (pairs evaluated by the walk) and max_dist."""
    max_dist = check_max_dist(max_dist)
    p32, v32, faces = _inputs(points, vertices, faces)
    if max_dist is None:
        max_dist = joint_diagonal(p32, v32)
    k, m = len(p32), len(faces)
    if k == 0 or m == 0:
        return np.full(k, np.inf), np.full(k, -1, np.int64), np.full((k, 3), np.inf)
    best, face, closest = _walk(p32.astype(np.float64), HostTable(v32, faces, _cell), _corners(v32, faces), max_dist, stats)
    return _finish(best, face, closest, max_dist)


@torch.no_grad()
def point_to_mesh(points, vertices, faces, max_dist=None, backend="host", device="cuda", return_tensors=False, _cell=None):
    """The exact distance from every point to a triangle mesh.

    points (k, 3) and vertices (n, 3) (used as fp32, all finite), faces (m, 3) integers; numpy arrays or tensors.  Returns
    (distance (k,) fp64, face (k,) int64, closest (k, 3) fp64): the least point-to-triangle distance over all faces, the smallest
    face index that attains it and the closest point on that face; +inf, -1 and (+inf, +inf, +inf) where the distance is not
    below max_dist (default: the diagonal of the joint bounding box of points and vertices) or the mesh has no face.
    backend="device": the same arrays from the GPU (`device`), without a host fall-back; return_tensors=True (device backend only)
    takes and returns device tensors, with no host copy and surf_amd.ops.MESHDIST_HOST_READS reads of the device (one more for
    every growth of the table's cell).
    Unsigned distances from the points given: nothing is sampled on the faces of either side.  _cell: the table's cell (tests)."""
    if backend == "device":
        from . import ops
        if torch.device(device).type == "cpu" or not torch.cuda.is_available():
            raise RuntimeError('point_to_mesh(backend="device") needs a GPU: there is no host fall-back for the device path')
        out = ops.point_to_mesh(_as_device(points, torch.float32, device).reshape(-1, 3),
                                _as_device(vertices, torch.float32, device).reshape(-1, 3),
                                _as_device(faces, torch.int32, device).reshape(-1, 3), max_dist, cell=_cell)
        return out if return_tensors else tuple(t.cpu().numpy() for t in out)
    if backend != "host":
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    if return_tensors:
        raise ValueError('return_tensors=True needs backend="device"')
    return point_to_mesh_host(points, vertices, faces, max_dist, _cell=_cell)


def _stats(count, found, largest, s1, s2):
    found = int(found)
    some = found > 0
    return {"count": int(count), "beyond": int(count) - found, "max": float(largest) if some else None,
            "mean": s1 / float(found) if some else None, "rms": math.sqrt(s2 / float(found)) if some else None}


def direction_stats(distance):
    """count, beyond, max, mean and rms of one direction from its distances (fp64, +inf = beyond), as the rule sums them."""
    distance = np.asarray(distance, np.float64)
    found = np.isfinite(distance)
    if not found.any():
        return _stats(len(distance), 0, 0.0, 0.0, 0.0)
    d = np.where(found, distance, 0.0)
    return _stats(len(distance), found.sum(), distance[found].max(), sum256_host(d), sum256_host(d * d))


@torch.no_grad()
def mesh_deviation(vertices_a, faces_a, vertices_b, faces_b, max_dist=None, backend="host", device="cuda", _cell=None):
    """The two-sided vertex-sampled deviation between the meshes A and B:

        {"forward": {count, beyond, max, mean, rms}, "backward": {...}, "hausdorff": max of the two max}

    forward queries the vertices of A that a face of A names against B, backward those of B against A; beyond counts the queries
    without a face of the other mesh nearer than max_dist (default: the diagonal of the joint bounding box of all vertices, so
    that nothing is beyond); max, mean and rms are over the others and None when there are none, and hausdorff is None if either
    max is.  Vertex sampling makes `hausdorff` a LOWER bound of the true Hausdorff distance; signed distances and samples on
    the faces are not attempted.  backend="device": the same dict from the GPU, without a host fall-back."""
    if backend not in ("host", "device"):
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    max_dist = check_max_dist(max_dist)
    _, va, fa = _inputs(np.zeros((0, 3), np.float32), vertices_a, faces_a, "mesh_deviation")
    _, vb, fb = _inputs(np.zeros((0, 3), np.float32), vertices_b, faces_b, "mesh_deviation")
    if max_dist is None:
        max_dist = joint_diagonal(va, vb)
    out = {}
    for name, (qv, qf), (mv, mf) in (("forward", (va, fa), (vb, fb)), ("backward", (vb, fb), (va, fa))):
        queries = qv[np.unique(qf)]                                        # the vertices a face names, in index order
        if backend == "device":
            from . import ops
            dist = point_to_mesh(queries, mv, mf, max_dist, backend="device", device=device, return_tensors=True, _cell=_cell)[0]
            out[name] = _stats(len(queries), *ops.meshdist_stats(dist)) if len(queries) else _stats(0, 0, 0.0, 0.0, 0.0)
        else:
            out[name] = direction_stats(point_to_mesh_host(queries, mv, mf, max_dist, _cell=_cell)[0])
    both = [out["forward"]["max"], out["backward"]["max"]]
    out["hausdorff"] = None if None in both else max(both)
    return out


def deviation_step(vertices_a, faces_a, vertices_b, faces_b, max_dist=None, backend="host", device="cuda"):
    """The scripts' deviation step: mesh_deviation of the mesh before (A) and after (B) smoothing and simplification -> the
    `deviation` block of their JSON lines, {forward, backward, hausdorff, max_dist, ms}."""
    max_dist = check_max_dist(max_dist)
    if max_dist is None:
        max_dist = joint_diagonal(_as_np(vertices_a), _as_np(vertices_b))
    t0 = time.perf_counter()
    rec = mesh_deviation(vertices_a, faces_a, vertices_b, faces_b, max_dist, backend=backend, device=device)
    return {**rec, "max_dist": max_dist, "ms": 1e3 * (time.perf_counter() - t0)}


def main(argv=None):
    import argparse
    import json
    from . import mesh_io
    ap = argparse.ArgumentParser(description="The vertex-sampled deviation between two PLY triangle meshes, as one JSON line.")
    ap.add_argument("mesh_a")
    ap.add_argument("mesh_b")
    ap.add_argument("--max_dist", type=float, default=None, help="queries without a face nearer than this count as `beyond` "
                                                                 "(default: the diagonal of the joint bounding box)")
    ap.add_argument("--device", default="cpu", choices=["cpu", "gpu"], help="gpu: csrc/mesh_distance.hip, the same numbers")
    args = ap.parse_args(argv)
    (va, fa), (vb, fb) = mesh_io.read_ply(args.mesh_a), mesh_io.read_ply(args.mesh_b)
    try:
        rec = deviation_step(va, fa, vb, fb, args.max_dist, backend="device" if args.device == "gpu" else "host")
    except ValueError as e:
        raise SystemExit(f"mesh_distance: {e}")
    rec = {"mesh_a": args.mesh_a, "mesh_b": args.mesh_b, "vertices": [len(va), len(vb)], "faces": [len(fa), len(fb)], **rec}
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
