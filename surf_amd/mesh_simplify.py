"""Mesh simplification: vertex clustering on a lattice anchored at the world origin, one output vertex per cell placed by the
cell's error quadric (Lindstrom 2000; Garland-Heckbert quadrics), so that edges and corners stay where they are.

THE RULE (rules 1-8) is written once, in include/surf_hip.h above the surf_simplify_* entry points.  backend="host" (the
default) is its numpy mirror below: fp64, one operation per operator in the header's order, per-cell sums by np.add.at, which
adds its terms one after the other in the order given - (face, corner) order for the face terms, vertex-index order for the
vertex terms - and the 3x3 solve written out as the header's LDL^T sequence (no LAPACK call).  backend="device" runs
csrc/mesh_simplify.hip through surf_amd.ops.simplify_mesh and returns the same arrays; it has no host fall-back.

Not attempted: iterative edge collapse, manifold or boundary preservation, repair of faces whose orientation flips."""
import time

import numpy as np
import torch

HALF = 1 << 20                   # cell indices lie in [-2^20, 2^20)
LAMBDA = 2.0 ** -20              # weight of the cell mean in the solve, relative to the quadric's trace


def _check_cell(cell):
    cell = float(cell)
    if not (cell > 0 and 0 < cell * cell < float("inf")):
        raise ValueError(f"simplify_mesh: cell must be finite and > 0, got {cell}")
    return cell


def cell_indices(vertices, cell):
    """Rule 1: ((n, 3) int64 cell indices, (n,) int64 keys) of (n, 3) fp32 vertices; ValueError beyond the lattice."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        f = np.floor(v / cell)
    if not np.all((f >= -HALF) & (f < HALF)):                       # false for NaN and +-inf
        raise ValueError(f"simplify_mesh: a vertex is not finite or lies outside the 2^21 cells of {cell} per axis")
    i = f.astype(np.int64)
    return i, ((i[:, 0] + HALF) << 42) | ((i[:, 1] + HALF) << 21) | (i[:, 2] + HALF)


def _add_at(n_cells, index, terms):
    """(n_cells, k) sums of terms (len(index), k) by cell, each added one after the other in the order given, from +0."""
    out = np.zeros((terms.shape[1], n_cells), np.float64)
    for j in range(terms.shape[1]):
        np.add.at(out[j], index, np.ascontiguousarray(terms[:, j]))
    return out.T


def _ldl3(A, b, s, mean):
    """(A + s I) x = b + s mean by the header's LDL^T sequence; A (k, 6) = (A00, A01, A02, A11, A12, A22), b, mean (k, 3), s (k,)."""
    m00, m11, m22 = A[:, 0] + s, A[:, 3] + s, A[:, 5] + s
    r0, r1, r2 = b[:, 0] + s * mean[:, 0], b[:, 1] + s * mean[:, 1], b[:, 2] + s * mean[:, 2]
    l10, l20 = A[:, 1] / m00, A[:, 2] / m00
    d1 = m11 - l10 * A[:, 1]
    u21 = A[:, 4] - l20 * A[:, 1]
    l21 = u21 / d1
    d2 = (m22 - l20 * A[:, 2]) - l21 * u21
    y1 = r1 - l10 * r0
    y2 = (r2 - l20 * r0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (r0 / m00 - l10 * x1) - l20 * x2
    return np.stack([x0, x1, x2], axis=1)


def simplify_mesh_host(vertices, faces, cell, normals=None, colors=None, stages=None):
    """The rule in numpy: (vertices (k, 3) fp32, faces (j, 3) int32, normals (k, 3) fp32 or None, colors (k, 3) uint8 or None,
    vertex_map (n,) int32).  stages: a list that receives (name, ms) per stage (scripts/time_simplify.py)."""
    t_stage = [time.perf_counter()]

    def stage(name):
        if stages is not None:
            now = time.perf_counter()
            stages.append((name, 1e3 * (now - t_stage[0])))
            t_stage[0] = now

    cell = _check_cell(cell)
    v32 = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces).reshape(-1, 3)
    n, m = len(v32), len(faces)
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError(f"face indices span [{faces.min()}, {faces.max()}], the mesh has {n} vertices")
    faces = faces.astype(np.int64)
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if colors is not None:
        colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    for a, name in ((normals, "normals"), (colors, "colors")):
        if a is not None and len(a) != n:
            raise ValueError(f"simplify_mesh: {name} {a.shape} for {n} vertices")
    idx, key = cell_indices(v32, cell)                              # rule 1
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None if normals is None else np.zeros((0, 3), np.float32),
             None if colors is None else np.zeros((0, 3), np.uint8), np.full(n, -1, np.int32))
    if n == 0 or m == 0:
        return empty
    ukeys, vcell = np.unique(key, return_inverse=True)
    vcell = vcell.reshape(-1)
    n_cells = len(ukeys)
    stage("keys+sort")

    # rule 7: faces over cells
    fc = vcell[faces]
    sc = np.sort(fc, axis=1)
    distinct = (sc[:, 0] != sc[:, 1]) & (sc[:, 1] != sc[:, 2])
    cand = np.flatnonzero(distinct)
    s = sc[cand]
    order = np.lexsort((s[:, 2], s[:, 1], s[:, 0]))                  # stable: the lowest face index leads its group
    s = s[order]
    first = np.ones(len(s), bool)
    first[1:] = (s[1:] != s[:-1]).any(axis=1)
    keep = np.zeros(m, bool)
    keep[cand[order[first]]] = True
    # rule 8
    used = np.zeros(n_cells, bool)
    used[fc[keep].reshape(-1)] = True
    cscan = np.cumsum(used) - 1
    out_f = cscan[fc[keep]].astype(np.int32)
    vmap = np.where(used[vcell], cscan[vcell], -1).astype(np.int32)
    stage("faces")
    if not keep.any():
        return empty

    v = v32.astype(np.float64)
    centre = (idx.astype(np.float64) + 0.5) * cell                   # per vertex: the centre of its cell
    with np.errstate(all="ignore"):
        # rule 2
        p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        L = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ok = (L > 0) & np.isfinite(L) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
        fo = faces[ok]
        L, p0 = L[ok], p0[ok]
        nrm = np.stack([cx[ok] / L, cy[ok] / L, cz[ok] / L], axis=1)                           # (k, 3)
        w = (L / 2.0) / (cell * cell)
        q = (p0[:, None, :] - centre[fo]) / cell                                               # (k, corner, 3)
        d = (nrm[:, None, 0] * q[:, :, 0] + nrm[:, None, 1] * q[:, :, 1]) + nrm[:, None, 2] * q[:, :, 2]     # (k, corner)
        g = w[:, None] * nrm
        wd = w[:, None] * d
        A_face = np.stack([g[:, 0] * nrm[:, 0], g[:, 0] * nrm[:, 1], g[:, 0] * nrm[:, 2], g[:, 1] * nrm[:, 1], g[:, 1] * nrm[:, 2],
                           g[:, 2] * nrm[:, 2]], axis=1)                                       # (k, 6), the same for each corner
        terms = np.concatenate([np.broadcast_to(A_face[:, None, :], (len(fo), 3, 6)), wd[:, :, None] * nrm[:, None, :]], axis=2)
        Ab = _add_at(n_cells, vcell[fo].reshape(-1), terms.reshape(-1, 9))                     # (face, corner) order
        A, b = Ab[:, :6], Ab[:, 6:]
        # rule 3
        count = np.bincount(vcell, minlength=n_cells).astype(np.int64)
        u = _add_at(n_cells, vcell, (v - centre) / cell)                                       # vertex-index order
        # rule 5
        t = (A[:, 0] + A[:, 3]) + A[:, 5]
        mean = u / count[:, None].astype(np.float64)
        x = np.where((t > 0)[:, None], _ldl3(A, b, LAMBDA * t, mean), mean)
        x = np.minimum(np.maximum(x, -0.5), 0.5)
        ucell = np.stack([(ukeys >> 42) & 0x1fffff, (ukeys >> 21) & 0x1fffff, ukeys & 0x1fffff], axis=1) - HALF
        pos = (((ucell.astype(np.float64) + 0.5) * cell) + x * cell).astype(np.float32)
        # rule 6
        out_c = out_n = None
        if colors is not None:
            csum = np.zeros((n_cells, 3), np.int64)
            np.add.at(csum, vcell, colors.astype(np.int64))
            out_c = ((2 * csum + count[:, None]) // (2 * count[:, None])).astype(np.uint8)[used]
        if normals is not None:
            S = _add_at(n_cells, vcell, normals.astype(np.float64))
            ln = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
            good = (ln > 0) & np.isfinite(ln)
            out_n = np.where(good[:, None], S / np.where(good, ln, 1.0)[:, None], 0.0).astype(np.float32)[used]
    stage("cells")
    return pos[used], out_f, out_n, out_c, vmap


def _as_device(x, dtype, device):
    if x is None:
        return None
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=device, dtype=dtype).contiguous()


@torch.no_grad()
def simplify_mesh(vertices, faces, cell, normals=None, colors=None, backend="host", device="cuda", return_tensors=False,
                  return_map=False):
    """Simplify a triangle mesh to one vertex per occupied cell of size `cell` (world units, lattice anchored at the origin).

    vertices (n, 3) (used as fp32), faces (m, 3) integers, optional per-vertex normals (n, 3) and colors (n, 3) uint8; numpy
    arrays or tensors.  Returns (vertices (k, 3) fp32, faces (j, 3) int32), then normals (k, 3) fp32 when given, colors (k, 3)
    uint8 when given, and with return_map vertex_map (n,) int32 (the output index of every input vertex, or -1).
    backend="device": the same arrays from the GPU (`device`), without a host fall-back; return_tensors=True (device backend only)
    takes and returns device tensors, with no host copy of the mesh."""
    if backend == "device":
        from . import ops
        if torch.device(device).type == "cpu" or not torch.cuda.is_available():
            raise RuntimeError('simplify_mesh(backend="device") needs a GPU: there is no host fall-back for the device path')
        cell = _check_cell(cell)
        res = ops.simplify_mesh(_as_device(vertices, torch.float32, device).reshape(-1, 3),
                                _as_device(faces, torch.int32, device).reshape(-1, 3), cell,
                                _as_device(normals, torch.float32, device), _as_device(colors, torch.uint8, device))
        if not return_tensors:
            res = tuple(None if r is None else r.cpu().numpy() for r in res)
    elif backend == "host":
        if return_tensors:
            raise ValueError('return_tensors=True needs backend="device"')
        as_np = lambda x: None if x is None else (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
        res = simplify_mesh_host(as_np(vertices), as_np(faces), cell, as_np(normals), as_np(colors))
    else:
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    v, f, nrm, col, vmap = res
    return (v, f) + (() if normals is None else (nrm,)) + (() if colors is None else (col,)) + ((vmap,) if return_map else ())


def simplify_step(vertices, faces, cell, normals=None, colors=None, backend="host", device="cuda"):
    """The scripts' last mesh step: simplify_mesh on host arrays -> (vertices, faces, normals or None, colors or None, record) with
    record = {cell, vertices_in, faces_in, vertices_out, faces_out, ms}, the `simplify` block of their JSON lines."""
    t0 = time.perf_counter()
    out = list(simplify_mesh(vertices, faces, cell, normals=normals, colors=colors, backend=backend, device=device))
    ms = 1e3 * (time.perf_counter() - t0)
    v, f = out[0], out[1]
    nrm = out[2] if normals is not None else None
    col = out[-1] if colors is not None else None
    rec = {"cell": float(cell), "vertices_in": int(len(vertices)), "faces_in": int(len(faces)), "vertices_out": int(len(v)),
           "faces_out": int(len(f)), "ms": ms}
    return v, f, nrm, col, rec
