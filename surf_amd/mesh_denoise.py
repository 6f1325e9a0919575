"""Feature-preserving mesh denoising: two-stage bilateral normal filtering.  Stage one filters the face normals over the faces
that share a vertex, with a weight that falls with the distance of the centroids AND with the difference of the normals, so that
faces across a crease do not average each other (Zheng, Fu, Au, Tai 2011, local iterative scheme); stage two moves the vertices
to fit the filtered normals (Sun, Rosin, Martin, Langbein 2007).  Depth noise and lattice ripple go, edges and corners stay, where
the umbrella operator of surf_amd/mesh_smooth.py rounds them.  Faces, colours, vertex count and vertex order never change.

THE RULE (rules 1-6) is written once, in include/surf_hip.h above the surf_denoise_* entry points.  backend="host" (the default)
is its numpy mirror below: fp64 on fp32 data, one operation per operator in the header's order, per-row sums by np.add.at, which
adds its terms one after the other in the order given.  backend="device" runs csrc/mesh_denoise.hip through
surf_amd.ops.denoise_mesh and returns the same arrays; it has no host fall-back."""
import math
import time

import numpy as np
import torch

from .mesh_simplify import _add_at, _as_device
from .mesh_smooth import MAX_ITERATIONS, _host_inputs, adjacency_host, cap_host, sum256_host, vertex_normals_host

PARAMS = ("normal_iterations", "vertex_iterations", "sigma_r", "sigma_s", "pin_boundary", "max_move")
DEFAULTS = {"normal_iterations": 10, "vertex_iterations": 10, "sigma_r": 0.35, "sigma_s": None, "pin_boundary": True,
            "max_move": None}
MAX_NEIGHBOURS = 2 ** 31 - 1       # entries of the face neighbour list (int32 offsets), host and device paths alike


def _positive(value, name, absent):
    """float(value) if it is finite and > 0 with a finite, positive square; ValueError naming it otherwise."""
    try:
        x = float(value)
    except (TypeError, ValueError):
        x = float("nan")
    if not (math.isfinite(x) and x > 0.0 and 0.0 < x * x < float("inf")):
        raise ValueError(f"denoise_mesh: {name} must be finite and > 0, got {value!r}{absent}")
    return x


def check_args(normal_iterations=10, vertex_iterations=10, sigma_r=0.35, sigma_s=None, pin_boundary=True, max_move=None):
    """The arguments as (int, int, float, float or None, bool, float or None); ValueError naming the value that is refused."""
    for name, it in (("normal_iterations", normal_iterations), ("vertex_iterations", vertex_iterations)):
        if isinstance(it, bool) or not isinstance(it, (int, np.integer)) or not 0 <= it <= MAX_ITERATIONS:
            raise ValueError(f"denoise_mesh: {name} must be an integer in [0, {MAX_ITERATIONS}], got {it!r}")
    r = _positive(sigma_r, "sigma_r", "")
    s = None if sigma_s is None else _positive(sigma_s, "sigma_s", " (None: the mean side length)")
    move = None if max_move is None else _positive(max_move, "max_move", " (None: no cap)")
    return int(normal_iterations), int(vertex_iterations), r, s, bool(pin_boundary), move


def check_params(denoise):
    """A `denoise` dict (extract_mesh, the scripts) -> the full argument dict; ValueError for a key that is no argument."""
    if not isinstance(denoise, dict):
        raise ValueError(f"denoise: expected a dict of {', '.join(PARAMS)}, got {denoise!r}")
    unknown = sorted(set(denoise) - set(PARAMS))
    if unknown:
        raise ValueError(f"denoise: unknown key(s) {unknown}; the arguments are {', '.join(PARAMS)}")
    return dict(zip(PARAMS, check_args(**{**DEFAULTS, **denoise})))


def mean_side(total, m):
    """Rule 2's last step: sigma_s from the tree sum of the 3 m side lengths; ValueError if it is not finite and > 0."""
    s = total / float(3 * m)
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"denoise_mesh: the mean side length of the mesh is {s!r}: give sigma_s")
    return s


def inverse_supports(sigma_s, sigma_r):
    """Rule 4's constants (is, ir) in fp64."""
    return 1.0 / (9.0 * sigma_s * sigma_s), 1.0 / (9.0 * sigma_r * sigma_r)


def face_records_host(v32, faces):
    """Rules 1 and 2: (records (m, 8) fp32, degenerate (m,) bool, side lengths (3 m,) fp64 in (face, side) order)."""
    v = v32.astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    F = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    records = np.zeros((len(f), 8), np.float32)
    with np.errstate(all="ignore"):
        L2 = (F[:, 0] * F[:, 0] + F[:, 1] * F[:, 1]) + F[:, 2] * F[:, 2]
        ok = (L2 > 0) & np.isfinite(L2)
        L = np.sqrt(np.where(ok, L2, 1.0))
        records[:, 0:3] = np.where(ok[:, None], F / L[:, None], 0.0).astype(np.float32)
        records[:, 3] = np.where(ok, 0.5 * L, 0.0).astype(np.float32)
        records[:, 4:7] = np.where(ok[:, None], ((p0 + p1) + p2) / 3.0, 0.0).astype(np.float32)
        sides = []
        for a, b in ((p0, p1), (p1, p2), (p2, p0)):
            d = b - a
            sides.append(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return records, ~ok, np.stack(sides, axis=1).reshape(-1)


def corners_host(faces, n):
    """(corner_order (3 m) int64, corner_start (n + 1) int64): the corners by vertex, in (face, corner) order within a vertex."""
    flat = np.asarray(faces).reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable")
    return order, np.searchsorted(flat[order], np.arange(n + 1))


def face_neighbours_host(faces, n):
    """Rule 3 as a CSR: (face_row_start (m + 1) int64, face_neighbours (total) int32)."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    m = len(f)
    order, start = corners_host(f, n)
    flat = f.reshape(-1)
    lengths = (start[1:] - start[:-1])[flat]                           # the corner list of every (face, slot)
    walked = np.zeros((m, 3), bool)                                    # the slot equals an earlier slot of its face
    walked[:, 1] = f[:, 1] == f[:, 0]
    walked[:, 2] = (f[:, 2] == f[:, 0]) | (f[:, 2] == f[:, 1])
    lengths = np.where(walked.reshape(-1), 0, lengths)
    total = int(lengths.sum())
    slot = np.repeat(np.arange(3 * m), lengths)                        # (face, slot) of every candidate, in the rule's order
    first = np.cumsum(lengths) - lengths
    pos = np.arange(total) - np.repeat(first, lengths)
    v = flat[slot]
    c = order[start[v] + pos]
    g, j = c // 3, c % 3
    face, k = slot // 3, slot % 3
    G = f[g]
    f0, f1 = f[face, 0], f[face, 1]
    drop = ((j >= 1) & (G[:, 0] == v)) | ((j == 2) & (G[:, 1] == v))
    drop |= (k >= 1) & (G == f0[:, None]).any(axis=1)
    drop |= (k == 2) & (G == f1[:, None]).any(axis=1)
    keep = ~drop
    rows = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(face[keep], minlength=m), out=rows[1:])
    if rows[-1] > MAX_NEIGHBOURS:
        raise ValueError(f"denoise_mesh: {int(rows[-1])} face neighbours exceed the limit of {MAX_NEIGHBOURS}")
    return rows, g[keep].astype(np.int32)


def spatial_factors_host(records, entry_face, entry_nbr, inv_s):
    """The part of rule 4's weight that no iteration changes: (entry_face, entry_nbr, a) of the entries with us > 0, in order, with
    a = (double)area_g * ((us*us)*(us*us)); entry_face / entry_nbr list (f, g) for g in N(f), row after row."""
    cen = records[:, 4:7].astype(np.float64)
    with np.errstate(all="ignore"):
        d = cen[entry_nbr] - cen[entry_face]
        us = 1.0 - ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) * inv_s
        use = us > 0.0
        us, entry_face, entry_nbr = us[use], entry_face[use], entry_nbr[use]
        return entry_face, entry_nbr, records[:, 3].astype(np.float64)[entry_nbr] * ((us * us) * (us * us))


def normal_step_host(normals32, degenerate, entry_face, entry_nbr, spatial, inv_r):
    """Rule 4: one iteration on fp32 normals (m, 3), over the entries and factors of spatial_factors_host."""
    nrm = normals32.astype(np.float64)
    with np.errstate(all="ignore"):
        ng = nrm[entry_nbr]
        e = ng - nrm[entry_face]
        ur = 1.0 - ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) * inv_r
        use = ur > 0.0
        ur, ng = ur[use], ng[use]
        w = spatial[use] * ((ur * ur) * (ur * ur))
        S = _add_at(len(nrm), entry_face[use], w[:, None] * ng)
        L2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
        ok = (L2 > 0) & np.isfinite(L2) & ~degenerate
        new = (S / np.sqrt(np.where(ok, L2, 1.0))[:, None]).astype(np.float32)
    return np.where(ok[:, None], new, normals32)


def vertex_step_host(x32, faces, normals32, corner_vertex, corner_face, count, moves):
    """Rule 5: one iteration on fp32 positions (n, 3); corner_vertex / corner_face list the corners of faces that are not
    degenerate by vertex in (face, corner) order, count (n,) is k_i, moves (n,) bool = k_i > 0 and not pinned."""
    x = x32.astype(np.float64)
    nrm = normals32.astype(np.float64)[corner_face]
    with np.errstate(all="ignore"):
        cen = (((x[faces[:, 0]] + x[faces[:, 1]]) + x[faces[:, 2]]) / 3.0)[corner_face]
        r = cen - x[corner_vertex]
        d = (r[:, 0] * nrm[:, 0] + r[:, 1] * nrm[:, 1]) + r[:, 2] * nrm[:, 2]
        T = _add_at(len(x), corner_vertex, nrm * d[:, None])
        new = (x + T / count[:, None].astype(np.float64)).astype(np.float32)
    return np.where(moves[:, None], new, x32)


def _untouched(v32, m, normals, given, sigma_r, sigma_s):
    n = len(v32)
    nrm = given if given is not None else (np.zeros((n, 3), np.float32) if normals is True else None)
    return v32, nrm, {"vertices": n, "faces": m, "degenerate_faces": 0, "boundary_vertices": 0, "sigma_s": sigma_s,
                      "sigma_r": sigma_r, "moved_max": 0.0, "moved_rms": 0.0, "capped": 0}


def denoise_mesh_host(vertices, faces, normal_iterations=10, vertex_iterations=10, sigma_r=0.35, sigma_s=None, pin_boundary=True,
                      max_move=None, normals=None, stages=None, keep=None, neighbours=None):
    """The rule in numpy: (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info).  normals: None (none wanted), True (wanted) or
    (n, 3) given normals that the recomputed ones stay aligned with.  stages: a list that receives (name, ms) per stage.  keep: a
    dict that receives the intermediate arrays face_row_start, face_neighbours (when there is a normal iteration) and records
    (m, 8), the face records after the normal stage.  neighbours: face_neighbours_host(faces, n) of THIS mesh, for a caller that
    denoises one mesh several times and would not build the list each time."""
    t_stage = [time.perf_counter()]

    def stage(name):
        if stages is not None:
            now = time.perf_counter()
            stages.append((name, 1e3 * (now - t_stage[0])))
            t_stage[0] = now

    normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move = check_args(
        normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move)
    try:
        v32, faces, given = _host_inputs(vertices, faces, normals)
    except ValueError as e:
        raise ValueError(str(e).replace("smooth_mesh:", "denoise_mesh:")) from None
    n, m = len(v32), len(faces)
    if n == 0 or m == 0:
        return _untouched(v32, m, normals, given, sigma_r, sigma_s)
    f = faces.astype(np.int64)
    boundary = adjacency_host(f, n)[2]
    records, degenerate, sides = face_records_host(v32, f)
    if sigma_s is None:
        sigma_s = mean_side(sum256_host(sides), m)
    inv_s, inv_r = inverse_supports(sigma_s, sigma_r)
    stage("records")
    nrm32 = np.ascontiguousarray(records[:, 0:3])
    if normal_iterations:
        rows, nbr = face_neighbours_host(f, n) if neighbours is None else neighbours
        if rows.shape != (m + 1,) or rows[-1] != len(nbr):
            raise ValueError(f"denoise_mesh: neighbours of {len(rows) - 1} faces and {len(nbr)} entries for a mesh of {m} faces")
        if keep is not None:
            keep.update(face_row_start=rows, face_neighbours=nbr)
        entry_face, entry_nbr, spatial = spatial_factors_host(records, np.repeat(np.arange(m), rows[1:] - rows[:-1]),
                                                              nbr.astype(np.int64), inv_s)
        stage("neighbours")
        for _ in range(normal_iterations):
            nrm32 = normal_step_host(nrm32, degenerate, entry_face, entry_nbr, spatial, inv_r)
        del entry_face, entry_nbr, spatial
        stage("normal_steps")
    if keep is not None:
        records = records.copy()
        records[:, 0:3] = nrm32
        keep.update(records=records)
    x = v32
    if vertex_iterations:
        order, _ = corners_host(f, n)
        corner_face = order // 3
        live = ~degenerate[corner_face]
        corner_face = corner_face[live]
        corner_vertex = f.reshape(-1)[order][live]
        count = np.bincount(corner_vertex, minlength=n).astype(np.int64)
        moves = (count > 0) & ~(boundary & pin_boundary)
        for _ in range(vertex_iterations):
            x = vertex_step_host(x, f, nrm32, corner_vertex, corner_face, count, moves)
        stage("vertex_steps")
    x, q, capped = cap_host(x, v32, max_move)
    info = {"vertices": n, "faces": m, "degenerate_faces": int(degenerate.sum()), "boundary_vertices": int(boundary.sum()),
            "sigma_s": sigma_s, "sigma_r": sigma_r, "moved_max": math.sqrt(float(q.max())),
            "moved_rms": math.sqrt(sum256_host(q) / float(n)), "capped": int(capped.sum())}
    stage("cap")
    nrm = None if normals is None else vertex_normals_host(x, faces, given)
    stage("normals")
    return np.ascontiguousarray(x), nrm, info


@torch.no_grad()
def denoise_mesh(vertices, faces, normal_iterations=10, vertex_iterations=10, sigma_r=0.35, sigma_s=None, pin_boundary=True,
                 max_move=None, normals=None, backend="host", device="cuda", return_tensors=False):
    """Denoise a triangle mesh and keep its edges and corners: `normal_iterations` bilateral filter passes over the face normals,
    then `vertex_iterations` passes that move every vertex towards the planes its faces should lie in.

    vertices (n, 3) (used as fp32, all finite), faces (m, 3) integers; numpy arrays or tensors.  sigma_r: how far two unit normals
    may differ (as a chord length) and still average each other - the weight vanishes at 3 sigma_r, 1.05 by default, so that
    faces across a right angle (chord 1.41) never mix.  sigma_s (world units): the same for the distance of two centroids; None
    takes the mean side length of the mesh.  pin_boundary: vertices on an edge of exactly one face stay where they are.  max_move
    (world units): no vertex ends further than that from where it started.  normals: None, True (recompute them from the result)
    or (n, 3) normals (recompute, and keep each on its given normal's side).
    Returns (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info) with info = {vertices, faces, degenerate_faces,
    boundary_vertices, sigma_s, sigma_r, moved_max, moved_rms, capped}.  backend="device": the same arrays from the GPU (`device`),
    without a host fall-back; return_tensors=True (device backend only) takes and returns device tensors."""
    if backend == "device":
        from . import ops
        if torch.device(device).type == "cpu" or not torch.cuda.is_available():
            raise RuntimeError('denoise_mesh(backend="device") needs a GPU: there is no host fall-back for the device path')
        args = check_args(normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move)
        given = normals if normals is None or normals is True else _as_device(normals, torch.float32, device)
        v, nrm, info = ops.denoise_mesh(_as_device(vertices, torch.float32, device).reshape(-1, 3),
                                        _as_device(faces, torch.int32, device).reshape(-1, 3), *args, normals=given)
        if not return_tensors:
            v, nrm = v.cpu().numpy(), None if nrm is None else nrm.cpu().numpy()
        return v, nrm, info
    if backend != "host":
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    if return_tensors:
        raise ValueError('return_tensors=True needs backend="device"')
    as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return denoise_mesh_host(as_np(vertices), as_np(faces), normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary,
                             max_move, normals=as_np(normals))


def denoise_step(vertices, faces, denoise, normals=None, backend="host", device="cuda"):
    """The scripts' denoising step: denoise_mesh on host arrays with the arguments of the dict `denoise` -> (vertices fp32, normals
    or None, record) with record = the arguments, info and ms, the `denoise` block of their JSON lines (sigma_s is the value
    used)."""
    params = check_params(denoise)
    t0 = time.perf_counter()
    v, nrm, info = denoise_mesh(vertices, faces, normals=normals, backend=backend, device=device, **params)
    ms = 1e3 * (time.perf_counter() - t0)
    return v, nrm, {**params, **info, "ms": ms}
