"""Mesh smoothing: Laplacian and Taubin lambda|mu steps with uniform weights (Taubin 1995), which take lattice ripple and depth
noise out of an extracted mesh; the Taubin pair does so without shrinking the model.  Faces, colours, vertex count and vertex
order never change: only positions move, and normals are recomputed from the result when asked for.

THE RULE (rules 1-5) is written once, in include/surf_hip.h above the surf_smooth_* entry points.  backend="host" (the default)
is its numpy mirror below: fp64 on fp32 positions, one operation per operator in the header's order, per-vertex sums by np.add.at,
which adds its terms one after the other in the order given - ascending neighbour index for a step, (face, corner) order for the
normals.  backend="device" runs csrc/mesh_smooth.hip through surf_amd.ops.smooth_mesh and returns the same arrays; it has no host
fall-back.

The umbrella operator rounds edges and corners; surf_amd/mesh_denoise.py is the filter that keeps them (bilateral normal filtering).
Not attempted: cotangent weights, implicit solves, remeshing."""
import math
import time

import numpy as np
import torch

from .mesh_simplify import _add_at, _as_device

PARAMS = ("iterations", "lam", "mu", "pin_boundary", "max_move")
DEFAULTS = {"iterations": 10, "lam": 0.5, "mu": -0.53, "pin_boundary": True, "max_move": None}
MAX_ITERATIONS = 10000


def check_args(iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None):
    """The arguments as (int, float, float or None, bool, float or None); ValueError naming the value that is refused."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"smooth_mesh: iterations must be an integer in [0, {MAX_ITERATIONS}], got {iterations!r}")
    try:
        lam_f = float(lam)
    except (TypeError, ValueError):
        lam_f = float("nan")
    if not 0.0 < lam_f <= 1.0:
        raise ValueError(f"smooth_mesh: lam must satisfy 0 < lam <= 1, got {lam!r}")
    mu_f = None
    if mu is not None:
        try:
            mu_f = float(mu)
        except (TypeError, ValueError):
            mu_f = float("nan")
        if not (math.isfinite(mu_f) and mu_f < -lam_f):
            raise ValueError(f"smooth_mesh: mu must be finite with mu < -lam = {-lam_f}, got {mu!r} (None: Laplacian steps)")
    move_f = None
    if max_move is not None:
        try:
            move_f = float(max_move)
        except (TypeError, ValueError):
            move_f = float("nan")
        if not (math.isfinite(move_f) and move_f > 0.0 and 0.0 < move_f * move_f < float("inf")):
            raise ValueError(f"smooth_mesh: max_move must be finite and > 0, got {max_move!r} (None: no cap)")
    return int(iterations), lam_f, mu_f, bool(pin_boundary), move_f


def check_params(smooth):
    """A `smooth` dict (extract_mesh, the scripts) -> the full argument dict; ValueError for a key that is no argument."""
    if not isinstance(smooth, dict):
        raise ValueError(f"smooth: expected a dict of {', '.join(PARAMS)}, got {smooth!r}")
    unknown = sorted(set(smooth) - set(PARAMS))
    if unknown:
        raise ValueError(f"smooth: unknown key(s) {unknown}; the arguments are {', '.join(PARAMS)}")
    return dict(zip(PARAMS, check_args(**{**DEFAULTS, **smooth})))


def schedule(iterations, lam, mu):
    """Rule 3: the factor of every step, in order."""
    return [lam] * iterations if mu is None else [lam, mu] * iterations


def adjacency_host(faces, n):
    """Rule 1: (src, dst, boundary (n,) bool, degree (n,) int64); (src[k], dst[k]) are the neighbour pairs in ascending (src, dst)
    order, so that the entries of a vertex list N(i) in ascending order."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    keys, fwd = [], []
    for k in range(3):
        a, b = f[:, k], f[:, (k + 1) % 3]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        key = (lo << 32) | hi
        drop = lo == hi
        for earlier in fwd:                                          # the face has this edge already
            drop |= earlier == key
        fwd.append(key)
        keys += [key[~drop], ((hi << 32) | lo)[~drop]]
    ukeys, uses = np.unique(np.concatenate(keys), return_counts=True)
    src, dst = ukeys >> 32, ukeys & 0xffffffff
    boundary = np.zeros(n, bool)
    boundary[src[uses == 1]] = True
    return src, dst, boundary, np.bincount(src, minlength=n).astype(np.int64)


def step_host(x32, src, dst, degree, moves, s):
    """Rule 2: one step with factor s on fp32 positions (n, 3); moves (n,) bool = neither isolated nor pinned."""
    x = x32.astype(np.float64)
    S = _add_at(len(x), src, x[dst])
    with np.errstate(all="ignore"):
        mean = S / degree[:, None].astype(np.float64)
        new = (x + s * (mean - x)).astype(np.float32)
    return np.where(moves[:, None], new, x32)


def sum256_host(values):
    """Rule 4's 256-ary sequential tree over fp64 values (at least one)."""
    values = np.asarray(values, np.float64)
    while len(values) > 1:
        rows = np.concatenate([values, np.zeros((-len(values)) % 256)]).reshape(-1, 256)      # + 0 leaves a run's sum as it is
        acc = np.zeros(len(rows))
        for k in range(256):
            acc = acc + rows[:, k]
        values = acc
    return float(values[0])


def cap_host(x32, x0_32, max_move):
    """Rule 4: (positions fp32, q (n,) fp64 of the final positions, capped (n,) bool)."""
    x0 = x0_32.astype(np.float64)

    def movement(x):
        d = x.astype(np.float64) - x0
        return d, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    d, q = movement(x32)
    capped = np.zeros(len(x32), bool)
    if max_move is not None:
        capped = q > max_move * max_move
        with np.errstate(all="ignore"):
            r = max_move / np.sqrt(q)
            x32 = np.where(capped[:, None], (x0 + d * r[:, None]).astype(np.float32), x32)
        d, q = movement(x32)
    return x32, q, capped


def vertex_normals_host(v32, faces, given=None):
    """Rule 5: (n, 3) fp32 area-weighted vertex normals of fp32 positions; given (n, 3) fp32 normals to stay aligned with."""
    v = np.asarray(v32, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    p0 = v[f[:, 0]]
    e1, e2 = v[f[:, 1]] - p0, v[f[:, 2]] - p0
    F = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    S = _add_at(len(v), f.reshape(-1), np.repeat(F, 3, axis=0))                # (face, corner) order
    with np.errstate(all="ignore"):
        L2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
        ok = (L2 > 0) & np.isfinite(L2)
        nrm = np.where(ok[:, None], S / np.sqrt(np.where(ok, L2, 1.0))[:, None], 0.0).astype(np.float32)
    if given is not None:
        g, w = np.asarray(given, np.float32).astype(np.float64), nrm.astype(np.float64)
        t = (w[:, 0] * g[:, 0] + w[:, 1] * g[:, 1]) + w[:, 2] * g[:, 2]
        nrm = np.where((ok & (t < 0))[:, None], -nrm, nrm)
    return nrm


def _host_inputs(vertices, faces, normals):
    v32 = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces).reshape(-1, 3)
    n, m = len(v32), len(faces)
    given = None
    if normals is not None and normals is not True:
        given = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if len(given) != n:
            raise ValueError(f"smooth_mesh: normals {given.shape} for {n} vertices")
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError(f"face indices span [{faces.min()}, {faces.max()}], the mesh has {n} vertices")
    bad = np.flatnonzero(~np.isfinite(v32).all(axis=1))
    if len(bad):
        raise ValueError(f"smooth_mesh: vertex {bad[0]} is not finite: {v32[bad[0]].tolist()}")
    return v32, faces, given


def _untouched(v32, normals, given):
    n = len(v32)
    nrm = given if given is not None else (np.zeros((n, 3), np.float32) if normals is True else None)
    return v32, nrm, {"vertices": n, "boundary_vertices": 0, "isolated_vertices": n, "moved_max": 0.0, "moved_rms": 0.0, "capped": 0}


def smooth_mesh_host(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None, normals=None,
                     stages=None):
    """The rule in numpy: (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info).  normals: None (none wanted), True (wanted) or
    (n, 3) given normals that the recomputed ones stay aligned with.  stages: a list that receives (name, ms) per stage."""
    t_stage = [time.perf_counter()]

    def stage(name):
        if stages is not None:
            now = time.perf_counter()
            stages.append((name, 1e3 * (now - t_stage[0])))
            t_stage[0] = now

    iterations, lam, mu, pin_boundary, max_move = check_args(iterations, lam, mu, pin_boundary, max_move)
    v32, faces, given = _host_inputs(vertices, faces, normals)
    n = len(v32)
    if n == 0 or len(faces) == 0:
        return _untouched(v32, normals, given)
    src, dst, boundary, degree = adjacency_host(faces, n)
    moves = (degree > 0) & ~(boundary & pin_boundary)
    stage("adjacency")
    x = v32
    for s in schedule(iterations, lam, mu):
        x = step_host(x, src, dst, degree, moves, s)
    stage("steps")
    x, q, capped = cap_host(x, v32, max_move)
    info = {"vertices": n, "boundary_vertices": int(boundary.sum()), "isolated_vertices": int((degree == 0).sum()),
            "moved_max": math.sqrt(float(q.max())), "moved_rms": math.sqrt(sum256_host(q) / float(n)), "capped": int(capped.sum())}
    stage("cap")
    nrm = None if normals is None else vertex_normals_host(x, faces, given)
    stage("normals")
    return np.ascontiguousarray(x), nrm, info


def boundary_flags(faces, n, backend="host", device="cuda"):
    """(n,) bool: the boundary vertices of rule 1 (an end of an edge that exactly one face has)."""
    if backend == "host":
        faces = np.asarray(faces).reshape(-1, 3)
        if len(faces) == 0:
            return np.zeros(n, bool)
        return adjacency_host(faces, n)[2]
    if backend != "device":
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    from . import ops
    f = _as_device(faces, torch.int32, device).reshape(-1, 3)
    if len(f) == 0 or n == 0:
        return np.zeros(n, bool)
    return ops.smooth_adjacency(f, int(n))[2].cpu().numpy().astype(bool)


@torch.no_grad()
def smooth_mesh(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, max_move=None, normals=None, backend="host",
                device="cuda", return_tensors=False):
    """Smooth a triangle mesh: `iterations` Taubin pairs (a step with lam, then one with mu < -lam), or with mu=None `iterations`
    Laplacian steps with lam; every step moves a vertex towards (lam) or away from (mu) the mean of its edge neighbours.

    vertices (n, 3) (used as fp32, all finite), faces (m, 3) integers; numpy arrays or tensors.  pin_boundary: vertices on an edge
    of exactly one face stay where they are.  max_move (world units): no vertex ends further than that from where it started.
    normals: None, True (recompute them from the result) or (n, 3) normals (recompute, and keep each on its given normal's side).
    Returns (vertices (n, 3) fp32, normals (n, 3) fp32 or None, info) with info = {vertices, boundary_vertices, isolated_vertices,
    moved_max, moved_rms, capped}.  backend="device": the same arrays from the GPU (`device`), without a host fall-back;
    return_tensors=True (device backend only) takes and returns device tensors, with no host copy of the mesh."""
    if backend == "device":
        from . import ops
        if torch.device(device).type == "cpu" or not torch.cuda.is_available():
            raise RuntimeError('smooth_mesh(backend="device") needs a GPU: there is no host fall-back for the device path')
        args = check_args(iterations, lam, mu, pin_boundary, max_move)
        given = normals if normals is None or normals is True else _as_device(normals, torch.float32, device)
        v, nrm, info = ops.smooth_mesh(_as_device(vertices, torch.float32, device).reshape(-1, 3),
                                       _as_device(faces, torch.int32, device).reshape(-1, 3), *args, normals=given)
        if not return_tensors:
            v, nrm = v.cpu().numpy(), None if nrm is None else nrm.cpu().numpy()
        return v, nrm, info
    if backend != "host":
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    if return_tensors:
        raise ValueError('return_tensors=True needs backend="device"')
    as_np = lambda x: x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return smooth_mesh_host(as_np(vertices), as_np(faces), iterations, lam, mu, pin_boundary, max_move, normals=as_np(normals))


def smooth_step(vertices, faces, smooth, normals=None, backend="host", device="cuda"):
    """The scripts' smoothing step: smooth_mesh on host arrays with the arguments of the dict `smooth` -> (vertices fp32, normals or
    None, record) with record = the arguments, info and ms, the `smooth` block of their JSON lines."""
    params = check_params(smooth)
    t0 = time.perf_counter()
    v, nrm, info = smooth_mesh(vertices, faces, normals=normals, backend=backend, device=device, **params)
    ms = 1e3 * (time.perf_counter() - t0)
    return v, nrm, {**params, **info, "ms": ms}
