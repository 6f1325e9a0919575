"""Textured meshes: the source photographs baked into one atlas image, so that a mesh of any density - a simplified one above all -
carries the photographs' detail and not one colour per vertex.  Positions, faces and vertex order are never touched; the result is
(uv, atlas) for mesh_io.write_obj.

    views = [view_from_item(item, k) for k in range(n_photographs)]            # world frame, full resolution
    uv, atlas = bake_texture(vertices, faces, views, texels_per_edge=8, depth_tol=2 * voxel, backend="device")
    mesh_io.write_obj("scan24_textured.obj", vertices, faces, uv, atlas)

THE RULE (rules 1-5) is written once, in include/surf_hip.h above the surf_texture_* entry points: a per-triangle atlas laid out by
arithmetic alone, every texel lifted to its point of the face, projected into every view, tested against the z-buffer of the mesh
itself at the four pixels of its bilinear footprint (all four within depth_tol of the texel's depth, nearer or further), and the
views that see it blended with weight cos^power.  backend="host" (the default) is the numpy mirror below: fp32, one operation per
operator in the header's order.  backend="device" runs
csrc/mesh_texture.hip through surf_amd.ops.bake_texture and returns the same arrays, bit for bit; it has no host fall-back.

The depth maps are the z-buffer of the mesh from every camera (mesh_depth_maps: surf_raster_first_hit in the view's own pixel units,
whose keys carry the fp32 depth).  That stage always runs on the device, as clean_mesh's first-hit test does; bake_texture(...,
mesh_depths=[...]) takes given maps, which keeps the host path free of the GPU.  The rasteriser's near rule stands: a face with a
vertex behind a camera (depth <= 1e-6) is not drawn for it and occludes nothing there.

Not in here: area-proportional or merged charts (every face gets the same T (T+1) / 2 texels, whatever its size); seam or exposure
levelling between views; a best-single-view mode (a large `power` approximates it); extract_mesh(texture=...); texturing the
--cloud_mesh; a renderer for the textured mesh."""
import math
import time
from collections import namedtuple

import numpy as np
import torch

from .fusion import _lerp, _np, _split_P, quantise_colors_host, similarity_scale
from .mesh_simplify import _as_device

TextureView = namedtuple("TextureView", "P image")
TextureView.__doc__ = """One photograph to bake.  P (3, 4): world -> (x z, y z, z), z in world units, x / y in pixel indices of `image`
(DepthView's convention); image (H, W, 3) fp32 in [0, 1] (array or tensor), H, W >= 2.  Views may differ in size."""

PARAMS = ("texels_per_edge", "depth_tol", "min_cos", "power", "two_sided", "z_min", "fill")
DEFAULTS = {"texels_per_edge": 8, "min_cos": 0.2, "power": 4, "two_sided": False, "z_min": 0.0, "fill": 0.5}
MAX_VIEWS = 16                  # SURF_FUSE_MAX_VIEWS: views per launch of surf_texture_bake
MAX_ATLAS_SIDE = 16384
HOST_CHUNK = 1 << 20            # texels per pass of the numpy mirror (texels are independent: the chunking is invisible)
_F32_MAX = np.float32(np.finfo(np.float32).max)


def _real(value, name, ok, want):
    try:
        f = float(value)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(value, bool) or not ok(f):
        raise ValueError(f"bake_texture: {name} must be {want}, got {value!r}")
    return f


def check_args(texels_per_edge=8, depth_tol=None, min_cos=0.2, power=4, two_sided=False, z_min=0.0, fill=0.5):
    """The arguments as (int, float, float, int, bool, float, float); ValueError naming the value that is refused."""
    for name, v, lo, hi in (("texels_per_edge", texels_per_edge, 4, 64), ("power", power, 1, 16)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"bake_texture: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    if depth_tol is None:
        raise ValueError("bake_texture: depth_tol has no default (world units; the scripts use two lattice steps), got None")
    fin = math.isfinite
    return (int(texels_per_edge), _real(depth_tol, "depth_tol", lambda f: fin(f) and f >= 0.0, "finite and >= 0"),
            _real(min_cos, "min_cos", lambda f: 0.0 <= f <= 1.0, "in [0, 1]"), int(power), bool(two_sided),
            _real(z_min, "z_min", lambda f: fin(f) and f >= 0.0, "finite and >= 0"),
            _real(fill, "fill", lambda f: 0.0 <= f <= 1.0, "in [0, 1]"))


def check_params(texture):
    """A `texture` dict (the scripts) -> the full argument dict; ValueError for a key that is no argument."""
    if not isinstance(texture, dict):
        raise ValueError(f"texture: expected a dict of {', '.join(PARAMS)}, got {texture!r}")
    unknown = sorted(set(texture) - set(PARAMS))
    if unknown:
        raise ValueError(f"texture: unknown key(s) {unknown}; the arguments are {', '.join(PARAMS)}")
    return dict(zip(PARAMS, check_args(**{**DEFAULTS, **texture})))


def view_from_item(inputs, k=0):
    """The TextureView of source photograph k of a `val` item (intrs, c2ws, scale_mat, imgs), in the world frame at the
    photograph's own resolution: fusion.view_from_val's float64 recipe without the lattice scaling.  With S = scale_mat (normalised
    -> world, a similarity of scale s): P = K_k (s (w2c_k S^-1))[:3, :4], formed in float64 and rounded to fp32 once."""
    imgs = inputs["imgs"]
    imgs = imgs.reshape((-1,) + tuple(imgs.shape[-3:]))
    S = _np(inputs["scale_mat"], np.float64).reshape(4, 4)
    K = _np(inputs["intrs"], np.float64).reshape(-1, 4, 4)[k, :3, :3]
    w2c = np.linalg.inv(_np(inputs["c2ws"], np.float64).reshape(-1, 4, 4)[k])
    P = (K @ (similarity_scale(S) * (w2c @ np.linalg.inv(S)))[:3, :4]).astype(np.float32)
    image = imgs[k].permute(1, 2, 0) if torch.is_tensor(imgs) else np.moveaxis(np.asarray(imgs[k]), 0, -1)
    return TextureView(P, _np(image, np.float32))


def view_centre(P):
    """The camera centre c = -M^-1 t of P = [M | t], formed in float64 and rounded once (fusion.lift_transform's)."""
    M, t, M_inv = _split_P(TextureView(P, None))
    return (-(M_inv @ t)).astype(np.float32)


def atlas_layout(m, T):
    """Rule 1: (ncell, cols, rows, Ha, Wa) of m faces at T texels per edge.  ValueError for a T outside [4, 64] and for an atlas
    side above 16384."""
    m = int(m)
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not 4 <= T <= 64 or m < 0:
        raise ValueError(f"atlas_layout: texels_per_edge must be an integer in [4, 64] and m >= 0, got T = {T!r}, m = {m}")
    T = int(T)
    ncell = (m + 1) // 2
    cols = math.isqrt(ncell)
    cols += cols * cols < ncell
    rows = -(-ncell // cols) if cols else 0
    Ha, Wa = rows * T, cols * (T + 1)
    if max(Ha, Wa) > MAX_ATLAS_SIDE:
        raise ValueError(f"bake_texture: {m} faces at texels_per_edge = {T} need an atlas of {Ha} x {Wa} texels, a side above "
                         f"{MAX_ATLAS_SIDE}: lower texels_per_edge, or simplify the mesh first (--simplify_mm)")
    return ncell, cols, rows, Ha, Wa


def face_uv(m, T):
    """Rule 1: uv (3m, 2) fp32, one row per face corner, the corners at the centres of their texels, v pointing up."""
    _, cols, _, Ha, Wa = atlas_layout(m, T)
    f = np.arange(int(m), dtype=np.int64)
    k, B = f // 2, (f % 2).astype(bool)
    ci = np.where(B[:, None], [[T, 2, T]], [[0, T - 2, 0]])
    cj = np.where(B[:, None], [[T - 1, T - 1, 1]], [[0, 0, T - 2]])
    x = ((k % max(cols, 1)) * (T + 1))[:, None] + ci
    y = ((k // max(cols, 1)) * T)[:, None] + cj
    uv = np.stack([(x + 0.5) / max(Wa, 1), 1.0 - (y + 0.5) / max(Ha, 1)], axis=-1)
    return uv.reshape(-1, 2).astype(np.float32)


def texel_faces(t, m, T, cols, Wa):
    """Rule 1 for the flat texel indices t (int64 array): (face (>= m: no face), i_or_T-i, j_or_T-1-j) - the integers whose
    quotients by T-2 are rule 2's beta and gamma."""
    Y, X = t // Wa, t % Wa
    cc, i = X // (T + 1), X % (T + 1)
    r, j = Y // T, Y % T
    B = i + j >= T
    return 2 * (r * cols + cc) + B, np.where(B, T - i, i), np.where(B, T - 1 - j, j)


def _faces32(faces):
    """Faces as int32 (m, 3); an index that is no int32 stays out of range (-1)."""
    f = _np(faces).reshape(-1, 3)
    if f.dtype != np.int32:
        f = np.where((f < 0) | (f > 2 ** 31 - 1), -1, f).astype(np.int32)
    return np.ascontiguousarray(f)


def _host_views(views, mesh_depths):
    out = []
    for k, (view, depth) in enumerate(zip(views, mesh_depths)):
        image, depth = _np(view.image, np.float32), _np(depth, np.float32)
        if image.ndim != 3 or image.shape[2] != 3 or min(image.shape[:2]) < 2 or depth.shape != image.shape[:2]:
            raise ValueError(f"bake_texture: views[{k}] needs an image (H, W, 3) with H, W >= 2 and a depth map (H, W), got "
                             f"{image.shape} and {depth.shape}")
        P = _np(view.P, np.float32).reshape(12)
        out.append((P, view_centre(view.P), image, depth))
    return out


def bake_host(v32, f32i, T, views, depth_tol, min_cos, power, two_sided, z_min, sums, count=None):
    """Rules 1-4 in numpy fp32 into sums (Ha, Wa, 4) (sum_r, sum_g, sum_b, sum_w) and count (Ha, Wa) int32 or None, both fully
    written.  views: (P (12,), centre (3,), image, depth) per view, in order."""
    f32 = np.float32
    n, m = len(v32), len(f32i)
    _, cols, _, Ha, Wa = atlas_layout(m, T)
    flat, cflat = sums.reshape(-1, 4), None if count is None else count.reshape(-1)
    vpad = v32 if n else np.zeros((1, 3), f32)
    depth_tol, min_cos, z_min, den = f32(depth_tol), f32(min_cos), f32(z_min), f32(T - 2)
    for s in range(0, Ha * Wa, HOST_CHUNK):
        t = np.arange(s, min(s + HOST_CHUNK, Ha * Wa), dtype=np.int64)
        face, bi, gi = texel_faces(t, m, T, cols, Wa)
        acc, cnt = np.zeros((len(t), 4), f32), np.zeros(len(t), np.int32)
        live = face < m
        idx = f32i[np.where(live, face, 0)].astype(np.int64)
        live &= ((idx >= 0) & (idx < n)).all(axis=1)
        idx = np.where(live[:, None], idx, 0)
        a, b, c = vpad[idx[:, 0]], vpad[idx[:, 1]], vpad[idx[:, 2]]
        with np.errstate(all="ignore"):
            live &= np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
            beta, gamma = (bi.astype(f32) / den)[:, None], (gi.astype(f32) / den)[:, None]
            e1, e2 = b - a, c - a
            p = (a + beta * e1) + gamma * e2
            nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                            e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
            live &= (nn > 0) & (nn <= _F32_MAX)
            ln = np.sqrt(nn)
            px, py, pz = p[:, 0], p[:, 1], p[:, 2]
            for P, centre, image, depth in views:
                H, W = depth.shape
                cx = ((P[0] * px + P[1] * py) + P[2] * pz) + P[3]
                cy = ((P[4] * px + P[5] * py) + P[6] * pz) + P[7]
                z = ((P[8] * px + P[9] * py) + P[10] * pz) + P[11]
                ok = live & (z > z_min)
                x, y = cx / z, cy / z
                ok &= (x >= 0) & (x <= f32(W - 1)) & (y >= 0) & (y <= f32(H - 1))
                d = centre[None, :] - p
                nd = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
                dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                cs = nd / (ln * np.sqrt(dd))
                if two_sided:
                    cs = np.abs(cs)
                ok &= cs >= min_cos
                x0 = np.minimum(np.where(ok, np.floor(x), 0).astype(np.int64), W - 2)
                y0 = np.minimum(np.where(ok, np.floor(y), 0).astype(np.int64), H - 2)
                u, v = x - x0.astype(f32), y - y0.astype(f32)
                for dy in (0, 1):
                    for dx in (0, 1):
                        D = depth[y0 + dy, x0 + dx]
                        ok &= (D > 0) & (z <= D + depth_tol) & (D <= z + depth_tol)
                w = cs
                for _ in range(power - 1):
                    w = w * cs
                top = _lerp(image[y0, x0], image[y0, x0 + 1], u[:, None])
                bot = _lerp(image[y0 + 1, x0], image[y0 + 1, x0 + 1], u[:, None])
                col = _lerp(top, bot, v[:, None])
                acc[:, :3] = np.where(ok[:, None], acc[:, :3] + w[:, None] * col, acc[:, :3])
                acc[:, 3] = np.where(ok, acc[:, 3] + w, acc[:, 3])
                cnt += ok
        flat[t] = acc
        if cflat is not None:
            cflat[t] = cnt
    return sums


def finish_host(sums, f32i, n, T, vertex_colors=None, fill=0.5):
    """Rule 5 in numpy fp32: atlas (Ha, Wa, 3) uint8 of sums (Ha, Wa, 4)."""
    f32 = np.float32
    m = len(f32i)
    _, cols, _, Ha, Wa = atlas_layout(m, T)
    flat = sums.reshape(-1, 4)
    face, bi, gi = texel_faces(np.arange(Ha * Wa, dtype=np.int64), m, T, cols, Wa)
    owned = face < m
    val = np.full((Ha * Wa, 3), f32(fill), f32)
    with np.errstate(all="ignore"):
        seen = owned & (flat[:, 3] > 0)
        val = np.where(seen[:, None], flat[:, :3] / flat[:, 3:4], val)
        if vertex_colors is not None:
            idx = f32i[np.where(owned, face, 0)].astype(np.int64)
            mix = owned & ~seen & ((idx >= 0) & (idx < n)).all(axis=1)
            idx = np.where(mix[:, None], idx, 0)
            vc = vertex_colors if n else np.zeros((1, 3), np.uint8)
            beta, gamma = bi.astype(f32) / f32(T - 2), gi.astype(f32) / f32(T - 2)
            s = beta + gamma
            beta, gamma = np.where(s > 1, beta / s, beta), np.where(s > 1, gamma / s, gamma)
            alpha = (f32(1.0) - beta) - gamma
            ca, cb, cc = (vc[idx[:, e]].astype(f32) / f32(255.0) for e in range(3))
            val = np.where(mix[:, None], (alpha[:, None] * ca + beta[:, None] * cb) + gamma[:, None] * cc, val)
    return quantise_colors_host(val).reshape(Ha, Wa, 3)


def bake_stats(sum_w, count, m, T):
    """The counts of the scripts' `texture` block from sum_w (Ha, Wa) and count (Ha, Wa) int32."""
    _, cols, _, Ha, Wa = atlas_layout(m, T)
    face, _, _ = texel_faces(np.arange(Ha * Wa, dtype=np.int64), m, T, cols, Wa)
    owned = face < m
    seen = owned & (np.asarray(sum_w).reshape(-1) > 0)
    faces_seen = np.zeros(m, bool)
    faces_seen[face[seen]] = True
    n_seen = int(seen.sum())
    return {"atlas": [Ha, Wa], "faces": int(m), "texels_owned": int(owned.sum()), "texels_seen": n_seen,
            "seen_share": n_seen / max(int(owned.sum()), 1), "faces_unseen": int(m - faces_seen.sum()),
            "views_per_seen_texel": float(np.asarray(count).reshape(-1)[seen].sum()) / max(n_seen, 1)}


def _valid_faces(f32i, n):
    return f32i[((f32i >= 0) & (f32i < n)).all(axis=1)]


@torch.no_grad()
def mesh_depth_maps(vertices, faces, views, device="cuda"):
    """The z-buffer of the mesh from every view's camera: a list of (H, W) fp32 device tensors, z-depth in world units at the
    view's own pixels, 0 where nothing is hit.  views: TextureViews, or (P, (H, W)) pairs.  Always on the device
    (surf_raster_first_hit with K = I, w2c = P: the fp32 depth is the upper half of its keys).  Faces with an index out of range
    are left out; the rasteriser's rules stand: a face with a non-finite vertex or of zero screen area is not drawn, and a face
    with a vertex at camera depth <= 1e-6 is not drawn at all, so it occludes nothing from that camera."""
    from . import ops
    if torch.device(device).type == "cpu" or not torch.cuda.is_available():
        raise RuntimeError("mesh_depth_maps needs a GPU: the rasteriser has no host path (pass mesh_depths= to bake_texture)")
    v = _as_device(vertices, torch.float32, device).reshape(-1, 3)
    f = torch.from_numpy(_valid_faces(_faces32(faces), len(v))).to(device)
    out = []
    for view in views:
        P, second = view[0], view[1]
        hw = tuple(int(s) for s in (second.shape[:2] if hasattr(second, "shape") and len(second.shape) == 3 else second))
        out.append(ops.raster_depth(v, f, np.asarray(_np(P), np.float32).reshape(3, 4), hw))
    return out


@torch.no_grad()
def bake_texture(vertices, faces, views, texels_per_edge=8, depth_tol=None, min_cos=0.2, power=4, two_sided=False, z_min=0.0,
                 fill=0.5, vertex_colors=None, mesh_depths=None, backend="host", device=None, stats=None, return_sums=False,
                 sums=None):
    """Bake the photographs `views` (TextureViews, in order) into a per-triangle atlas of the mesh: (uv (3m, 2) fp32, one row per
    face corner, atlas (Ha, Wa, 3) uint8).  vertices (n, 3) (used as fp32), faces (m, 3) integers; numpy arrays or tensors.

    texels_per_edge T in [4, 64]: every face gets T (T+1) / 2 texels.  depth_tol (world units, no default): a texel is hidden from
    a view unless the mesh's own depth map lies within this of the texel's depth at all four pixels around its projection.
    min_cos: views that look at the face more obliquely are not used (two_sided: either side of the face counts); a view's weight
    is cos^power (integer, 1..16).  z_min: nearest camera depth used.  A texel no view sees takes the mix of vertex_colors (n, 3)
    uint8 when given, `fill` otherwise; faces with an index out of range, a vertex that is not finite or no area are filled the
    same way and raise nothing.  mesh_depths: the (H, W) fp32 z-buffers of the mesh, one per view (default: mesh_depth_maps, on the
    device whatever the backend).  stats (dict): receives atlas, faces, texels_owned, texels_seen, seen_share, faces_unseen,
    views_per_seen_texel.  return_sums: also return (sum_rgb (Ha, Wa, 3), sum_w (Ha, Wa)) fp32, rule 4's accumulators; sums (host
    backend): an (Ha, Wa, 4) fp32 array to accumulate in, overwritten.  backend="device": the same arrays from the GPU (`device`),
    without a host fall-back.  ValueError names a refused argument; an atlas side above 16384 is one."""
    T, depth_tol, min_cos, power, two_sided, z_min, fill = check_args(texels_per_edge, depth_tol, min_cos, power, two_sided, z_min,
                                                                      fill)
    if backend not in ("host", "device"):
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    v32 = np.ascontiguousarray(_np(vertices), dtype=np.float32).reshape(-1, 3)
    f32i = _faces32(faces)
    n, m = len(v32), len(f32i)
    views = list(views)
    _, cols, rows, Ha, Wa = atlas_layout(m, T)
    vc = None
    if vertex_colors is not None:
        vc = np.ascontiguousarray(_np(vertex_colors))
        if vc.dtype != np.uint8 or vc.shape != (n, 3):
            raise ValueError(f"bake_texture: vertex_colors must be uint8 ({n}, 3), got {vc.dtype} {vc.shape}")
    uv = face_uv(m, T)
    if m == 0:
        empty = np.zeros((0, 0, 3), np.uint8)
        return (uv, empty, np.zeros((0, 0, 3), np.float32), np.zeros((0, 0), np.float32)) if return_sums else (uv, empty)
    dev = device if device is not None else "cuda"
    if mesh_depths is None:
        mesh_depths = mesh_depth_maps(v32, f32i, views, dev)
    mesh_depths = list(mesh_depths)
    if len(mesh_depths) != len(views):
        raise ValueError(f"bake_texture: {len(mesh_depths)} mesh_depths for {len(views)} views")
    if backend == "device":
        from . import ops
        if torch.device(dev).type == "cpu" or not torch.cuda.is_available():
            raise RuntimeError('bake_texture(backend="device") needs a GPU: there is no host fall-back for the device path')
        packed = [(np.asarray(_np(w.P), np.float32).reshape(12), view_centre(w.P), _as_device(w.image, torch.float32, dev),
                   _as_device(d, torch.float32, dev)) for w, d in zip(views, mesh_depths)]
        atlas_t, sums_t, count_t = ops.bake_texture(_as_device(v32, torch.float32, dev), _as_device(f32i, torch.int32, dev), packed, T,
                                                    cols, rows, depth_tol, min_cos, power, two_sided, z_min, fill,
                                                    None if vc is None else _as_device(vc, torch.uint8, dev), count=stats is not None)
        atlas = atlas_t.cpu().numpy()
        acc = sums_t.cpu().numpy() if (return_sums or stats is not None) else None
        count = None if count_t is None else count_t.cpu().numpy()
    else:
        acc = np.empty((Ha, Wa, 4), np.float32) if sums is None else sums
        if acc.shape != (Ha, Wa, 4) or acc.dtype != np.float32:
            raise ValueError(f"bake_texture: sums must be fp32 ({Ha}, {Wa}, 4), got {acc.dtype} {acc.shape}")
        count = np.empty((Ha, Wa), np.int32) if stats is not None else None
        bake_host(v32, f32i, T, _host_views(views, mesh_depths), depth_tol, min_cos, power, two_sided, z_min, acc, count)
        atlas = finish_host(acc, f32i, n, T, vc, fill)
    if stats is not None:
        stats.update(bake_stats(acc[..., 3], count, m, T), views=len(views))
    if return_sums:
        return uv, atlas, np.ascontiguousarray(acc[..., :3]), np.ascontiguousarray(acc[..., 3])
    return uv, atlas


def texture_step(vertices, faces, views, params, backend="host", device=None, vertex_colors=None, mesh_depths=None):
    """The scripts' texture step: bake_texture with the arguments of the dict `params` -> (uv, atlas, record) with record = the
    `texture` block of their JSON lines, without `files` (the caller writes them)."""
    params = check_params(params)
    t0 = time.perf_counter()
    st = {}
    uv, atlas = bake_texture(vertices, faces, views, vertex_colors=vertex_colors, mesh_depths=mesh_depths, backend=backend,
                             device=device, stats=st, **params)
    ms = 1e3 * (time.perf_counter() - t0)
    rec = {"texels_per_edge": params["texels_per_edge"], **st, "depth_tol": params["depth_tol"], "min_cos": params["min_cos"],
           "power": params["power"], "ms": ms}
    return uv, atlas, rec
