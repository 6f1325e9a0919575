"""Fusion of the depth maps of many `val` forwards into ONE scene mesh.

A `val` forward returns the mesh that one group of 3-7 views sees, in that group's normalised frame.  A scan has 49 views, a
Tanks and Temples scene hundreds: the whole object comes from one forward per reference view whose rendered depth map
(`sdf_depth` / `render_depth`, z-depth in the reference camera) is integrated into a world-frame truncated-signed-distance
lattice - the standard scene-mesh step of this family of methods (VolRecon, ReTR) - followed by iso-surface extraction.

    vol = FusionVolume((lo, hi, voxel), colors=True)
    for each reference view:  out = model("val", {**inputs, "extract_geometry": False});  vol.integrate([view_from_val(inputs, out)])
    vertices, triangles, colors = vol.extract_mesh()             # world frame: mesh_io.write_ply as it is

backend="device": csrc/fuse.hip (16 views per launch, the lattice point's state in registers across them) and the marching
cubes of csrc/mcubes.hip with the observed-corner rule.  backend="host": the numpy-fp32 mirror of the update sequence written
out in fuse.hip's header comment, operation by operation - the two give equal arrays.  The mesh step always runs on the GPU.

FusionVolume(..., sparse=True) (SparseFusionVolume, csrc/fuse_sparse.hip) keeps that state only in the 8^3-point bricks near the
measured surfaces and returns the same mesh, array for array, for -1 < isovalue < 1 - also on lattices of 2^31 points and more,
where the dense volume's mesh step stops (8 B per point, 20 B with colours, besides).  Only points some view updates with
diff < trunc ever leave tsdf == 1, so only those and their lattice neighbours can carry geometry; bricks are allocated per depth
pixel as a superset of the bricks that hold them, and every view is integrated over every allocated point with the dense
arithmetic.  Allocation has to see all views first: integrate() records the views (device copies of depth and image: 33 MB per
1080p view with colours) and the state is built at first use; a later integrate() rebuilds it.  The class docstring has the limits.

Which pixels go in: filter_views(views, min_consistent) keeps the depths that enough other views agree with - a pixel is lifted,
projected into another view, that view's depth is read there and projected back; it agrees when the round trip ends within a
pixel of where it started and within 1 % of the depth (csrc/depth_filter.hip, 16 sources per launch; consistency_host is its
numpy-fp32 mirror, equal arrays again).  It needs no object masks, unlike the DTU cleaner.

The other product of the same depth maps: fuse_points(views, min_consistent) merges the consistent depths into ONE point cloud,
one point per surface sample (csrc/point_cloud.hip; backend="host" is its numpy-fp32 mirror, equal arrays) - no lattice, no
quantisation to a voxel size; mesh_io.write_ply_points writes it, evaluation.dtu_eval scores it with mode="pcd".

Looking at the fused model: vol.ray_cast(P, (H, W)) casts one ray per pixel of any camera through the lattice (dense or sparse,
csrc/ray_cast.hip; backend="host": ray_cast_host, its numpy-fp32 mirror, equal arrays) and returns the z-depth of the first
front-to-inside crossing - a DepthView depth with dscale 1 - the surface normal and the fused colour there, without a mesh;
view_residual(view, cast) is how far a view's own depth map lies from the model, a quality number that needs no ground truth.
"""
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .marching_cubes import to_host

DepthView = namedtuple("DepthView", "P depth dscale image", defaults=(None,))
DepthView.__doc__ = """One depth map to fuse.  P (3, 4): world -> (x z, y z, z), z in world units, x / y in pixel indices of `depth`;
depth (H, W) fp32 (array or tensor), dscale: depth units -> world units; image (H, W, 3) fp32 or None.  A depth that is 0,
negative, NaN or inf is no measurement."""

_F32_MAX = np.float32(np.finfo(np.float32).max)
SKIP_REASONS = ("behind", "outside", "no_measurement", "beyond_trunc")


def _np(x, dtype=None):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x if dtype is None else np.ascontiguousarray(x, dtype=dtype)


def similarity_scale(S):
    """The scale s of a 4x4 similarity (rotation times uniform scale plus translation)."""
    return float(abs(np.linalg.det(np.asarray(S, dtype=np.float64)[:3, :3])) ** (1.0 / 3.0))


def view_from_val(inputs, outputs, depth="sdf_depth", mask=None):
    """The DepthView of a `val` item's reference camera.  inputs: the item (intrs, c2ws, scale_mat, imgs); outputs: the forward's
    (depth maps on the validation lattice (Hl, Wl), color_fine).  depth: "sdf_depth", "render_depth" or an (Hl, Wl) array;
    mask: bool (Hl, Wl), False = the pixel's depth is dropped.
    With S = scale_mat (normalised -> world, a similarity of scale s): P = K_lat (s (w2c_ref S^-1))[:3, :4], formed in float64 and
    rounded to fp32 once, and dscale = s.  K_lat = diag((Wl-1)/(W-1), (Hl-1)/(H-1), 1) K: the validation lattice is
    linspace(0, W-1, Wl) (datasets.dtu.choose_pixels), not K / level."""
    d = _np(outputs[depth] if isinstance(depth, str) else depth, np.float32)
    if d.ndim != 2:
        raise ValueError("view_from_val: depth (Hl, Wl)")
    Hl, Wl = d.shape
    H, W = (int(v) for v in inputs["imgs"].shape[-2:])
    S = _np(inputs["scale_mat"], np.float64).reshape(4, 4)
    K = _np(inputs["intrs"], np.float64).reshape(-1, 4, 4)[0, :3, :3]
    w2c = np.linalg.inv(_np(inputs["c2ws"], np.float64).reshape(-1, 4, 4)[0])
    s = similarity_scale(S)
    lat = np.diag([(Wl - 1) / (W - 1) if W > 1 else 1.0, (Hl - 1) / (H - 1) if H > 1 else 1.0, 1.0])
    P = ((lat @ K) @ (s * (w2c @ np.linalg.inv(S)))[:3, :4]).astype(np.float32)
    if mask is not None:
        m = _np(mask)
        if m.dtype != np.bool_ or m.shape != d.shape:
            raise ValueError("view_from_val: mask is a bool (Hl, Wl) array")
        d = np.where(m, d, np.float32(0.0))
    image = None
    if "color_fine" in outputs:
        image = _np(outputs["color_fine"], np.float32).reshape(Hl, Wl, 3)
    return DepthView(P, d, s, image)


def bounds_from_scale_mats(scale_mats):
    """World-frame axis-aligned box (lo (3,), hi (3,)) of the union of the groups' normalised [-1, 1]^3 boxes."""
    corners = np.array([[x, y, z, 1.0] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])
    pts = np.concatenate([(corners @ _np(S, np.float64).reshape(4, 4).T)[:, :3] for S in scale_mats])
    return pts.min(0), pts.max(0)


def lattice_axes(lo, hi, voxel):
    """Three fp32 coordinate arrays lo + i voxel (formed in float64) that cover [lo, hi] per axis."""
    lo, hi, voxel = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3), float(voxel)
    if not voxel > 0 or not (hi >= lo).all():
        raise ValueError("FusionVolume: (lo, hi, voxel) with hi >= lo and voxel > 0")
    return [(lo[a] + voxel * np.arange(int(np.ceil((hi[a] - lo[a]) / voxel - 1e-9)) + 1)).astype(np.float32) for a in range(3)]


def integrate_host(tsdf, weight, color, axes, views, trunc, stats=None, points=None, valid=None):
    """The update sequence of fuse.hip's header comment in numpy fp32, one operation per operator in its order, over the whole
    lattice view by view (lattice points are independent, so this is the kernel's per-point loop).  tsdf / weight / color:
    fp32 arrays updated in place; stats (dict, optional): per skip reason the number of (point, view) pairs it dropped, "updated"
    the number of pairs integrated.  points / valid (brick-major state): the three coordinate arrays, broadcastable to the
    state's shape, instead of the axes' outer product, and the bool mask of the entries that are lattice points at all."""
    f32 = np.float32
    px, py, pz = (axes[0][:, None, None], axes[1][None, :, None], axes[2][None, None, :]) if points is None else points
    trunc = f32(trunc)
    for v in views:
        P = np.asarray(v.P, dtype=f32).reshape(12)
        depth = np.asarray(v.depth, dtype=f32)
        H, W = depth.shape
        with np.errstate(all="ignore"):
            cx = ((P[0] * px + P[1] * py) + P[2] * pz) + P[3]
            cy = ((P[4] * px + P[5] * py) + P[6] * pz) + P[7]
            cz = ((P[8] * px + P[9] * py) + P[10] * pz) + P[11]
            front = cz > 0
            rx, ry = np.rint(cx / cz), np.rint(cy / cz)
            inside = front & (rx >= 0) & (rx <= f32(W - 1)) & (ry >= 0) & (ry <= f32(H - 1))
            ix, iy = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
            d = depth[iy, ix] * f32(v.dscale)
            measured = inside & (d > 0) & (d <= _F32_MAX)
            diff = d - cz
            ok = measured & (diff >= -trunc)
            if valid is not None:
                ok = ok & valid
            t = np.minimum(diff / trunc, f32(1.0))
            wn = weight + f32(1.0)
            tsdf[...] = np.where(ok, (tsdf * weight + t) / wn, tsdf)
            if color is not None:
                img = np.asarray(v.image, dtype=f32)[iy, ix]
                color[...] = np.where(ok[..., None], (color * weight[..., None] + img) / wn[..., None], color)
            weight[...] = np.where(ok, wn, weight)
        if stats is not None:
            for key, n in zip(SKIP_REASONS + ("updated",), (~front, front & ~inside, inside & ~measured, measured & ~ok, ok)):
                stats[key] = stats.get(key, 0) + int(n.sum())


# ---- multi-view geometric consistency: which pixels of the depth maps go into the lattice (csrc/depth_filter.hip) ----

# the thresholds of the reference's models/losses/consistency_loss.py:43-52: a round trip through the other view ends within 1 pixel
# of where it started and within 1 % (relative) of the depth it started with
CONSISTENCY_PX = 1.0
CONSISTENCY_REL = 0.01


def _split_P(view):
    """(M (3, 3), t (3,), M^-1) in float64 of a view's P = [M | t]."""
    P = _np(view.P, np.float64).reshape(3, 4)
    return P[:, :3], P[:, 3], np.linalg.inv(P[:, :3])


def _pair(r, s):
    """pair_transforms from two _split_P triples."""
    (Mr, tr, Mr_inv), (Ms, ts, Ms_inv) = r, s
    A_rs, A_sr = Ms @ Mr_inv, Mr @ Ms_inv
    return (A_rs.astype(np.float32), (ts - A_rs @ tr).astype(np.float32), A_sr.astype(np.float32), (tr - A_sr @ ts).astype(np.float32))


def pair_transforms(view_r, view_s):
    """fp32 (A_rs (3, 3), b_rs (3,), A_sr, b_sr): with q = P_r X = (x z, y z, z) of a world point X in view r, A_rs q + b_rs = P_s X,
    and back with A_sr / b_sr.  A_rs = M_s M_r^-1, b_rs = t_s - A_rs t_r for P = [M | t], formed in float64 and rounded once."""
    return _pair(_split_P(view_r), _split_P(view_s))


def consistency_host(views, r, sources, px_thresh=CONSISTENCY_PX, rel_thresh=CONSISTENCY_REL, matches=None):
    """The rule of depth_filter.hip's header comment in numpy fp32, one operation per operator in its order, over the whole map
    of views[r], source by source (pixels are independent, so this is the kernel's per-pixel loop).  sources: indices into
    `views`, tested in this order.  Returns (count (H, W) int32, zsum (H, W) fp32).  matches (list, optional): receives per
    source (s, agree (H, W) bool, sx, sy (H, W) fp32), the pixel's projection into s (meaningful where it agrees)."""
    f32 = np.float32
    ref = views[r]
    depth_r = _np(ref.depth, f32)
    H, W = depth_r.shape
    px = f32(px_thresh)
    px2, rel_thresh = px * px, f32(rel_thresh)
    count, zsum = np.zeros((H, W), np.int32), np.zeros((H, W), f32)
    split_r = _split_P(ref)

    def measured(d):
        return (d > 0) & (d <= _F32_MAX)

    def rows(A, b, x, y, z):
        return [((A[k, 0] * x + A[k, 1] * y) + A[k, 2] * z) + b[k] for k in range(3)]

    with np.errstate(all="ignore"):
        d = depth_r * f32(ref.dscale)
        live = measured(d)
        yf, xf = (a.astype(f32) for a in np.mgrid[:H, :W])
        qx, qy, qz = xf * d, yf * d, d
        for s in sources:
            src = views[s]
            depth_s, dscale_s = _np(src.depth, f32), f32(src.dscale)
            Hs, Ws = depth_s.shape
            A_rs, b_rs, A_sr, b_sr = _pair(split_r, _split_P(src))
            ux, uy, uz = rows(A_rs, b_rs, qx, qy, qz)
            ok = live & (uz > 0)
            sx, sy = ux / uz, uy / uz
            ok &= (sx >= 0) & (sx <= f32(Ws - 1)) & (sy >= 0) & (sy <= f32(Hs - 1))
            x0f, y0f = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0f, sy - y0f
            x0, y0 = np.where(ok, x0f, 0).astype(np.int64), np.where(ok, y0f, 0).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
            d00, d01 = depth_s[y0, x0] * dscale_s, depth_s[y0, x1] * dscale_s
            d10, d11 = depth_s[y1, x0] * dscale_s, depth_s[y1, x1] * dscale_s
            ok &= measured(d00) & measured(d01) & measured(d10) & measured(d11)
            top = d00 + (d01 - d00) * fx
            bot = d10 + (d11 - d10) * fx
            ds = top + (bot - top) * fy
            wx, wy, wz = rows(A_sr, b_sr, sx * ds, sy * ds, ds)
            ok &= wz > 0
            ex, ey = wx / wz - xf, wy / wz - yf
            e2 = ex * ex + ey * ey
            rel = np.abs(wz - d) / d
            ok &= (e2 < px2) & (rel < rel_thresh)
            count += ok
            zsum[...] = np.where(ok, zsum + wz, zsum)
            if matches is not None:
                matches.append((s, ok, sx, sy))
    return count, zsum


def finish_host(view, count, zsum, min_consistent, average=False):
    """The finish step of depth_filter.hip's header comment in numpy fp32: (out depth (H, W) fp32, keep (H, W) bool)."""
    f32 = np.float32
    depth = _np(view.depth, f32)
    with np.errstate(all="ignore"):
        d = depth * f32(view.dscale)
        keep = (d > 0) & (d <= _F32_MAX) & (count >= min_consistent)
        value = ((zsum + d) / (count + 1).astype(f32)) / f32(view.dscale) if average else depth
        return np.where(keep, value, f32(0.0)).astype(f32), keep


def nearest_sources(views, n):
    """Per view the indices of the n other views whose optical axes (the third row of M, normalised, float64) make the smallest
    angle with its own, nearest first; ties go to the lower index."""
    axes = np.stack([_np(v.P, np.float64).reshape(3, 4)[2, :3] for v in views])
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    cos = axes @ axes.T
    out = []
    for i in range(len(views)):
        others = [j for j in range(len(views)) if j != i]
        out.append(sorted(others, key=lambda j: -cos[i, j])[:n])            # sorted() is stable: equal angles stay in index order
    return out


def filter_views(views, min_consistent, px_thresh=CONSISTENCY_PX, rel_thresh=CONSISTENCY_REL, sources=None, average=False,
                 backend="device", device=None, stats=None):
    """The views with the depths dropped (set to 0) that fewer than min_consistent other views agree with: a list of new
    DepthViews with the same P, dscale and image objects.  sources: None = every other view, or per view the list of the indices
    it is tested against (nearest_sources), never itself.  average: a kept depth becomes the mean over the view and its agreeing
    sources.  backend "device" (csrc/depth_filter.hip; every depth map is uploaded once, the new depths stay on `device`) or
    "host" (consistency_host: equal arrays).  stats (dict, optional): receives "measured" and "kept" (a list of pixel counts per
    view) and "count_hist" (per view the histogram of count over its measured pixels, len(its sources) + 1 bins).
    min_consistent = 0 filters nothing: `views` itself is returned."""
    if backend not in ("device", "host"):
        raise ValueError(f"filter_views: backend {backend!r} (device or host)")
    if int(min_consistent) != min_consistent or min_consistent < 0:
        raise ValueError("filter_views: min_consistent is a count >= 0")
    if min_consistent == 0:
        return views
    views = [v if isinstance(v, DepthView) else DepthView(*v) for v in views]
    n = len(views)
    if sources is None:
        sources = [[s for s in range(n) if s != r] for r in range(n)]
    if len(sources) != n:
        raise ValueError("filter_views: sources lists the source views of every view")
    for r, src in enumerate(sources):
        if any(int(s) != s or not 0 <= s < n or s == r for s in src):
            raise ValueError(f"filter_views: sources[{r}] holds indices of other views")
    on_device = backend == "device"
    if on_device:
        if not torch.cuda.is_available():
            raise RuntimeError("filter_views(backend='device') needs a GPU (the SuRF hot path has no CPU fallback)")
        dev = torch.device("cuda" if device is None else device)
        depths = [v.depth.to(dev, torch.float32).contiguous() if torch.is_tensor(v.depth) else
                  torch.from_numpy(np.ascontiguousarray(v.depth, dtype=np.float32)).to(dev) for v in views]
        split = [_split_P(v) for v in views]
    out, tallies = [], []
    for r, view in enumerate(views):
        if on_device:
            ref = (depths[r], float(view.dscale))
            count = torch.zeros(depths[r].shape, dtype=torch.int32, device=dev)
            zsum = torch.zeros(depths[r].shape, dtype=torch.float32, device=dev)
            for c in range(0, len(sources[r]), ops.FUSE_MAX_VIEWS):
                ops.depth_consistency(ref, [(_pair(split[r], split[s]), depths[s], float(views[s].dscale))
                                            for s in sources[r][c:c + ops.FUSE_MAX_VIEWS]], count, zsum, px_thresh, rel_thresh)
            depth, keep = ops.depth_consistency_finish(ref, count, zsum, min_consistent, average)
            if stats is not None:                              # counted on the device, read back once after the last view
                is_measured = ops.depth_consistency_finish(ref, count, zsum, 0)[1].bool()
                tallies.append(torch.cat([is_measured.sum().reshape(1), keep.sum().reshape(1),
                                          torch.bincount(count[is_measured].long(), minlength=len(sources[r]) + 1)]))
        else:
            count, zsum = consistency_host(views, r, sources[r], px_thresh, rel_thresh)
            depth, keep = finish_host(view, count, zsum, min_consistent, average)
            if stats is not None:
                is_measured = finish_host(view, count, zsum, 0)[1]
                tallies.append(np.concatenate([[is_measured.sum(), keep.sum()],
                                               np.bincount(count[is_measured], minlength=len(sources[r]) + 1)]))
        out.append(view._replace(depth=depth))
    if stats is not None:
        if on_device and tallies:
            sizes = [len(t) for t in tallies]
            tallies = np.split(torch.cat(tallies).cpu().numpy(), np.cumsum(sizes)[:-1])
        stats["measured"] = [int(t[0]) for t in tallies]
        stats["kept"] = [int(t[1]) for t in tallies]
        stats["count_hist"] = [np.asarray(t[2:], dtype=np.int64) for t in tallies]
    return out


# ---- fused point clouds: the consistent depths of all views merged into one cloud (csrc/point_cloud.hip) ----

PointCloud = namedtuple("PointCloud", "points colors origin")
PointCloud.__doc__ = """A fused cloud: points (N, 3) fp32 in the world frame, colors (N, 3) uint8 or None, origin (N, 2) int32 =
(view index, flat row-major pixel index) of the pixel a point was lifted from; ordered by view, then pixel."""


def lift_transform(view):
    """The 12 fp32 values (M^-1 row-major, then c = -M^-1 t) of a view's P = [M | t]: X = M^-1 (x z, y z, z) + c.  Formed in
    float64 and rounded once, so that no fp32 subtraction of the large t takes place."""
    M, t, M_inv = _split_P(view)
    return np.concatenate([M_inv.reshape(9), -(M_inv @ t)]).astype(np.float32)


def lift_host(lift, x, y, z):
    """The lift of point_cloud.hip's header comment in numpy fp32: pixels (x, y) (integer arrays) at depth z (fp32, world units)
    -> points (n, 3) fp32."""
    f32 = np.float32
    lift, z = np.asarray(lift, f32), np.asarray(z, f32)
    qx, qy = np.asarray(x).astype(f32) * z, np.asarray(y).astype(f32) * z
    return np.stack([((lift[3 * k] * qx + lift[3 * k + 1] * qy) + lift[3 * k + 2] * z) + lift[9 + k] for k in range(3)], axis=-1)


def quantise_colors_host(c):
    """fp32 colours -> uint8 as fuse_vertex_colors_kernel converts: q = c * 256; q = fmin(fmax(q, 0), 255); (uint8)q."""
    with np.errstate(all="ignore"):
        q = np.asarray(c, np.float32) * np.float32(256.0)
        return np.fmin(np.fmax(q, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


def fuse_points(views, min_consistent, px_thresh=CONSISTENCY_PX, rel_thresh=CONSISTENCY_REL, sources=None, average=True,
                backend="device", device=None, stats=None):
    """The depth maps of `views` merged into one PointCloud with one point per surface sample (the rule is written out in
    csrc/point_cloud.hip's header comment).  Views are visited in index order; a pixel that is measured, not yet used and that at
    least min_consistent of its sources agree with (filter_views' test) is emitted, and the pixel it lands on in every agreeing
    source is marked used: it may still support other views, but is not emitted again.  min_consistent = 0 emits every unused
    measured pixel.  sources: None = every other view, or per view the list of the indices it is tested against
    (nearest_sources), never itself.  average: a point is lifted at the mean depth over the view and its agreeing sources.
    Colours are image[y, x] as uint8 when the views carry images (all of them or none).  backend "device"
    (csrc/point_cloud.hip; the arrays are copied to the host once, at the end) or "host" (numpy fp32: equal arrays).
    stats (dict, optional): receives per view "candidates" (measured, unused pixels), "emitted" (points) and "marked" (pixels of
    other views it newly marked used), and "used": the final used maps, (H, W) uint8 arrays."""
    if backend not in ("device", "host"):
        raise ValueError(f"fuse_points: backend {backend!r} (device or host)")
    if int(min_consistent) != min_consistent or min_consistent < 0:
        raise ValueError("fuse_points: min_consistent is a count >= 0")
    views = [v if isinstance(v, DepthView) else DepthView(*v) for v in views]
    n = len(views)
    if sources is None:
        sources = [[s for s in range(n) if s != r] for r in range(n)]
    if len(sources) != n:
        raise ValueError("fuse_points: sources lists the source views of every view")
    for r, src in enumerate(sources):
        if any(int(s) != s or not 0 <= s < n or s == r for s in src):
            raise ValueError(f"fuse_points: sources[{r}] holds indices of other views")
    with_colors = n > 0 and views[0].image is not None
    if any((v.image is not None) != with_colors for v in views):
        raise ValueError("fuse_points: either every view carries an image or none does")
    for r, v in enumerate(views):
        if len(v.depth.shape) != 2 or (with_colors and tuple(v.image.shape) != tuple(v.depth.shape) + (3,)):
            raise ValueError(f"fuse_points: views[{r}] holds depth (H, W) and image (H, W, 3)")
    min_consistent, average = int(min_consistent), bool(average)
    lifts = [lift_transform(v) for v in views]
    points, colors, origin, tallies = [], [], [], []
    if backend == "device":
        if not torch.cuda.is_available():
            raise RuntimeError("fuse_points(backend='device') needs a GPU (the SuRF hot path has no CPU fallback)")
        dev = torch.device("cuda" if device is None else device)

        def up(x):
            return x.to(dev, torch.float32).contiguous() if torch.is_tensor(x) else \
                torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        depths = [up(v.depth) for v in views]
        used = [torch.zeros(d.shape, dtype=torch.uint8, device=dev) for d in depths]
        split = [_split_P(v) for v in views]
        for r, view in enumerate(views):
            cand = ops.points_candidates(depths[r], used[r])
            ref = (cand, float(view.dscale))
            count = torch.zeros(cand.shape, dtype=torch.int32, device=dev)
            zsum = torch.zeros(cand.shape, dtype=torch.float32, device=dev)
            chunks = [[(_pair(split[r], split[s]), depths[s], float(views[s].dscale)) for s in sources[r][c:c + ops.FUSE_MAX_VIEWS]]
                      for c in range(0, len(sources[r]), ops.FUSE_MAX_VIEWS)]
            for chunk in chunks:
                ops.depth_consistency(ref, chunk, count, zsum, px_thresh, rel_thresh)
            keep = ops.depth_consistency_finish(ref, count, zsum, min_consistent)[1]
            if stats is not None:
                targets = sorted(set(sources[r]))
                before = sum(used[s].sum() for s in targets) if targets else torch.zeros((), dtype=torch.int64, device=dev)
            for c, chunk in enumerate(chunks):
                ops.points_mark(ref, keep, chunk, [used[s] for s in sources[r][c * ops.FUSE_MAX_VIEWS:(c + 1) * ops.FUSE_MAX_VIEWS]],
                                px_thresh, rel_thresh)
            kept = torch.nonzero(keep.reshape(-1)).reshape(-1)                    # ascending: the cloud's order within a view
            p, c, o = ops.points_lift(ref, count, zsum, kept, lifts[r], r, average, up(view.image) if with_colors else None)
            points.append(p)
            colors.append(c)
            origin.append(o)
            if stats is not None:
                after = sum(used[s].sum() for s in targets) if targets else before
                n_cand = ops.depth_consistency_finish(ref, count, zsum, 0)[1].sum()
                tallies.append(torch.stack([n_cand, after - before]))
        if n:
            points, origin = torch.cat(points).cpu().numpy(), torch.cat(origin).cpu().numpy()
            colors = torch.cat(colors).cpu().numpy() if with_colors else None
        if stats is not None:
            tallies = [t.cpu().numpy() for t in tallies]
            stats["used"] = [u.cpu().numpy() for u in used]
    else:
        f32 = np.float32
        host = [view._replace(depth=_np(view.depth, f32)) for view in views]
        used = [np.zeros(v.depth.shape, np.uint8) for v in host]
        for r, view in enumerate(host):
            cand = view._replace(depth=np.where(used[r] != 0, f32(0.0), view.depth))
            masked = host[:r] + [cand] + host[r + 1:]                            # only the reference is masked: sources are read as they are
            matches = []
            count, zsum = consistency_host(masked, r, sources[r], px_thresh, rel_thresh, matches)
            keep = finish_host(cand, count, zsum, min_consistent)[1]
            before = sum(int(u.sum()) for u in used)
            for s, agree, sx, sy in matches:
                hit = keep & agree
                used[s][np.rint(sy[hit]).astype(np.int64), np.rint(sx[hit]).astype(np.int64)] = 1
            H, W = cand.depth.shape
            kept = np.flatnonzero(keep)
            y, x = kept // W, kept % W
            with np.errstate(all="ignore"):
                d = cand.depth * f32(view.dscale)
                z = ((zsum + d) / (count + 1).astype(f32) if average else d).astype(f32)
            points.append(lift_host(lifts[r], x, y, z[y, x]))
            if with_colors:
                colors.append(quantise_colors_host(_np(view.image, f32)[y, x]))
            origin.append(np.stack([np.full(len(kept), r), kept], axis=-1).astype(np.int32))
            tallies.append((int(finish_host(cand, count, zsum, 0)[1].sum()), sum(int(u.sum()) for u in used) - before))
        if n:
            points, origin = np.concatenate(points).astype(f32), np.concatenate(origin)
            colors = np.concatenate(colors) if with_colors else None
        if stats is not None:
            stats["used"] = used
    if not n:
        points, colors, origin = np.zeros((0, 3), np.float32), None, np.zeros((0, 2), np.int32)
    if stats is not None:
        stats["candidates"] = [int(t[0]) for t in tallies]
        stats["marked"] = [int(t[1]) for t in tallies]
        stats["emitted"] = [int(c) for c in np.bincount(origin[:, 0], minlength=n)]
    return PointCloud(points, colors, origin)


# ---- ray casting of the fused state (csrc/ray_cast.hip): depth, normal and colour of the model from any camera ----

RAY_REFINE_EVALS = 3             # evaluations of the interpolant that refine a root inside its cell (ray_cast.hip's constant)


def uniform_lattice(axes):
    """(lo (3,) float64, voxel) of coordinate arrays that are one uniform lattice lo + voxel * index to fp32 rounding: voxel is the
    mean step of the longest axis, and every value lies within 2 ulp (of its axis' largest magnitude) of a[0] + voxel * i - one for
    the rounding of the values themselves, one for the step taken from another axis.  ValueError naming the reason otherwise."""
    axes = [np.asarray(a, np.float64).reshape(-1) for a in axes]
    if any(len(a) < 2 for a in axes):
        raise ValueError("ray_cast: every axis needs two lattice points (a lattice without cells has nothing to cast)")
    longest = max(axes, key=len)
    voxel = float(longest[-1] - longest[0]) / (len(longest) - 1)
    if not voxel > 0:
        raise ValueError("ray_cast: the lattice axes must increase")
    for name, a in zip("xyz", axes):
        tol = 2.0 * float(np.spacing(np.float32(np.abs(a).max())))
        dev = float(np.abs(a - (a[0] + voxel * np.arange(len(a)))).max())
        if not dev <= tol:
            raise ValueError(f"ray_cast needs a uniform lattice: axis {name} departs by {dev:.3g} from a uniform step of {voxel:.6g} "
                             f"(fp32 rounding allows {tol:.3g})")
    return np.array([a[0] for a in axes]), voxel


def ray_lift(P, lo, voxel):
    """The 12 fp32 values of ray_cast.hip's camera, in lattice-index units: L (9, row-major) = M^-1 / voxel, then
    c = (-M^-1 t - lo) / voxel of P = [M | t], formed in float64 and rounded once.  Pixel (x, y) at z-depth z is the lattice-index
    point c + z L (x, y, 1)."""
    P = _np(P, np.float64)
    if P.size != 12:
        raise ValueError("ray_cast: P (3, 4)")
    P = P.reshape(3, 4)
    M_inv = np.linalg.inv(P[:, :3])
    lo, voxel = np.asarray(lo, np.float64).reshape(3), float(voxel)
    return np.concatenate([(M_inv / voxel).reshape(9), (-(M_inv @ P[:, 3]) - lo) / voxel]).astype(np.float32)


def _lerp(a, b, u):
    return (np.float32(1.0) - u) * a + u * b


def _clamp01(v):
    return np.minimum(np.maximum(v, np.float32(0.0)), np.float32(1.0))


def _trilerp(v, ux, uy, uz):
    """ray_cast.hip's f: corner index dx * 4 + dy * 2 + dz, lerp over x, then y, then z."""
    c00, c10, c01, c11 = _lerp(v[0], v[4], ux), _lerp(v[2], v[6], ux), _lerp(v[1], v[5], ux), _lerp(v[3], v[7], ux)
    return _lerp(_lerp(c00, c10, uy), _lerp(c01, c11, uy), uz)


def ray_cast_host(tsdf, weight, color, shape, lift, hw, z_min=0.0, level=0.0, normals=True, table=None):
    """The rule of ray_cast.hip's header comment in numpy fp32, one operation per operator in its order, vectorised over the rays
    with a masked loop over the crossings (rays are independent, so this is the kernel's per-ray loop).  Dense state
    (table None: tsdf / weight (nx, ny, nz), color (nx, ny, nz, 3) or None) or brick-major state (table: the brick table, tsdf /
    weight (n_slots * 512,), color (n_slots * 512, 3) or None) of the uniform lattice `shape`; lift: ray_lift(); level = -isovalue.
    Returns (depth (H, W), normal (H, W, 3) or None, color (H, W, 3) or None) fp32."""
    f32 = np.float32
    shape = tuple(int(v) for v in shape)
    nx, ny, nz = shape
    H, W = (int(v) for v in hw)
    N = H * W
    L = np.asarray(lift, f32).reshape(12)
    level, inf = f32(level), f32(np.inf)
    tsdf_f, weight_f = np.asarray(tsdf, f32).reshape(-1), np.asarray(weight, f32).reshape(-1)
    color_f = None if color is None else np.asarray(color, f32).reshape(-1, 3)
    out_d, out_n, out_c = np.zeros(N, f32), np.zeros((N, 3), f32), np.zeros((N, 3), f32)

    def result():
        return (out_d.reshape(H, W), out_n.reshape(H, W, 3) if normals else None, None if color is None else out_c.reshape(H, W, 3))

    if N == 0 or min(shape) < 2 or tsdf_f.size == 0:
        return result()
    if table is not None:
        table = np.asarray(table).reshape(-1)
        nbp = (max(shape) + 7) // 8

    def corners(ic):
        """(positions of the eight corners in the flat state, all allocated)"""
        pos, ok = [], np.ones(len(ic[0]), bool)
        for k in range(8):
            x, y, z = ic[0] + (k >> 2), ic[1] + ((k >> 1) & 1), ic[2] + (k & 1)
            if table is None:
                pos.append((x * ny + y) * nz + z)
            else:
                s = table[((x >> 3) * nbp + (y >> 3)) * nbp + (z >> 3)].astype(np.int64)
                ok &= s >= 0
                pos.append(np.maximum(s, 0) * 512 + (((x & 7) << 6) | ((y & 7) << 3) | (z & 7)))
        return pos, ok

    yy, xx = np.mgrid[:H, :W]
    xf, yf = xx.reshape(-1).astype(f32), yy.reshape(-1).astype(f32)
    with np.errstate(all="ignore"):
        r = [(L[3 * a] * xf + L[3 * a + 1] * yf) + L[3 * a + 2] for a in range(3)]
        c = [L[9 + a] for a in range(3)]
        m = [f32(shape[a] - 1) for a in range(3)]
        # ---- clip to the box of cells and to z > z_min ----
        te, tx, live = np.full(N, f32(z_min)), np.full(N, inf), np.ones(N, bool)
        for a in range(3):
            moves = r[a] != 0
            t0, t1 = (f32(0.0) - c[a]) / r[a], (m[a] - c[a]) / r[a]
            nr, fr = np.where(t0 < t1, t0, t1), np.where(t0 < t1, t1, t0)
            te = np.where(moves & (nr > te), nr, te)
            tx = np.where(moves & (fr < tx), fr, tx)
            live &= moves | ((c[a] >= 0) & (c[a] <= m[a]))
        live &= te < tx
        idx = np.flatnonzero(live)                         # the rays still walking, and their state
        r = [ra[idx] for ra in r]
        t_in = te[idx]
        ic, u = [], []
        for a in range(3):
            p = c[a] + t_in * r[a]
            fl = np.minimum(np.maximum(np.floor(p), f32(0.0)), m[a] - f32(1.0))
            ic.append(fl.astype(np.int64))
            u.append(_clamp01(p - fl))
        for _ in range(nx + ny + nz):
            if len(idx) == 0:
                break
            # ---- the crossing that ends this cell, from the integer plane indices ----
            tc = [np.where(r[a] != 0, (np.where(r[a] > 0, ic[a] + 1, ic[a]).astype(f32) - c[a]) / r[a], inf) for a in range(3)]
            axis, to = np.zeros(len(idx), np.int64), tc[0]
            for a in (1, 2):
                sooner = tc[a] < to
                axis, to = np.where(sooner, a, axis), np.where(sooner, tc[a], to)
            keep = np.abs(to) <= _F32_MAX                  # no finite crossing: the walk ends
            if not keep.all():
                idx, t_in, axis, to = idx[keep], t_in[keep], axis[keep], to[keep]
                r, ic, u = [v[keep] for v in r], [v[keep] for v in ic], [v[keep] for v in u]
            w, step = [], []
            for a in range(3):
                p = c[a] + to * r[a]
                w.append(np.where(axis == a, np.where(r[a] > 0, f32(1.0), f32(0.0)), _clamp01(p - ic[a].astype(f32))))
                step.append(np.where(axis == a, np.where(r[a] > 0, 1, -1), 0))
            # ---- does the cell count?  all eight corners observed ----
            pos, counted = corners(ic)
            for k in range(8):
                counted &= weight_f[pos[k]] > 0
            v = [tsdf_f[pos[k]] - level for k in range(8)]
            f_in, f_out = _trilerp(v, *u), _trilerp(v, *w)
            hit = counted & (f_in > 0) & (f_out <= 0)
            if hit.any():
                h = np.flatnonzero(hit)
                ta, fa, tb, fb = t_in[h], f_in[h], to[h], f_out[h]
                vh, rh, fi = [vk[h] for vk in v], [ra[h] for ra in r], [ia[h].astype(f32) for ia in ic]

                def local(t):
                    return [_clamp01((c[a] + t * rh[a]) - fi[a]) for a in range(3)]
                for _e in range(RAY_REFINE_EVALS):
                    t = ta + (tb - ta) * (fa / (fa - fb))
                    g = _trilerp(vh, *local(t))
                    front = g > 0
                    ta, fa, tb, fb = np.where(front, t, ta), np.where(front, g, fa), np.where(front, tb, t), np.where(front, fb, g)
                z = ta + (tb - ta) * (fa / (fa - fb))
                ux, uy, uz = local(z)
                out_d[idx[h]] = z
                gx = _lerp(_lerp(vh[4] - vh[0], vh[6] - vh[2], uy), _lerp(vh[5] - vh[1], vh[7] - vh[3], uy), uz)
                gy = _lerp(_lerp(vh[2] - vh[0], vh[6] - vh[4], ux), _lerp(vh[3] - vh[1], vh[7] - vh[5], ux), uz)
                gz = _lerp(_lerp(vh[1] - vh[0], vh[5] - vh[4], ux), _lerp(vh[3] - vh[2], vh[7] - vh[6], ux), uy)
                length = np.sqrt((gx * gx + gy * gy) + gz * gz)
                out_n[idx[h]] = np.where((length > 0)[:, None], np.stack([gx / length, gy / length, gz / length], axis=-1), f32(0.0))
                if color_f is not None:
                    cv = [color_f[pos[k][h]] for k in range(8)]
                    out_c[idx[h]] = _trilerp(cv, ux[:, None], uy[:, None], uz[:, None])
            # ---- step through the crossed face ----
            keep = ~hit
            for a in range(3):
                ic[a] = ic[a] + step[a]
                keep &= (ic[a] >= 0) & (ic[a] <= shape[a] - 2)
                u[a] = np.where(axis == a, f32(1.0) - w[a], w[a])
            idx, t_in = idx[keep], to[keep]
            r, ic, u = [v_[keep] for v_ in r], [v_[keep] for v_ in ic], [v_[keep] for v_ in u]
    return result()


def view_residual(view, cast, voxel=None):
    """How far a view's own depth map lies from the fused model seen from the same camera.  cast: FusionVolume.ray_cast(view.P,
    view.depth.shape) (or its depth array, then with voxel=).  Over the view's measured pixels: "measured" (their number), "hit"
    (those the model also hits), "hit_share" = hit / measured, and over the hit ones the median and 90th percentile of
    |d_view * dscale - d_model| in world units ("median", "p90") and in lattice steps ("median_voxels", "p90_voxels"; None without a
    voxel size); "residuals": the world-unit values themselves (fp64), for pooling over views.  No hit pixel: the four are None."""
    model = cast["depth"] if isinstance(cast, dict) else cast
    if voxel is None and isinstance(cast, dict):
        voxel = cast.get("voxel")
    model = _np(model, np.float64)
    with np.errstate(all="ignore"):
        d = (_np(view.depth, np.float32) * np.float32(view.dscale)).astype(np.float64)
    if model.shape != d.shape:
        raise ValueError("view_residual: the cast has the size of the view's depth map")
    measured = (d > 0) & (d <= float(_F32_MAX))
    both = measured & (model > 0)
    res = np.abs(d[both] - model[both])
    out = {"measured": int(measured.sum()), "hit": int(both.sum()), "hit_share": float(both.sum()) / max(int(measured.sum()), 1),
           "residuals": res}
    out.update(pooled_residual(res, voxel))
    return out


def pooled_residual(residuals, voxel=None):
    """median / p90 (world units) and median_voxels / p90_voxels of world-unit residuals (view_residual's, or several views'
    concatenated)."""
    if len(residuals) == 0:
        return {"median": None, "p90": None, "median_voxels": None, "p90_voxels": None}
    med, p90 = float(np.median(residuals)), float(np.percentile(residuals, 90))
    return {"median": med, "p90": p90, "median_voxels": None if voxel is None else med / float(voxel),
            "p90_voxels": None if voxel is None else p90 / float(voxel)}


class FusionVolume:
    """A dense world-frame TSDF lattice that depth views are integrated into.

    grid: three coordinate arrays (any spacing), or (lo, hi, voxel).  trunc: truncation distance in world units (None: 4 x the
    largest axis step).  colors: also fuse the views' images.  backend "device" (HIP, state on `device`) or "host" (numpy fp32,
    equal arrays).  integrate() may be called any number of times with any number of views.
    sparse=True gives a SparseFusionVolume: the same mesh from state kept only near the measured surfaces."""

    def __new__(cls, *args, sparse=False, **kwargs):
        sparse = sparse or (len(args) > 5 and args[5])
        return object.__new__(SparseFusionVolume if sparse and cls is FusionVolume else cls)

    def __init__(self, grid, trunc=None, colors=False, backend="device", device=None, sparse=False):
        self._init_lattice(grid, trunc, backend, device)
        if backend == "device":
            self.tsdf = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
            self.weight = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
            self.color = torch.zeros(self.shape + (3,), dtype=torch.float32, device=self.device) if colors else None
        else:
            self.tsdf, self.weight = np.zeros(self.shape, np.float32), np.zeros(self.shape, np.float32)
            self.color = np.zeros(self.shape + (3,), np.float32) if colors else None

    def _init_lattice(self, grid, trunc, backend, device):
        if backend not in ("device", "host"):
            raise ValueError(f"FusionVolume: backend {backend!r} (device or host)")
        if len(grid) != 3:
            raise ValueError("FusionVolume: three axis arrays or (lo, hi, voxel)")
        by_voxel = isinstance(grid[2], (int, float, np.integer, np.floating))
        axes = lattice_axes(*grid) if by_voxel else [_np(a, np.float32).reshape(-1) for a in grid]
        if any(len(a) < 1 for a in axes):
            raise ValueError("FusionVolume: an axis without lattice points")
        steps = [float(np.abs(np.diff(a.astype(np.float64))).max()) for a in axes if len(a) > 1]
        if trunc is None:
            if not steps:
                raise ValueError("FusionVolume: trunc=None needs an axis with two lattice points")
            trunc = 4.0 * max(steps)
        self.trunc = float(np.float32(trunc))
        if not (self.trunc > 0 and np.isfinite(self.trunc)):
            raise ValueError("FusionVolume: trunc > 0")
        self.backend, self.shape, self.n_views = backend, tuple(len(a) for a in axes), 0
        self.axes_host = axes
        self._by_voxel = (np.asarray(grid[0], np.float64).reshape(3), float(grid[2])) if by_voxel else None     # ray_cast's (lo, voxel)
        if backend == "device":
            if not torch.cuda.is_available():
                raise RuntimeError("FusionVolume(backend='device') needs a GPU (the SuRF hot path has no CPU fallback)")
            self.device = torch.device("cuda" if device is None else device)
            self.axes = [torch.from_numpy(a).to(self.device) for a in axes]
        else:
            self.device = None if device is None else torch.device(device)
            self.axes = axes

    def _dev(self, x):
        if torch.is_tensor(x):
            return x.to(self.device, torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)

    def integrate(self, views, stats=None):
        """Fuses `views` (DepthViews) in order; on the device 16 per launch.  stats: integrate_host's counters (host backend)."""
        views = [v if isinstance(v, DepthView) else DepthView(*v) for v in views]
        if self.color is not None and any(v.image is None for v in views):
            raise ValueError("FusionVolume.integrate: colours are fused but a view has no image")
        if self.backend == "host":
            host = [DepthView(_np(v.P, np.float32), _np(v.depth, np.float32), float(v.dscale),
                              None if v.image is None else _np(v.image, np.float32)) for v in views]
            integrate_host(self.tsdf, self.weight, self.color, self.axes, host, self.trunc, stats)
        else:
            if stats is not None:
                raise ValueError("FusionVolume.integrate: stats are counted by the host backend")
            for s in range(0, len(views), ops.FUSE_MAX_VIEWS):
                batch = [(_np(v.P, np.float32), self._dev(v.depth), float(v.dscale),
                          None if self.color is None else self._dev(v.image)) for v in views[s:s + ops.FUSE_MAX_VIEWS]]
                ops.fuse_integrate(self.tsdf, self.weight, self.color, self.axes, batch, self.trunc)
        self.n_views += len(views)

    def observed_share(self):
        """Share of the lattice points that at least one view updated."""
        return float((self.weight > 0).sum()) / float(np.prod(self.shape))

    def extract_mesh(self, isovalue=0.0, simplify_cell=None, smooth=None, denoise=None):
        """(vertices (V, 3) float64 in the world frame, triangles (F, 3) int64[, colors (V, 3) uint8 when colours are fused]) as
        numpy arrays: marching cubes at u = -tsdf = isovalue over the cells whose eight corners were observed, one copy to the
        host.  Runs on the GPU whatever the backend (the host backend's state is uploaded).
        simplify_cell (world units): the mesh is simplified before it is returned - mesh_simplify.simplify_mesh of exactly the
        arrays that simplify_cell=None returns, by the volume's backend (on the device the full mesh never visits the host);
        positions are then fp32 values.
        smooth (a dict of mesh_smooth.smooth_mesh's iterations, lam, mu, pin_boundary, max_move; {} for the defaults): the mesh is
        smoothed first - mesh_smooth.smooth_mesh of exactly the arrays that smooth=None returns, by the volume's backend, before
        simplify_cell is applied; positions are then fp32 values.
        denoise (a dict of mesh_denoise.denoise_mesh's normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary,
        max_move; {} for the defaults): the mesh is denoised before anything else - mesh_denoise.denoise_mesh of exactly the arrays
        that denoise=None returns, by the volume's backend; smooth and simplify_cell then apply to the denoised mesh."""
        if self.backend == "device":
            dev, tsdf, weight, color, axes = self.device, self.tsdf, self.weight, self.color, self.axes
        else:
            if not torch.cuda.is_available():
                raise RuntimeError("FusionVolume.extract_mesh: marching cubes runs on the GPU (the SuRF hot path has no CPU fallback)")
            dev = torch.device("cuda") if self.device is None else self.device
            tsdf, weight = torch.from_numpy(self.tsdf).to(dev), torch.from_numpy(self.weight).to(dev)
            color = None if self.color is None else torch.from_numpy(self.color).to(dev)
            axes = [torch.from_numpy(a).to(dev) for a in self.axes]
        v, t = ops.marching_cubes(ops.fuse_lattice(tsdf, weight), float(isovalue), observed_only=True)
        c = None if color is None else ops.fuse_vertex_colors(v, color)
        return self._finished(v, t, c, axes, simplify_cell, smooth, denoise)

    def lattice(self):
        """(lo (3,) float64, voxel) of a uniform lattice: the (lo, hi, voxel) it was built from, or what its coordinate arrays
        follow to fp32 rounding (uniform_lattice; ValueError naming the reason otherwise)."""
        if self._by_voxel is not None and min(self.shape) >= 2:
            return self._by_voxel
        return uniform_lattice(self.axes_host)

    def _ray_state(self):
        """(tsdf, weight, color, table or None, lattice has state at all) for ray_cast."""
        return self.tsdf, self.weight, self.color, None, True

    def ray_cast(self, P, hw, z_min=0.0, isovalue=0.0, normals=True, return_tensors=False):
        """The fused model seen from the camera P (3, 4) (DepthView's: world -> (x z, y z, z)) at an (H, W) image:
        {"depth": (H, W) fp32 z-depth in world units at the first front-to-inside crossing of u = -tsdf = isovalue over the cells
        whose eight corners were observed, 0 where the ray meets none - a DepthView depth with dscale 1; "normal": (H, W, 3) unit
        normals in the world frame pointing into free space (0 without a hit; None with normals=False); "color": (H, W, 3) fp32 in
        image units when colours are fused, else None; "voxel": the lattice step}.  The rule is written out in csrc/ray_cast.hip's
        header comment; backend "host" is its numpy-fp32 mirror (equal arrays), and a sparse volume returns the dense volume's
        arrays.  z_min >= 0: rays start at that z-depth.  Needs a uniform lattice (lattice()).  numpy arrays unless
        return_tensors (device backend: device tensors, no host copy)."""
        P = _np(P, np.float64)
        if P.shape not in ((3, 4), (12,)) or not np.isfinite(P).all():
            raise ValueError("FusionVolume.ray_cast: P is a finite (3, 4) matrix")
        try:
            H, W = (int(v) for v in hw)
            ok = len(hw) == 2 and H >= 1 and W >= 1 and all(int(v) == v for v in hw)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("FusionVolume.ray_cast: hw = (H, W), two positive integers")
        if not -1.0 < float(isovalue) < 1.0:
            raise ValueError("FusionVolume.ray_cast: -1 < isovalue < 1")
        if not (0.0 <= float(z_min) <= float(_F32_MAX)):
            raise ValueError("FusionVolume.ray_cast: z_min >= 0")
        lo, voxel = self.lattice()
        P = P.reshape(3, 4)
        if not abs(np.linalg.det(P[:, :3])) > 0:
            raise ValueError("FusionVolume.ray_cast: P = [M | t] with an invertible M")
        lift, level = ray_lift(P, lo, voxel), -float(isovalue)
        tsdf, weight, color, table, any_state = self._ray_state()
        if self.backend == "device":
            if not any_state:
                d, n, c = (torch.zeros((H, W) + tail, dtype=torch.float32, device=self.device) for tail in ((), (3,), (3,)))
                d, n, c = d, (n if normals else None), (c if self.color is not None else None)
            elif table is None:
                d, n, c = ops.fuse_ray_cast(tsdf, weight, color, lift, (H, W), z_min, level, normals)
            else:
                d, n, c = ops.fuse_ray_cast_bricks(tsdf, weight, color, table, self.shape, lift, (H, W), z_min, level, normals)
            if not return_tensors:
                flat = to_host(torch.cat([x.reshape(-1) for x in (d, n, c) if x is not None])).numpy()
                parts = np.split(flat, np.cumsum([x.numel() for x in (d, n, c) if x is not None])[:-1])
                it = iter(parts)
                d, n, c = (None if x is None else next(it).reshape(tuple(x.shape)) for x in (d, n, c))
        else:
            d, n, c = ray_cast_host(tsdf, weight, color, self.shape, lift, (H, W), z_min, level, normals, table=table)
            if return_tensors:
                d, n, c = (None if x is None else torch.from_numpy(x) for x in (d, n, c))
        return {"depth": d, "normal": n, "color": c, "voxel": voxel}

    @staticmethod
    def _world(v, axes):
        """Device vertices in lattice-index units -> world: linear along the lattice edge, in float64 (exact for a uniform axis up
        to its fp32 values)."""
        cols = []
        for a in range(3):
            ax = axes[a].double()
            lo = v[:, a].floor().long().clamp_(0, max(len(ax) - 2, 0))
            hi = (lo + 1).clamp_(max=len(ax) - 1)
            cols.append(ax[lo] + (ax[hi] - ax[lo]) * (v[:, a] - lo.double()))
        return torch.stack(cols, dim=1) if len(v) else v

    def _finished(self, v, t, c, axes, cell, smooth, denoise=None):
        """extract_mesh's arrays of the device mesh (v in lattice-index units), denoised if `denoise` is given, smoothed if
        `smooth` is, then simplified if `cell` is.  Device backend: all on the device, one copy of the final mesh; host backend:
        the numpy paths on the full mesh's host arrays."""
        if cell is None and smooth is None and denoise is None:
            return self._mesh_to_host(v, t, c, axes)
        from . import mesh_denoise
        from .mesh_simplify import simplify_mesh
        from .mesh_smooth import check_params, smooth_mesh
        params = None if smooth is None else check_params(smooth)
        dparams = None if denoise is None else mesh_denoise.check_params(denoise)
        if self.backend == "device":
            out = [self._world(v, axes), t] + ([] if c is None else [c])
            if dparams is not None and len(v):
                out[0] = mesh_denoise.denoise_mesh(out[0], t, backend="device", device=v.device, return_tensors=True, **dparams)[0]
            if params is not None and len(v):
                out[0] = smooth_mesh(out[0], t, backend="device", device=v.device, return_tensors=True, **params)[0]
            if cell is not None:
                out = simplify_mesh(out[0], t, cell, colors=c, backend="device", device=v.device, return_tensors=True)
            out = [to_host(x).numpy() for x in out]
        else:
            out = list(self._mesh_to_host(v, t, c, axes))
            if dparams is not None and len(out[0]):
                out[0] = mesh_denoise.denoise_mesh(out[0], out[1], backend="host", **dparams)[0]
            if params is not None and len(out[0]):
                out[0] = smooth_mesh(out[0], out[1], backend="host", **params)[0]
            if cell is not None:
                out = simplify_mesh(out[0], out[1], cell, colors=out[2] if c is not None else None, backend="host")
        return (out[0].astype(np.float64), out[1].astype(np.int64)) + tuple(out[2:])

    @staticmethod
    def _mesh_to_host(v, t, c, axes):
        """Device mesh in lattice-index units (+ uint8 vertex colours or None) -> extract_mesh's numpy arrays, one copy."""
        parts = []
        if c is not None:
            c = c.reshape(-1)
            parts = [torch.cat([c, c.new_zeros((-c.numel()) % 8)]).view(torch.int64)]
        vw = FusionVolume._world(v, axes)
        both = to_host(torch.cat([vw.reshape(-1).view(torch.int64), t.reshape(-1).to(torch.int64)] + parts))
        nv, nt = vw.numel(), t.numel()
        out = (both[:nv].view(torch.float64).numpy().reshape(-1, 3), both[nv:nv + nt].numpy().reshape(-1, 3))
        if c is not None:
            out += (both[nv + nt:].view(torch.uint8)[:nv].numpy().reshape(-1, 3),)
        return out


# ---- brick-sparse fusion (csrc/fuse_sparse.hip): the same mesh from state kept only near the measured surfaces ----

MARK_MARGIN = 2                  # lattice steps the index box of a pixel's pyramid is widened by (fuse_sparse.hip's header argues it)


def mark_bricks_host(axes, views, trunc):
    """The mark rule of fuse_sparse.hip's header comment in numpy fp32, one operation per operator in its order, over the pixels
    of every view: the ascending int32 ids (bx nbp + by) nbp + bz, nbp = ceil(max(shape) / 8), of the bricks that can hold a
    lattice point some view updates with diff < trunc, or a lattice neighbour of one.  axes: strictly increasing fp32 arrays."""
    f32 = np.float32
    n = [len(a) for a in axes]
    nbp = (max(n) + 7) // 8
    mark = np.zeros((nbp, nbp, nbp), bool)
    trunc = f32(trunc)
    for v in views:
        L = lift_transform(v)
        depth = _np(v.depth, f32)
        with np.errstate(all="ignore"):
            d = depth * f32(v.dscale)
            yy, xx = np.nonzero((d > 0) & (d <= _F32_MAX))
            d = d[yy, xx]
            zs = (np.maximum(d - trunc, f32(0.0)), d + trunc)
            ys = (yy.astype(f32) - f32(0.5), yy.astype(f32) + f32(0.5))
            xs = (xx.astype(f32) - f32(0.5), xx.astype(f32) + f32(0.5))
            lo = [np.full(d.shape, np.inf, f32) for _ in range(3)]
            hi = [np.full(d.shape, -np.inf, f32) for _ in range(3)]
            fin = [np.ones(d.shape, bool) for _ in range(3)]
            for sz in zs:
                for sy in ys:
                    for sx in xs:
                        qx, qy = sx * sz, sy * sz
                        for k in range(3):
                            X = ((L[3 * k] * qx + L[3 * k + 1] * qy) + L[3 * k + 2] * sz) + L[9 + k]
                            fin[k] &= np.abs(X) <= _F32_MAX
                            lo[k], hi[k] = np.fmin(lo[k], X), np.fmax(hi[k], X)
        keep, cols = np.ones(d.shape, bool), []
        for k in range(3):
            i0 = np.where(fin[k], np.searchsorted(axes[k], lo[k], side="left"), 0)               # #{i : a[i] < lo}
            i1 = np.where(fin[k], np.searchsorted(axes[k], hi[k], side="right") - 1, n[k] - 1)   # #{i : a[i] <= hi} - 1
            i0, i1 = np.maximum(i0 - MARK_MARGIN, 0), np.minimum(i1 + MARK_MARGIN, n[k] - 1)
            keep &= i0 <= i1
            cols += [i0 >> 3, i1 >> 3]
        for b in np.unique(np.stack(cols, axis=1)[keep], axis=0):
            mark[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1] = True
    return np.flatnonzero(mark.reshape(-1)).astype(np.int32)


def integrate_bricks_host(tsdf, weight, color, bricks, axes, views, trunc, chunk=2048):
    """integrate_host on brick-major state (fuse_integrate_bricks' layout): every view, in order, at every lattice point of the
    listed bricks; points past the upper faces are never updated."""
    n = [len(a) for a in axes]
    nbp = (max(n) + 7) // 8
    ids = np.asarray(bricks, np.int64)
    for s in range(0, len(ids), chunk):
        part = ids[s:s + chunk]
        m = len(part)
        origin = (part // (nbp * nbp), (part // nbp) % nbp, part % nbp)
        idx = [origin[a][:, None] * 8 + np.arange(8) for a in range(3)]                     # (m, 8) lattice indices per axis
        shapes = ((m, 8, 1, 1), (m, 1, 8, 1), (m, 1, 1, 8))
        points = [axes[a][np.minimum(idx[a], n[a] - 1)].reshape(shapes[a]) for a in range(3)]
        inside = [(idx[a] < n[a]).reshape(shapes[a]) for a in range(3)]
        sl = slice(s * 512, (s + m) * 512)
        integrate_host(tsdf[sl].reshape(m, 8, 8, 8), weight[sl].reshape(m, 8, 8, 8),
                       None if color is None else color[sl].reshape(m, 8, 8, 8, 3), None, views, trunc, points=points,
                       valid=inside[0] & inside[1] & inside[2])


class SparseFusionVolume(FusionVolume):
    """FusionVolume(..., sparse=True): the TSDF state in 8^3-point bricks near the measured surfaces only (mesh_band.hip's brick
    table), for lattices the dense volume cannot hold - it takes 8 B per lattice point, 20 B with colours, and its mesh step
    stops at 2^31 points.  extract_mesh() returns the dense volume's arrays, in the same order.

    Why a subset is enough: a lattice point that no view updates with diff < trunc ends with tsdf == 1 exactly (or unobserved), and
    at an isovalue in (-1, 1) an edge or cell carries geometry only when one of its corners has tsdf < 1.  The needed points are
    those updated with diff < trunc, dilated by one lattice step; allocated are the bricks marked per depth pixel by the rule of
    fuse_sparse.hip's header comment, a superset of the bricks that hold a needed point.  Every view is integrated over every
    point of every allocated brick with the dense kernel's per-point arithmetic, so the state there equals the dense state.

    Deferred integration: a brick allocated after a view was integrated would lack that view's free-space updates, so
    integrate() only RECORDS its views - copies of depth and image on `device` (host backend: numpy), P and dscale; a 1080p view
    with colours is 33 MB, 300 of them 10 GB - and the state is built at first use (finalize(), extract_mesh(), observed_share()
    or any state attribute): bricks are allocated over all recorded views, then all views are integrated in order,
    ops.FUSE_MAX_VIEWS per launch.  A later integrate() drops the state; it is rebuilt from all views at the next use.

    Limits: strictly increasing axes, 2 <= max(shape) <= 8192, fewer than 2^31 / 512 allocated bricks, -1 < isovalue < 1.  The
    brick table is dense, ceil(max(shape) / 8)^3 int32: 512 MB for a side of 4096.
    State: bricks (int32 brick ids, ascending), table (brick id -> slot or -1), tsdf / weight (n_bricks * 512,) and color
    (n_bricks * 512, 3), brick-major: slot * 512 + (lx << 6 | ly << 3 | lz); backend "host" is the numpy-fp32 mirror, equal arrays."""

    def __init__(self, grid, trunc=None, colors=False, backend="device", device=None, sparse=True):
        self._init_lattice(grid, trunc, backend, device)
        if any(len(a) > 1 and not bool((np.diff(a) > 0).all()) for a in self.axes_host):
            raise ValueError("FusionVolume(sparse=True): strictly increasing axes")
        if not 2 <= max(self.shape) <= 8192:
            raise ValueError("FusionVolume(sparse=True): 2 <= max(shape) <= 8192 (the band kernels' limit)")
        self.colors = bool(colors)
        self.res, self.nbp = ops.fuse_brick_dims(self.shape)
        self._views, self._state = [], None

    def integrate(self, views, stats=None):
        """Records `views` (DepthViews, copied); they are fused, in order after the earlier ones, when the state is next used."""
        views = [v if isinstance(v, DepthView) else DepthView(*v) for v in views]
        if self.colors and any(v.image is None for v in views):
            raise ValueError("FusionVolume.integrate: colours are fused but a view has no image")
        if stats is not None:
            raise ValueError("FusionVolume.integrate: stats are counted by the dense host backend")
        for v in views:
            if len(v.depth.shape) != 2 or (self.colors and tuple(v.image.shape) != tuple(v.depth.shape) + (3,)):
                raise ValueError("FusionVolume.integrate: a view holds depth (H, W) and image (H, W, 3)")
            keep = self._copy_dev if self.backend == "device" else (lambda x: np.array(_np(x), dtype=np.float32, order="C"))
            self._views.append(DepthView(np.array(_np(v.P), dtype=np.float32).reshape(3, 4), keep(v.depth), float(v.dscale),
                                         keep(v.image) if self.colors else None))
        self.n_views += len(views)
        self._state = None

    def _copy_dev(self, x):
        y = self._dev(x)
        return y.clone() if torch.is_tensor(x) and y.data_ptr() == x.data_ptr() else y

    def finalize(self):
        """Builds the state from all recorded views (a no-op when it is current).  Returns self."""
        if self._state is not None:
            return self
        views, nt = self._views, self.nbp ** 3
        if self.backend == "device":
            mark = torch.zeros(nt, dtype=torch.uint8, device=self.device)
            for v in views:
                ops.fuse_mark_bricks(mark, self.axes, lift_transform(v), v.depth, v.dscale, self.trunc)
            table, bricks = ops.fuse_assign_bricks(mark)
            m = int(bricks.shape[0])
            tsdf = torch.zeros(m * 512, dtype=torch.float32, device=self.device)
            weight = torch.zeros(m * 512, dtype=torch.float32, device=self.device)
            color = torch.zeros(m * 512, 3, dtype=torch.float32, device=self.device) if self.colors else None
            for s in range(0, len(views), ops.FUSE_MAX_VIEWS):
                ops.fuse_integrate_bricks(tsdf, weight, color, bricks, self.axes,
                                          [(v.P, v.depth, v.dscale, v.image) for v in views[s:s + ops.FUSE_MAX_VIEWS]], self.trunc)
        else:
            bricks = mark_bricks_host(self.axes, views, self.trunc)
            m = len(bricks)
            if m * 512 >= 2 ** 31:
                raise ValueError("FusionVolume(sparse=True): 2^31 / 512 allocated bricks or more")
            table = np.full(nt, -1, np.int32)
            table[bricks] = np.arange(m, dtype=np.int32)
            tsdf, weight = np.zeros(m * 512, np.float32), np.zeros(m * 512, np.float32)
            color = np.zeros((m * 512, 3), np.float32) if self.colors else None
            integrate_bricks_host(tsdf, weight, color, bricks, self.axes, views, self.trunc)
        self._state = (bricks, table, tsdf, weight, color)
        return self

    bricks = property(lambda self: self.finalize()._state[0])
    table = property(lambda self: self.finalize()._state[1])
    tsdf = property(lambda self: self.finalize()._state[2])
    weight = property(lambda self: self.finalize()._state[3])
    color = property(lambda self: self.finalize()._state[4])

    @property
    def n_bricks(self):
        return int(self.bricks.shape[0])

    def allocated_share(self):
        """Allocated bricks over the bricks of the lattice."""
        return self.n_bricks / float(np.prod([(n + 7) // 8 for n in self.shape]))

    def state_bytes(self):
        """Bytes of the built state: tsdf, weight (and colours) of the allocated bricks, the brick list and the brick table."""
        return self.n_bricks * (512 * (20 if self.colors else 8) + 4) + 4 * self.nbp ** 3

    def _ray_state(self):
        bricks, table, tsdf, weight, color = self.finalize()._state
        return tsdf, weight, color, table, self.n_bricks > 0

    def extract_mesh(self, isovalue=0.0, simplify_cell=None, smooth=None, denoise=None):
        """FusionVolume.extract_mesh's arrays, the same mesh in the same order, for -1 < isovalue < 1 (ValueError otherwise: the
        allocation covers only what such an isovalue can cut).  Runs on the GPU whatever the backend.  simplify_cell, smooth,
        denoise: as there."""
        if not -1.0 < float(isovalue) < 1.0:
            raise ValueError("FusionVolume(sparse=True).extract_mesh: -1 < isovalue < 1")
        self.finalize()
        if self.n_bricks == 0:
            empty = (np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64))
            return empty + ((np.zeros((0, 3), np.uint8),) if self.colors else ())
        bricks, table, tsdf, weight, color = self._state
        axes = self.axes
        if self.backend == "host":
            if not torch.cuda.is_available():
                raise RuntimeError("FusionVolume.extract_mesh: marching cubes runs on the GPU (the SuRF hot path has no CPU fallback)")
            dev = torch.device("cuda") if self.device is None else self.device
            bricks, table, tsdf, weight = (torch.from_numpy(x).to(dev) for x in (bricks, table, tsdf, weight))
            color = None if color is None else torch.from_numpy(color).to(dev)
            axes = [torch.from_numpy(a).to(dev) for a in self.axes]
        band = ops.Band(self.res, table, None, bricks, ops.fuse_band_values(tsdf, weight), {}, shape=self.shape)
        v, t = ops.marching_cubes_band(band, float(isovalue), observed_only=True)
        c = None if color is None else ops.fuse_vertex_colors_bricks(v, color, table, self.shape)
        return self._finished(v, t, c, axes, simplify_cell, smooth, denoise)
