"""A mesh from the oriented point cloud (fusion.fuse_points + point_filter.estimate_normals): a point-set surface on the fusion lattice.

    cloud = fusion.fuse_points(views, 2)
    cloud, _ = point_filter.remove_outliers(cloud, max_dist=10 * voxel)
    normals = point_filter.estimate_normals(cloud, point_filter.camera_centres(views), max_dist=10 * voxel)
    vertices, triangles, colors = reconstruct(cloud, normals, voxel)            # world frame: mesh_io.write_ply as it is

The field is Kolluri's implicit moving-least-squares surface: at a lattice node x, f(x) = sum_i w_i n_i . (x - p_i) / sum_i w_i over
the points within the support radius R, with the compact weight w = (1 - |x - p|^2 / R^2)^4.  It is one gather pass - no global
solve, unlike a Poisson reconstruction - built from + - * / and comparisons only, and it leaves space without points unobserved, as
the TSDF does, instead of closing it.  THE RULE (rules 1-6: taking part, brick of a point, order, the pair arithmetic, node state,
allocation) is written once, in include/surf_hip.h above the surf_cloud_* entry points.

The field is stored as fusion state: tsdf = clamp(f / R, -1, 1) (positive on the normals' side, as in front of a measured surface),
weight = the number of admitted points, colour = the weighted mean, in the 8^3-point bricks near the cloud (SparseFusionVolume's
layout).  PointSetVolume therefore inherits extract_mesh (marching cubes over the cells whose eight corners are observed, vertex
colours, simplify_cell), ray_cast, n_bricks, allocated_share and state_bytes unchanged.

backend="device" runs csrc/point_surface.hip through surf_amd.ops (composite brick keys and torch's sort, bricks marked per point,
one workgroup per brick that stages its candidates through LDS) and has no host fall-back.  backend="host" is field_bricks_host,
the numpy-fp32 mirror, and returns equal arrays.  The mesh step runs on the GPU whatever the backend, as everywhere in fusion.
"""
import numpy as np
import torch

from .fusion import PointCloud, SparseFusionVolume, uniform_lattice

REACH_MARGIN = 1e-5                  # relative margin of reach (include/surf_hip.h, above rule 1)
REACH_ULPS = 4.0                     # ... and its absolute part, in fp32 spacings at the largest axis value


def support_reach(axes, voxel, radius):
    """reach of include/surf_hip.h in lattice steps (fp64): (R / voxel) (1 + 1e-5) + 4 ulp32(A) / voxel, A the largest |axis
    value|.  Every admitted (node, point) pair lies within it per axis; both backends use this one number."""
    A = max(float(np.abs(np.asarray(a, np.float32)).max()) for a in axes)
    return (float(np.float32(radius)) / float(voxel)) * (1.0 + REACH_MARGIN) + REACH_ULPS * float(np.spacing(np.float32(A))) / float(voxel)


def _ring(reach):
    from .ops import cloud_ring
    return cloud_ring(reach)


def _check_radius(radius, min_points, what):
    R = np.float32(radius)
    with np.errstate(all="ignore"):
        R2 = R * R
    if not (R > 0 and np.isfinite(R) and R2 > 0 and np.isfinite(R2)):
        raise ValueError(f"{what}: radius must be finite and > 0 (and so must its fp32 square), got {radius}")
    if isinstance(min_points, bool) or int(min_points) != min_points or min_points < 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1, got {min_points}")
    return R, R2, int(min_points)


def _cloud_arrays(points, normals, colors):
    P = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    N = normals.detach().cpu().numpy() if torch.is_tensor(normals) else np.asarray(normals)
    P, N = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(N, dtype=np.float32).reshape(-1, 3)
    if P.shape != N.shape:
        raise ValueError(f"point surface: one normal per point, got {P.shape} points and {N.shape} normals")
    if len(P) > 2 ** 31 - 1:
        raise ValueError(f"points: {len(P)} points exceed int32 indexing")
    C = None
    if colors is not None:
        C = colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors)
        if C.dtype != np.uint8 or C.shape != P.shape:
            raise ValueError(f"point surface: colors (n, 3) uint8, got {C.dtype} {C.shape}")
        C = np.ascontiguousarray(C)
    return P, N, C


def taking_part_host(points, normals):
    """Rule 1 without the lattice: the mask of the points whose coordinates and normal are finite and whose normal is not zero."""
    P, N, _ = _cloud_arrays(points, normals, None)
    return np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & (N != 0).any(axis=1)


# ---- the host mirror ----

def sort_cloud_host(points, normals, colors, axes, lo, voxel, reach):
    """Rules 1-3 in numpy: (sorted brick keys (m,) int64, the caller's index of every row (m,) int64, u (m, 3) float64 lattice
    coordinates) of the points taking part, in ascending (bx, by, bz, index) order."""
    P, N, _ = _cloud_arrays(points, normals, colors)
    ring = _ring(reach)
    nb = np.array([(len(a) + 7) // 8 for a in axes], np.int64)
    ext = nb + 2 * ring
    part = np.flatnonzero(np.isfinite(P).all(axis=1) & np.isfinite(N).all(axis=1) & (N != 0).any(axis=1))
    u = (P[part].astype(np.float64) - np.asarray(lo, np.float64).reshape(1, 3)) / float(voxel)
    bf = np.floor(u / 8.0)
    ok = ((bf >= -ring) & (bf < (nb + ring)[None, :])).all(axis=1)
    part, u, b = part[ok], u[ok], bf[ok].astype(np.int64)
    key = ((b[:, 0] + ring) * ext[1] + (b[:, 1] + ring)) * ext[2] + (b[:, 2] + ring)
    order = np.lexsort((part, key))
    return key[order], part[order].astype(np.int64), u[order]


def _reach_box(u, reach):
    """Rule 6's node interval per axis, unclamped: (i0, i1) int64 (m, 3)."""
    return np.ceil(u - reach).astype(np.int64), np.floor(u + reach).astype(np.int64)


def mark_bricks_host(u, shape, reach):
    """Rule 6: the ascending int32 ids of the bricks the points at lattice coordinates u (m, 3) allocate."""
    n = np.array(shape, np.int64)
    nbp = (int(n.max()) + 7) // 8
    i0, i1 = _reach_box(u, reach)
    i0, i1 = np.maximum(i0, 0), np.minimum(i1, n[None, :] - 1)
    keep = (i0 <= i1).all(axis=1)
    boxes = np.concatenate([i0[keep] >> 3, i1[keep] >> 3], axis=1)
    mark = np.zeros((nbp, nbp, nbp), bool)
    for b in (np.unique(boxes, axis=0) if len(boxes) else ()):
        mark[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1] = True
    return np.flatnonzero(mark.reshape(-1)).astype(np.int32)


def field_bricks_host(points, normals, colors, axes, radius, min_points=4, lattice=None, alloc_reach=None, stats=None):
    """The numpy-fp32 mirror of rules 1-6 (include/surf_hip.h), one operation per operator in the rule's order: (bricks (m,) int32
    ascending, table (nbp^3,) int32, tsdf, weight (m * 512,) fp32, color (m * 512, 3) fp32 or None), brick-major.
    axes: three fp32 coordinate arrays of a uniform lattice; lattice: its (lo, voxel), default uniform_lattice(axes).
    alloc_reach (tests): the reach rule 6 allocates with, e.g. 8 * ring for the blanket neighbourhood; the field does not depend
    on it.  stats (dict): receives points (taking part), candidates_max, pairs (node x staged candidate) and admitted."""
    R, R2, min_points = _check_radius(radius, min_points, "field_bricks_host")
    P, N, C = _cloud_arrays(points, normals, colors)
    axes = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in axes]
    lo, voxel = uniform_lattice(axes) if lattice is None else lattice
    lo, voxel = np.asarray(lo, np.float64).reshape(3), float(voxel)
    shape = [len(a) for a in axes]
    nbp = (max(shape) + 7) // 8
    reach = support_reach(axes, voxel, R)
    ring = _ring(reach)
    side = 2 * ring + 1
    ext = [(s + 7) // 8 + 2 * ring for s in shape]
    skey, sidx, u = sort_cloud_host(P, N, None, axes, lo, voxel, reach)
    bricks = mark_bricks_host(u, shape, reach if alloc_reach is None else float(alloc_reach))
    m = len(bricks)
    if m * 512 >= 2 ** 31:
        raise ValueError("point surface: 2^31 / 512 allocated bricks or more")
    table = np.full(nbp ** 3, -1, np.int32)
    table[bricks] = np.arange(m, dtype=np.int32)
    tsdf, weight = np.zeros(m * 512, np.float32), np.zeros(m * 512, np.float32)
    color = None if C is None else np.zeros((m * 512, 3), np.float32)
    SP, SN = P[sidx], N[sidx]
    SC = None if C is None else (C[sidx].astype(np.float32) + np.float32(0.5)) / np.float32(256.0)
    i0, i1 = _reach_box(u, reach)
    inv = np.float32(1.0) / R2
    one, zero = np.float32(1.0), np.float32(0.0)
    cand_max = pairs = admitted = 0
    for slot, bid in enumerate(bricks.astype(np.int64)):
        B = (bid // (nbp * nbp), (bid // nbp) % nbp, bid % nbp)
        runs = []
        for jx in range(side):
            for jy in range(side):
                k0 = ((B[0] + jx) * ext[1] + (B[1] + jy)) * ext[2] + B[2]
                runs.append(np.arange(np.searchsorted(skey, k0, "left"), np.searchsorted(skey, k0 + side, "left")))
        sel = np.concatenate(runs)
        keep = np.ones(len(sel), bool)
        for a in range(3):                                   # a candidate whose rule-6 box misses the brick is dropped
            keep &= (i0[sel, a] <= B[a] * 8 + 7) & (i1[sel, a] >= B[a] * 8)
        sel = sel[keep]
        cand_max, pairs = max(cand_max, len(sel)), pairs + 512 * len(sel)
        if not len(sel):
            continue
        idx = [B[a] * 8 + np.arange(8) for a in range(3)]
        x, y, z = (axes[a][np.minimum(idx[a], shape[a] - 1)] for a in range(3))
        inside = ((idx[0] < shape[0])[:, None, None] & (idx[1] < shape[1])[None, :, None] & (idx[2] < shape[2])[None, None, :]).reshape(512)
        p, nr = SP[sel], SN[sel]
        with np.errstate(all="ignore"):
            dx = np.broadcast_to((x[:, None] - p[None, :, 0])[:, None, None, :], (8, 8, 8, len(sel))).reshape(512, -1)
            dy = np.broadcast_to((y[:, None] - p[None, :, 1])[None, :, None, :], (8, 8, 8, len(sel))).reshape(512, -1)
            dz = np.broadcast_to((z[:, None] - p[None, :, 2])[None, None, :, :], (8, 8, 8, len(sel))).reshape(512, -1)
            d2 = (dx * dx + dy * dy) + dz * dz
            adm = d2 < R2
            t = one - d2 * inv
            t2 = t * t
            w = np.where(adm, t2 * t2, zero)
            g = (dx * nr[None, :, 0] + dy * nr[None, :, 1]) + dz * nr[None, :, 2]
            count = adm.sum(axis=1)
            sw = np.add.accumulate(w, axis=1, dtype=np.float32)[:, -1]               # sequential fp32 sums
            sf = np.add.accumulate(np.where(adm, w * g, zero), axis=1, dtype=np.float32)[:, -1]
            obs = inside & (count >= min_points) & (sw > 0)
            admitted += int(count.sum())
            sl = slice(slot * 512, slot * 512 + 512)
            tsdf[sl] = np.where(obs, np.fmin(np.fmax((sf / sw) / R, -one), one), zero)
            weight[sl] = np.where(obs, count.astype(np.float32), zero)
            if color is not None:
                for ch in range(3):
                    sc = np.add.accumulate(w * SC[sel][None, :, ch], axis=1, dtype=np.float32)[:, -1]
                    color[sl, ch] = np.where(obs, sc / sw, zero)
    if stats is not None:
        stats.update(points=len(skey), candidates_max=cand_max, pairs=pairs, admitted=admitted)
    return bricks, table, tsdf, weight, color


# ---- the public surface ----

class PointSetVolume(SparseFusionVolume):
    """The point-set surface of an oriented cloud as brick-sparse fusion state (module docstring; the rule: include/surf_hip.h).

    grid: (lo, hi, voxel) or three coordinate arrays of a UNIFORM lattice (fusion.uniform_lattice), SparseFusionVolume's limits.
    radius: the support radius R in world units; the support may reach across at most 4 bricks (R just under 32 voxels).
    min_points: a node is observed when at least this many points lie within R of it.  The default 4 is a judgement - one or two
    points give a plane through noise, not a surface - not a measurement.  colors: also blend the cloud's colours.
    set_cloud(cloud, normals) gives the cloud (a later call replaces it); the state is built at first use, as SparseFusionVolume
    builds its own: finalize(), extract_mesh(), ray_cast() or any state attribute.  integrate() raises: there are no depth views.
    backend "device" (HIP, state on `device`) or "host" (numpy fp32, equal arrays)."""

    def __init__(self, grid, radius, min_points=4, colors=False, backend="device", device=None):
        self.radius, _, self.min_points = _check_radius(radius, min_points, "PointSetVolume")
        super().__init__(grid, trunc=float(self.radius), colors=colors, backend=backend, device=device)
        self._lattice = self.lattice()
        self.reach = support_reach(self.axes_host, self._lattice[1], self.radius)
        _ring(self.reach)
        self._cloud, self._alloc_reach, self.stats = None, None, {}

    def integrate(self, views, stats=None):
        raise TypeError("PointSetVolume takes a cloud (set_cloud), not depth views")

    def set_cloud(self, cloud, normals):
        """cloud: a PointCloud or (n, 3) points (arrays or tensors, used as fp32); normals (n, 3), pointing into free space.  The
        arrays are copied.  With colors=True the cloud must carry colours (n, 3) uint8.  Returns self."""
        points, colors = (cloud.points, cloud.colors) if isinstance(cloud, PointCloud) else (cloud, None)
        if self.colors and colors is None:
            raise ValueError("PointSetVolume.set_cloud: colours are blended but the cloud has none")
        P, N, C = _cloud_arrays(points, normals, colors if self.colors else None)
        if self.backend == "device":
            self._cloud = tuple(None if x is None else torch.from_numpy(x).to(self.device) for x in (P, N, C))
        else:
            self._cloud = tuple(None if x is None else x.copy() for x in (P, N, C))
        self._state = None
        return self

    def finalize(self):
        """Builds the state from the cloud (a no-op when it is current).  Returns self."""
        if self._state is not None:
            return self
        if self._cloud is None:
            raise ValueError("PointSetVolume: no cloud yet (set_cloud)")
        P, N, C = self._cloud
        lo, voxel = self._lattice
        alloc = self.reach if self._alloc_reach is None else float(self._alloc_reach)
        if self.backend == "device":
            from . import ops
            cloud = ops.cloud_sort(P, N, C, self.axes, lo, voxel, self.reach)
            mark = torch.zeros(self.nbp ** 3, dtype=torch.uint8, device=self.device)
            ops.cloud_mark_bricks(mark, cloud[1], self.axes, lo, voxel, alloc)
            table, bricks = ops.fuse_assign_bricks(mark)
            tsdf, weight, color, staged = ops.cloud_field_bricks(cloud, bricks, self.axes, lo, voxel, self.reach, float(self.radius),
                                                                 self.min_points, staged=True)
            self._staged = staged
            self.stats = {"points": int(cloud[0].shape[0])}
            self._state = (bricks, table, tsdf, weight, color)
        else:
            self.stats = {}
            self._state = field_bricks_host(P, N, C, self.axes, self.radius, self.min_points, lattice=(lo, voxel), alloc_reach=alloc,
                                            stats=self.stats)
        return self

    def cloud_stats(self):
        """{points: taking part, bricks, allocated_share, candidates_max: the most candidates one brick ran through, pairs: node x
        candidate evaluations} of the built state (device backend: two host reads)."""
        self.finalize()
        out = {"points": self.stats["points"], "bricks": self.n_bricks, "allocated_share": self.allocated_share()}
        if self.backend == "device":
            staged = self._staged.long()
            out.update(candidates_max=int(staged.max()) if staged.numel() else 0, pairs=512 * int(staged.sum()))
        else:
            out.update(candidates_max=self.stats["candidates_max"], pairs=self.stats["pairs"])
        return out


def cloud_bounds(points, normals, radius):
    """(lo, hi) float64: the box of the points taking part (rule 1), padded by the radius."""
    P, N, _ = _cloud_arrays(points, normals, None)
    part = P[taking_part_host(P, N)].astype(np.float64)
    if not len(part):
        raise ValueError("reconstruct: no point of the cloud takes part (finite coordinates and a finite non-zero normal)")
    return part.min(axis=0) - float(radius), part.max(axis=0) + float(radius)


@torch.no_grad()
def reconstruct(cloud, normals, voxel, radius=None, min_points=4, bounds=None, colors=None, simplify_cell=None, backend="device",
                device=None, stats=None, smooth=None, denoise=None):
    """(vertices (V, 3) float64, triangles (F, 3) int64[, colors (V, 3) uint8]) as PointSetVolume.extract_mesh returns them: the
    zero set of the point-set surface of `cloud` (a PointCloud or (n, 3) points) with `normals` (n, 3) on a lattice of step voxel.
    radius: default 3 voxel.  bounds (lo, hi): default the box of the points taking part, padded by the radius.  colors: None =
    blended when the cloud has them.  simplify_cell, smooth, denoise, backend, device: as extract_mesh's and the volume's.
    stats (dict): receives points, bricks, allocated_share, candidates_max, vertices, faces."""
    voxel = float(voxel)
    radius = 3.0 * voxel if radius is None else float(radius)
    points = cloud.points if isinstance(cloud, PointCloud) else cloud
    has = isinstance(cloud, PointCloud) and cloud.colors is not None
    colors = has if colors is None else bool(colors)
    lo, hi = cloud_bounds(points, normals, radius) if bounds is None else bounds
    vol = PointSetVolume((lo, hi, voxel), radius, min_points=min_points, colors=colors, backend=backend, device=device)
    vol.set_cloud(cloud, normals)
    mesh = vol.extract_mesh(simplify_cell=simplify_cell, smooth=smooth, denoise=denoise)
    if stats is not None:
        cs = vol.cloud_stats()
        stats.update(points=cs["points"], bricks=cs["bricks"], allocated_share=cs["allocated_share"],
                     candidates_max=cs["candidates_max"], vertices=int(len(mesh[0])), faces=int(len(mesh[1])))
    return mesh
