"""The mesh cleaner of the DTU evaluation protocol (evaluation/clean_mesh.py:13-29, 101-162, 189-256, 293-316 of the reference):
the step between the world-frame PLY of `--mode val` and evaluation/dtu_eval.py, run with the DTU_TEST object masks.  It is NOT
the runner's cleaner (surf_amd.evaluation.clean_mesh, utils/clean_mesh.py): this one takes world-frame millimetre vertices, the
full-resolution projection P = K4 @ E of the MVSNet camera files, an OpenCV elliptical dilation, a ROUNDED projection into a mask
padded by a one-pixel ring of ones, and it removes vertices, not only faces.

  1. clean_faces_by_mask          keep the vertices that more than `minimal_vis` of the views see (points_in_masks), and the
                                  faces whose three vertices are kept; unreferenced kept vertices stay
  2. clean_faces_outside_frustum  keep the faces that are the first hit of a ray through a set pixel of some view's dilated mask,
                                  then drop connected components of fewer than 500 faces and unreferenced vertices

Meshes are (vertices (V,3) float64, faces (F,3) int) arrays, generalised from the reference's hard-coded 1200 x 1600 to the
masks' own (H, W).  cv2 / trimesh / open3d / pyembree are not dependencies; the stand-ins, none of which the tests can pin
against the library it replaces (none is available to the build):
  * ellipse_footprint is a restatement of cv2.getStructuringElement(MORPH_ELLIPSE) from its documented row rule;
  * the first-hit test is the z-buffer rasterisation of surf_amd.evaluation.clean_mesh.visible_faces (upscale=1: the integer
    pixels) in place of pyembree's intersects_first, with that module's one deviation: the no-hit marker is excluded explicitly
    instead of dropping `values[1:]`;
  * trimesh.load merges duplicate vertices; read_ply_mesh does not (a no-op on marching-cubes meshes, whose vertices are unique).

backend="host" (the default) is the path above.  backend="device" runs every stage on the GPU (csrc/dtu_clean.hip and
csrc/mesh_clean.hip through surf_amd.ops) and returns the same arrays; the *_device functions are the stage-by-stage twins."""
import argparse
import glob
import math
import os

import numpy as np
import torch
from PIL import Image
from scipy import ndimage

from ..datasets import mvs_io
from . import clean_mesh as CM

# evaluation/clean_mesh.py:293-300 (settings data)
DTU_SCANS = [24, 37, 40, 55, 63, 65, 69, 83, 97, 105, 106, 110, 114, 118, 122]
VIEW_SETS = {0: [23, 24, 33, 22, 15, 34, 14, 32, 16, 35, 25], 1: [43, 42, 44, 33, 34, 32, 45, 23, 41, 24, 31]}
MASK_THRESHOLD = 128
COORD_LIMIT = float(2 ** 30)


def ellipse_half_widths(k):
    """Half-width dx of every row of ellipse_footprint(k): row i covers the columns [c - dx, c + dx]."""
    k = int(k)
    if k < 1 or k % 2 == 0:
        raise ValueError(f"ellipse footprint: expected an odd size, got {k}")
    r = c = k // 2
    return [int(round(c * math.sqrt((r * r - (i - r) * (i - r)) / (r * r)))) if r else 0 for i in range(k)]


def ellipse_footprint(k):
    """cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) for odd k as a (k, k) bool array: with r = c = k // 2, row i
    (dy = i - r) is set on the columns [c - dx, c + dx], dx = round(c * sqrt((r*r - dy*dy) / (r*r))) (half to even).  Row widths
    at k = 11: 1, 7, 9, 11, 11, 11, 11, 11, 9, 7, 1.  A stand-in: cv2 is not available to the build, so no test pins this table
    against OpenCV itself."""
    half = ellipse_half_widths(k)
    c = len(half) // 2
    cols = np.arange(len(half))
    return np.stack([np.abs(cols - c) <= dx for dx in half])


def dilate_ellipse(mask_u8, k):
    """cv2.dilate(mask, ellipse_footprint(k)) of a uint8 (H, W) mask: the maximum over the footprint; pixels outside the image do
    not contribute.  Row by row of the footprint: a horizontal running maximum of the row's width, shifted by the row's dy."""
    m = np.asarray(mask_u8)
    if m.dtype != np.uint8 or m.ndim != 2:
        raise TypeError("dilate_ellipse: expected a uint8 (H, W) mask")
    half = ellipse_half_widths(k)
    r, H = len(half) // 2, m.shape[0]
    out = np.zeros_like(m)
    rows = {}
    for i, dx in enumerate(half):
        if dx not in rows:
            rows[dx] = ndimage.maximum_filter1d(m, 2 * dx + 1, axis=1, mode="constant", cval=0) if dx else m
        dy = i - r
        lo, hi = max(0, -dy), min(H, H - dy)
        if lo < hi:
            np.maximum(out[lo:hi], rows[dx][lo + dy:hi + dy], out=out[lo:hi])
    return out


def projection_matrix(cam_file):
    """read_cam_file of evaluation/clean_mesh.py:13-29: the float32 4 x 4 K4 @ E of an MVSNet camera file, at the file's own
    resolution (no intrinsics scaling, no depth range)."""
    intrinsics, extrinsics, _ = mvs_io.read_cam_file(cam_file)
    return intrinsics @ extrinsics


def _project(points, P):
    """(qx, qy, Z) of clean_points_by_mask's projection in float64, one operation per operator, left to right as written: no
    matmul, so no fused multiply-add and no BLAS summation order.  This is the sequence csrc/dtu_clean.hip evaluates."""
    p = np.asarray(points, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        X = ((P[0, 0] * x + P[0, 1] * y) + P[0, 2] * z) + P[0, 3]
        Y = ((P[1, 0] * x + P[1, 1] * y) + P[1, 2] * z) + P[1, 3]
        Z = ((P[2, 0] * x + P[2, 1] * y) + P[2, 2] * z) + P[2, 3]
        return X / Z, Y / Z, Z


def points_in_masks(points, P_list, masks_u8, dilate=11):
    """clean_points_by_mask (evaluation/clean_mesh.py:101-141) up to its threshold: the (V,) int32 number of views that see each
    point.  Per view: u = rint(X / Z) + 1, v = rint(Y / Z) + 1 (half to even, as np.round); the view counts when 0 <= u <= W,
    0 <= v <= H and the padded mask - (dilated > 128) inside a one-pixel ring of ones - is set at (v, u).  As in the reference,
    u = W + 1 and v = H + 1 lie on the ring but are not in range, and Z is not tested for sign.  Two cases the reference leaves
    undefined are defined here: a view does not count when Z == 0, or when |X / Z| or |Y / Z| is not finite or exceeds 2^30.
    masks_u8: (nv, H, W) uint8, or a list of (H, W); dilate=0 or None: the masks are taken as already dilated."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    count = np.zeros(len(points), dtype=np.int32)
    for P, mask in zip(P_list, masks_u8):
        mask = np.asarray(mask)
        H, W = mask.shape
        padded = np.ones((H + 2, W + 2), dtype=bool)
        padded[1:-1, 1:-1] = (dilate_ellipse(mask, dilate) if dilate else mask) > MASK_THRESHOLD
        qx, qy, Z = _project(points, P)
        with np.errstate(all="ignore"):
            ok = (Z != 0) & (np.abs(qx) <= COORD_LIMIT) & (np.abs(qy) <= COORD_LIMIT)
        u = np.rint(np.where(ok, qx, -2.0)).astype(np.int64) + 1
        v = np.rint(np.where(ok, qy, -2.0)).astype(np.int64) + 1
        ok &= (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
        count += (ok & padded[v.clip(0, H + 1), u.clip(0, W + 1)]).astype(np.int32)
    return count


def clean_faces_by_mask(vertices, faces, count, minimal_vis=1):
    """clean_mesh_faces_by_mask (evaluation/clean_mesh.py:144-162): the vertices with count > minimal_vis in their order -
    including ones no face references - and the faces whose three vertices are kept, re-indexed."""
    vertices, faces = np.asarray(vertices), np.asarray(faces).reshape(-1, 3)
    keep = np.asarray(count) > minimal_vis
    index = np.cumsum(keep) - 1
    face_keep = keep[faces].all(axis=1) if len(faces) else np.zeros(0, dtype=bool)
    return vertices[keep], index[faces[face_keep]]


def _frustum_cameras(P_list):
    """load_K_Rt_from_P of every view (evaluation/clean_mesh.py:217): (intrinsics, camera-to-world poses) as fp32 tensors."""
    K, pose = zip(*(mvs_io.decompose_projection(np.asarray(P)[:3]) for P in P_list))
    return torch.from_numpy(np.stack(K)).float(), torch.from_numpy(np.stack(pose)).float()


def _outside_frustum_host(vertices, faces, P_list, masks_set, min_component, device, ids=None):
    """The second stage with the masks already dilated and thresholded; `ids` (one row per vertex, optional) goes through the
    same two compactions as the vertices."""
    intrs, c2ws = _frustum_cameras(P_list)
    keep = CM.visible_faces(vertices, faces, torch.from_numpy(np.stack(masks_set)), intrs, c2ws, upscale=1, device=device)
    va, fa = CM.update_faces(vertices, faces, keep)
    keep_b = CM.face_components(fa, min_component)
    vb, fb = CM.update_faces(va, fa, keep_b)
    if ids is not None:
        ids = CM.update_faces(CM.update_faces(ids, faces, keep)[0], fa, keep_b)[0]
    return vb, fb, ids


def clean_faces_outside_frustum(vertices, faces, P_list, masks_u8, dilate=11, min_component=500, device="cuda"):
    """clean_mesh_faces_outside_frustum (evaluation/clean_mesh.py:189-256): the union over the views of the faces that are the
    first hit of the ray through an integer pixel whose dilated mask is > 128, then components under `min_component` faces and
    unreferenced vertices dropped.  The z-buffer first hit of clean_mesh.visible_faces stands in for pyembree (it runs on the
    GPU in the host path too, as in clean_mesh.clean_mesh_outside_frustum)."""
    vertices, faces = np.asarray(vertices), np.asarray(faces).reshape(-1, 3)
    if len(faces) == 0 or len(P_list) == 0:
        return vertices[:0], faces[:0]
    masks = [(dilate_ellipse(np.asarray(m), dilate) if dilate else np.asarray(m)) > MASK_THRESHOLD for m in masks_u8]
    return _outside_frustum_host(vertices, faces, P_list, masks, min_component, device)[:2]


# ---- the device path ----

def _dev_masks_u8(masks_u8, device):
    m = masks_u8 if torch.is_tensor(masks_u8) else torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x) for x in masks_u8])))
    if m.dtype != torch.uint8 or m.dim() != 3:
        raise TypeError("masks: expected (n_views, H, W) uint8")
    return m.to(device).contiguous()


def _proj_tensor(P_list):
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(P, dtype=np.float32) for P in P_list])))


def dilate_ellipse_device(masks_u8, k, device="cuda"):
    """dilate_ellipse of one (H, W) mask or of every slice of (nv, H, W) masks: uint8 device tensor of the same shape."""
    from .. import ops
    m = masks_u8 if torch.is_tensor(masks_u8) else torch.from_numpy(np.ascontiguousarray(masks_u8))
    if m.dim() == 2:
        return ops.dtu_clean_dilate(_dev_masks_u8(m[None], device), ellipse_half_widths(k))[0]
    return ops.dtu_clean_dilate(_dev_masks_u8(m, device), ellipse_half_widths(k))


def points_in_masks_device(points, P_list, masks_u8, dilate=11, device="cuda"):
    """points_in_masks on the device, in the float64 operation order written in csrc/dtu_clean.hip: (V,) int32 device tensor."""
    from .. import ops
    p = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float64)))
    p = p.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    if len(P_list) == 0:
        return torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
    m = _dev_masks_u8(masks_u8, device)
    if dilate:
        m = ops.dtu_clean_dilate(m, ellipse_half_widths(dilate))
    return ops.dtu_clean_points_in_masks(p, m, _proj_tensor(P_list))


def clean_faces_by_mask_device(vertices, faces, count, minimal_vis=1, device="cuda"):
    """clean_faces_by_mask on the device: (vertices in the dtype they came in, faces int64) device tensors, order preserved."""
    from .. import ops
    v = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.ascontiguousarray(vertices))
    c = count if torch.is_tensor(count) else torch.from_numpy(np.ascontiguousarray(count))
    v = v.to(device).reshape(-1, 3).contiguous()
    out_v, out_f, _ = ops.dtu_clean_remove_vertices(v, CM._dev_faces(faces, device), c.to(device=device, dtype=torch.int32).contiguous(),
                                                    minimal_vis)
    return out_v, out_f.long()


def clean_faces_outside_frustum_device(vertices, faces, P_list, masks_u8, dilate=11, min_component=500, device="cuda"):
    """clean_faces_outside_frustum on the device: (vertices, faces int64) device tensors."""
    from .. import ops
    v, v32, f = CM._dev_mesh(vertices, faces, device)
    v = v.reshape(-1, 3)
    if f.shape[0] == 0 or len(P_list) == 0:
        return v[:0], f[:0].long()
    intrs, c2ws = _frustum_cameras(P_list)
    m = _dev_masks_u8(masks_u8, device)
    if dilate:
        m = ops.dtu_clean_dilate(m, ellipse_half_widths(dilate))
    return CM._outside_frustum_device(ops, v, v32.reshape(-1, 3), f, (m > MASK_THRESHOLD).to(torch.uint8).contiguous(), intrs, c2ws,
                                      1, min_component)


# ---- both stages ----

@torch.no_grad()
def clean_dtu(vertices, faces, P_list, masks_u8, dilate=11, minimal_vis=1, min_component=500, backend="host", device="cuda",
              return_tensors=False, return_index=False):
    """Both stages (evaluation/clean_mesh.py:314-316) for one mesh, given the views' projections (float32 4 x 4) and raw uint8
    masks.  backend="device": the same result with every stage on the GPU; return_tensors=True (device only) keeps it there.
    return_index=True: also the (V',) int64 ids, in the input mesh, of the vertices that survive."""
    if backend not in ("host", "device"):
        raise ValueError(f"backend: expected 'host' or 'device', got {backend!r}")
    if backend == "host":
        if return_tensors:
            raise ValueError('return_tensors=True needs backend="device"')
        vertices, faces = np.asarray(vertices, dtype=np.float64).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
        dilated = [dilate_ellipse(np.asarray(m), dilate) if dilate else np.asarray(m) for m in masks_u8]
        count = points_in_masks(vertices, P_list, dilated, dilate=None)
        index = np.flatnonzero(count > minimal_vis)
        v1, f1 = clean_faces_by_mask(vertices, faces, count, minimal_vis)
        if len(f1) == 0 or len(P_list) == 0:
            v2, f2, index = v1[:0], f1[:0], index[:0]
        else:
            v2, f2, index = _outside_frustum_host(v1, f1, P_list, [d > MASK_THRESHOLD for d in dilated], min_component, device, index)
        return (v2, f2, index) if return_index else (v2, f2)
    from .. import ops
    if str(device) == "cpu" or not torch.cuda.is_available():
        raise RuntimeError('clean_dtu(backend="device") needs a GPU: there is no host fall-back for the device path')
    v, _, f = CM._dev_mesh(vertices, faces, device)
    v = v.to(torch.float64).reshape(-1, 3).contiguous()
    m = _dev_masks_u8(masks_u8, device)
    if dilate and m.numel():
        m = ops.dtu_clean_dilate(m, ellipse_half_widths(dilate))
    if len(P_list):
        count = ops.dtu_clean_points_in_masks(v, m, _proj_tensor(P_list))
    else:
        count = torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)
    v1, f1, vkeep = ops.dtu_clean_remove_vertices(v, f, count, minimal_vis)
    index = None
    if f1.shape[0] == 0 or len(P_list) == 0:
        v2, f2 = v1[:0], f1[:0].long()
        if return_index:
            index = torch.zeros(0, dtype=torch.int64, device=v.device)
    else:
        intrs, c2ws = _frustum_cameras(P_list)
        mb = (m > MASK_THRESHOLD).to(torch.uint8).contiguous()
        keep = ops.clean_visible_faces(v1.to(torch.float32).contiguous(), f1, mb, intrs, c2ws, 1)
        va, fa = ops.clean_update_faces(v1, f1, keep)
        keep_b = ops.clean_components(fa, min_component)
        v2, f2 = ops.clean_update_faces(va, fa, keep_b)
        if return_index:                               # the same two compactions on the rows (id, id, id)
            ids = torch.nonzero(vkeep).reshape(-1, 1).repeat(1, 3).contiguous()
            ia, _ = ops.clean_update_faces(ids, f1, keep)
            ib, _ = ops.clean_update_faces(ia, fa, keep_b)
            index = ib[:, 0].contiguous()
        f2 = f2.long()
    if not return_tensors:
        v2, f2 = v2.cpu().numpy(), f2.cpu().numpy()
        index = None if index is None else index.cpu().numpy()
    return (v2, f2, index) if return_index else (v2, f2)


def read_scan_views(root_dir, scan, view_set=1, n_view=3):
    """(view ids, projections, masks) of a scan of a DTU_TEST tree: cameras/{vid:08d}_cam.txt and channel 0 of
    scan{N}/mask/{vid:03d}.png (cv2.imread's first channel of a grey mask), read through PIL."""
    if view_set not in VIEW_SETS:
        raise ValueError(f"view_set: expected one of {sorted(VIEW_SETS)}, got {view_set!r}")
    vids = VIEW_SETS[view_set][:n_view]
    P_list = [projection_matrix(os.path.join(root_dir, "cameras", f"{vid:08d}_cam.txt")) for vid in vids]
    masks = []
    for vid in vids:
        m = np.array(Image.open(os.path.join(root_dir, f"scan{scan}", "mask", f"{vid:03d}.png")))
        masks.append(np.ascontiguousarray(m[..., 0] if m.ndim == 3 else m).astype(np.uint8))
    return vids, P_list, masks


def clean_dtu_scan(vertices, faces, root_dir, scan, view_set=1, n_view=3, backend="host", device="cuda", return_tensors=False,
                   return_index=False):
    """The protocol's cleaning of one scan's world-frame mesh with the DTU_TEST tree under root_dir: the first n_view views of
    the view set, 11 x 11 elliptical dilation, minimal_vis = 1, components under 500 faces dropped."""
    _, P_list, masks = read_scan_views(root_dir, scan, view_set, n_view)
    return clean_dtu(vertices, faces, P_list, masks, dilate=11, minimal_vis=1, min_component=500, backend=backend, device=device,
                     return_tensors=return_tensors, return_index=return_index)


def main(argv=None):
    """evaluation/clean_mesh.py's command: <out_dir>/*scan{N}_epoch0.ply -> <out_dir>/final/clean_{N:03d}.ply (first stage) and
    <out_dir>/final/scan{N}.ply (both stages, the file evaluation/dtu_eval.py reads)."""
    from .. import mesh_io
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--root_dir", required=True, help="DTU_TEST tree: cameras/ and scan{N}/mask/")
    ap.add_argument("--out_dir", default="./outputs/mesh", help="directory of the *scan{N}_epoch0.ply meshes")
    ap.add_argument("--n_view", type=int, default=3)
    ap.add_argument("--set", type=int, default=1, choices=sorted(VIEW_SETS))
    ap.add_argument("--scans", type=int, nargs="+", default=DTU_SCANS)
    ap.add_argument("--backend", default="host", choices=["host", "device"])
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    os.makedirs(os.path.join(args.out_dir, "final"), exist_ok=True)
    for scan in args.scans:
        found = sorted(glob.glob(os.path.join(args.out_dir, f"*scan{scan}_epoch0.ply")))
        if not found:
            raise SystemExit(f"clean_dtu: no *scan{scan}_epoch0.ply under {args.out_dir}")
        vertices, faces = mesh_io.read_ply_mesh(found[0])
        _, P_list, masks = read_scan_views(args.root_dir, scan, args.set, args.n_view)
        if args.backend == "device":
            count = points_in_masks_device(vertices, P_list, masks, 11, args.device)
            v1, f1 = (x.cpu().numpy() for x in clean_faces_by_mask_device(vertices, faces, count, 1, args.device))
            stage2 = clean_faces_outside_frustum_device
        else:
            v1, f1 = clean_faces_by_mask(vertices, faces, points_in_masks(vertices, P_list, masks, 11), 1)
            stage2 = clean_faces_outside_frustum
        mesh_io.write_ply(os.path.join(args.out_dir, "final", f"clean_{scan:03d}.ply"), v1, f1)
        v2, f2 = (x.cpu().numpy() if torch.is_tensor(x) else x for x in stage2(v1, f1, P_list, masks, 11, 500, args.device))
        mesh_io.write_ply(os.path.join(args.out_dir, "final", f"scan{scan}.ply"), v2, f2)
        print(f"scan{scan}: {len(faces)} faces -> {len(f1)} in the masks -> {len(f2)} seen, in components of 500 or more")


if __name__ == "__main__":
    main()
