#!/usr/bin/env python3
"""Golden results of the REFERENCE's protocol mesh cleaner: generated in the build container by importing
/root/reference/evaluation/clean_mesh.py and running ITS `clean_points_by_mask` (minimal_vis 0, 1, 2) and
`clean_mesh_faces_by_mask` (minimal_vis 1) on the synthetic DTU_TEST tree of tests/golden/dtu_test_scene.py (1200 x 1600, the
size the reference hard-codes).  Only data is committed (tests/golden/clean_dtu.npz): the vertices, faces and projection
matrices that went in, and the masks / mesh that came out.  The mask PNGs are written into a temporary directory.

Third-party modules the reference imports and this image lacks are stood in for, for exactly the calls it makes:
  cv2.imread(path)                                     -> PIL, as a three-channel uint8 array
  cv2.getStructuringElement(MORPH_ELLIPSE, (k, k))     -> surf_amd.evaluation.clean_dtu.ellipse_footprint (OpenCV's row rule)
  cv2.dilate(img, kernel, iterations=1)                -> scipy.ndimage.grey_dilation per channel with that footprint, zeros outside
  cv2.decomposeProjectionMatrix(P)                     -> mvs_io.decompose_projection (not reached by the functions recorded here)
  trimesh.load / trimesh.Trimesh / .export             -> objects that hold the arrays (no vertex merging, no file)
  open3d, tqdm                                         -> empty modules
  np.long, np.bool                                     -> np.int64, bool (removed from numpy since the reference was written)
Everything else that runs is the reference's own code: the camera-file parser, P = K4 @ E, the matmul projection, the rounding,
the padded mask and its asymmetric range test, the threshold, the vertex / face re-indexing.  What this fixture therefore does
NOT pin is OpenCV's ellipse table and dilation themselves.

The reference projects with np.matmul, whose summation order (and use of fused multiply-adds) is not defined; a vertex whose
float64 X / Z or Y / Z lies within BAND px of a half-integer in some view could round either way and is excluded by the tests.
This generator asserts that the committed vertices keep that share under CAP (expected: none)."""
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from surf_amd.datasets import mvs_io  # noqa: E402
from surf_amd.evaluation import clean_dtu  # noqa: E402
from tests.golden import dtu_test_scene as S  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402

BAND, CAP = 1e-6, 1e-3


def near_tie(vertices, P_list, band=BAND):
    """(V,) bool: float64 X / Z or Y / Z within `band` px of a half-integer in some view."""
    near = np.zeros(len(vertices), dtype=bool)
    for P in P_list:
        qx, qy, _ = clean_dtu._project(vertices, P)
        with np.errstate(all="ignore"):
            for q in (qx, qy):
                near |= np.abs(np.abs(q - np.floor(q)) - 0.5) < band
    return near


def _cv2_stub():
    m = types.ModuleType("cv2")
    m.MORPH_ELLIPSE = 2

    def imread(path):
        return np.ascontiguousarray(np.array(Image.open(path).convert("RGB"))[..., ::-1])

    def get_structuring_element(shape, ksize):
        assert shape == m.MORPH_ELLIPSE and ksize[0] == ksize[1]
        return clean_dtu.ellipse_footprint(ksize[0]).astype(np.uint8)

    def dilate(img, kernel, iterations=1):
        assert iterations == 1 and img.dtype == np.uint8
        fp = kernel.astype(bool)
        return np.stack([ndimage.grey_dilation(img[..., c], footprint=fp, mode="constant", cval=0) for c in range(img.shape[-1])], axis=-1)

    def decompose(P):
        intr, pose = mvs_io.decompose_projection(P)
        c = np.concatenate([pose[:3, 3].astype(np.float64), [1.0]])[:, None]
        return intr[:3, :3].copy(), pose[:3, :3].astype(np.float64).T, c
    m.imread, m.getStructuringElement, m.dilate, m.decomposeProjectionMatrix = imread, get_structuring_element, dilate, decompose
    return m


def _trimesh_stub(store):
    m = types.ModuleType("trimesh")

    class Trimesh:
        def __init__(self, vertices, faces):
            self.vertices, self.faces = np.asarray(vertices), np.asarray(faces)

        def export(self, path):
            store[path] = (self.vertices.copy(), self.faces.copy())

    def load(path):
        v, f = store[path]
        return Trimesh(v.copy(), f.copy())
    m.Trimesh, m.load = Trimesh, load
    return m


def main():
    store = {}
    sys.modules["cv2"] = _cv2_stub()
    sys.modules["trimesh"] = _trimesh_stub(store)
    sys.modules["open3d"] = types.ModuleType("open3d")
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, *a, **k: x
    sys.modules["tqdm"] = tq
    np.long, np.bool = np.int64, bool
    sys.path.insert(0, os.path.join(G.REF, "evaluation"))
    import clean_mesh as R                                   # the reference's evaluation/clean_mesh.py

    vertices, faces = S.soup()
    out = {"vertices": vertices, "faces": faces.astype(np.int32)}
    with tempfile.TemporaryDirectory() as root:
        S.write_tree(root)
        args = types.SimpleNamespace(root_dir=root)
        P_list = [R.read_cam_file(os.path.join(root, "cameras", f"{vid:08d}_cam.txt")) for vid in S.VIEW_IDS]
        out["P"] = np.stack(P_list).astype(np.float32)
        assert all(np.array_equal(P, clean_dtu.projection_matrix(os.path.join(root, "cameras", f"{vid:08d}_cam.txt")))
                   for P, vid in zip(P_list, S.VIEW_IDS))
        for mv in (0, 1, 2):
            out[f"inside_minvis{mv}"] = np.asarray(R.clean_points_by_mask(args, vertices, S.SCAN, S.VIEW_IDS, mv, 11), dtype=bool)
        store["in.ply"] = (vertices, faces)
        R.clean_mesh_faces_by_mask(args, "in.ply", "out.ply", S.SCAN, S.VIEW_IDS, minimal_vis=1, mask_dilated_size=11)
        out["clean_vertices"], out["clean_faces"] = store["out.ply"][0], store["out.ply"][1].astype(np.int32)
    near = near_tie(vertices, P_list)
    assert near.mean() <= CAP, f"{int(near.sum())} of {len(near)} vertices lie within {BAND} px of a rounding tie"
    for mv in (0, 1, 2):
        print(f"minimal_vis {mv}: {int(out[f'inside_minvis{mv}'].sum())} of {len(vertices)} vertices inside")
    print(f"near a tie: {int(near.sum())}; cleaned mesh: {len(out['clean_vertices'])} vertices, {len(out['clean_faces'])} faces")
    path = os.path.join(HERE, "clean_dtu.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
