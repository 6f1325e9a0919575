"""A synthetic DTU_TEST tree for the protocol mesh cleaner (surf_amd.evaluation.clean_dtu): MVSNet camera files under cameras/,
object masks under scan{N}/mask/, and a seeded vertex / face soup in world millimetres.  Shared by the golden generator
(make_golden_clean_dtu.py) and the tests; the masks are integer arithmetic, so every machine draws the same ones."""
import os

import numpy as np
from PIL import Image

from tests.golden.dtu_scene import write_cam

H, W = 1200, 1600
K = np.array([[2892.33, 0.0, 823.2], [0.0, 2883.18, 619.07], [0.0, 0.0, 1.0]])
VIEW_IDS = [43, 42, 44]                       # the first three views of the reference's view set 1
SCAN = 24


def ring_cams(n=3, radius=600.0):
    """world-to-camera matrices of n cameras on a ring about `radius` mm from the origin, looking at it."""
    cams = []
    for i in range(n):
        a = 0.35 * (i - n // 2)
        o = np.array([radius * np.sin(a), 25.0 * i - 20.0, -radius * np.cos(a)])
        z = -o / np.linalg.norm(o)
        x = np.cross([0, 1.0, 0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, o
        cams.append(np.linalg.inv(c2w))
    return cams


def masks(h=H, w=W):
    """Three uint8 (h, w) masks, 0 / 255: an ellipse, a rectangle that touches the top and the right border, a blob (union of
    discs) with a hole.  Scaled with the image, in integers."""
    yy, xx = np.mgrid[:h, :w].astype(np.int64)
    a, b = (5 * w) // 16, (5 * h) // 24
    m0 = ((xx - w // 2) ** 2) * b * b + ((yy - h // 2) ** 2) * a * a <= a * a * b * b
    m1 = (yy < (7 * h) // 10) & (xx >= (4 * w) // 10)
    r = h // 5
    m2 = np.zeros((h, w), dtype=bool)
    for cx, cy, rr in ((w // 2, h // 2, r), (w // 2 + r, h // 2 - r // 2, (3 * r) // 4), (w // 2 - r, h // 2 + r // 3, (2 * r) // 3)):
        m2 |= (xx - cx) ** 2 + (yy - cy) ** 2 <= rr * rr
    m2 &= (xx - w // 2) ** 2 + (yy - h // 2) ** 2 > (r // 3) ** 2
    return [(m.astype(np.uint8) * 255) for m in (m0, m1, m2)]


def write_tree(root, scans=(SCAN,), view_ids=VIEW_IDS, mask_list=None, h=H, w=W):
    """cameras/{vid:08d}_cam.txt and scan{N}/mask/{vid:03d}.png (three-channel PNGs, as DTU's) under root; returns the
    world-to-camera matrices."""
    cams = ring_cams(len(view_ids))
    mask_list = masks(h, w) if mask_list is None else mask_list
    os.makedirs(os.path.join(root, "cameras"), exist_ok=True)
    for vid, w2c in zip(view_ids, cams):
        write_cam(os.path.join(root, "cameras", f"{vid:08d}_cam.txt"), w2c, K, 425.0, 2.5)
    for scan in scans:
        os.makedirs(os.path.join(root, f"scan{scan}", "mask"), exist_ok=True)
        for vid, m in zip(view_ids, mask_list):
            Image.fromarray(np.stack([m, m, m], axis=-1)).save(os.path.join(root, f"scan{scan}", "mask", f"{vid:03d}.png"))
    return cams


def soup(n_vertices=8000, n_faces=16000, seed=5, h=H, w=W):
    """Seeded float64 vertices (world mm) and random faces: 70 % in a ball of 150 mm diameter around the origin, 10 % on rays
    through random pixels of a view, 12 % projecting up to 3 px outside one of a view's image borders (and up to 1 px inside),
    8 % behind a camera."""
    g = np.random.default_rng(seed)
    cams = ring_cams(3)
    n_ball = (70 * n_vertices) // 100
    n_pix = n_vertices // 10
    n_edge = (12 * n_vertices) // 100
    n_back = n_vertices - n_ball - n_pix - n_edge
    d = g.standard_normal((n_ball, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * (75.0 * g.random((n_ball, 1)) ** (1 / 3))

    def lift(view, u, v, depth):
        cam = np.stack([(u - K[0, 2]) / K[0, 0] * depth, (v - K[1, 2]) / K[1, 1] * depth, depth, np.ones_like(depth)], axis=1)
        return (cam @ np.linalg.inv(cams[view]).T)[:, :3]

    def lifted(n, u, v, depth):
        view = g.integers(0, 3, n)
        out = np.empty((n, 3))
        for i in range(3):
            s = view == i
            out[s] = lift(i, u[s], v[s], depth[s])
        return out

    pix = lifted(n_pix, g.uniform(0, w - 1, n_pix), g.uniform(0, h - 1, n_pix), g.uniform(520, 680, n_pix))
    side = g.integers(0, 4, n_edge)
    off = g.uniform(-1.0, 3.0, n_edge)                     # pixels beyond the border
    u = np.where(side == 0, -off, np.where(side == 1, (w - 1) + off, g.uniform(0, w - 1, n_edge)))
    v = np.where(side == 2, -off, np.where(side == 3, (h - 1) + off, g.uniform(0, h - 1, n_edge)))
    edge = lifted(n_edge, u, v, g.uniform(520, 680, n_edge))
    back = lifted(n_back, g.uniform(0, w - 1, n_back), g.uniform(0, h - 1, n_back), -g.uniform(100, 700, n_back))
    vertices = np.concatenate([ball, pix, edge, back])
    vertices = vertices[g.permutation(len(vertices))]
    faces = g.integers(0, len(vertices), (n_faces, 3)).astype(np.int64)
    return np.ascontiguousarray(vertices, dtype=np.float64), faces
