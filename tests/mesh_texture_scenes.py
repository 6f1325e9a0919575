"""Scenes shared by tests/test_mesh_texture_host.py and tests/test_mesh_texture_gpu.py.  Every mesh has planar faces, so the mesh is
the true surface: the centred lattice cubes cube(3) and cube(8) painted with a smooth analytic colour c(X); two parallel quads,
the smaller in front of the larger for the cameras on its side, each painted with a colour of its own; a mesh with every kind of
bad face (zero area, a NaN vertex, an index out of range) and an odd face count; a single face.  Cameras sit on a ring around the
origin and above it and look at it; their images are small, ragged and of two sizes.  The photographs and the depth maps of the
mesh are rendered here, in float64, by brute-force ray-triangle intersection."""
import functools

import numpy as np

from tests.mesh_denoise_scenes import cube

VIEW_COUNTS = (1, 3, 16, 17, 33)                                   # both sides of the 16-view launch boundary
SIZES = ((23, 31), (37, 53))                                       # (H, W), alternating over the cameras
BACKGROUND = 0.25                                                  # what a ray that hits nothing photographs
DEPTH_TOL = 0.3                                                    # world units; the quads stand 1.0 apart
MIN_COS = 0.4
N_CAMERAS = max(VIEW_COUNTS)


def colour(X):
    """The world's colour at points X (..., 3) float64: one low-frequency sinusoid per channel, inside [0.3, 0.7]."""
    X = np.asarray(X, np.float64)
    return np.stack([0.5 + 0.2 * np.sin(0.8 * X[..., 0] + 0.4 * X[..., 1] + 0.3),
                     0.5 + 0.2 * np.sin(0.7 * X[..., 1] - 0.5 * X[..., 2] + 1.1),
                     0.5 + 0.2 * np.sin(0.8 * X[..., 2] + 0.4 * X[..., 0] - 0.6)], axis=-1)


def front_paint(X):
    return colour(X) * np.array([0.3, 0.3, 0.3]) + np.array([0.65, 0.05, 0.05])            # red: (0.74 .. 0.86, 0.14 .. 0.26, ..)


def back_paint(X):
    return colour(X) * np.array([0.3, 0.3, 0.3]) + np.array([0.05, 0.05, 0.65])            # blue


PAINTS = (colour, front_paint, back_paint)


def _grid_quad(x, half, k):
    """A square of side 2 half in the plane X = x, facing +X, as a k x k grid of split cells."""
    g = np.linspace(-half, half, k + 1)
    yy, zz = np.meshgrid(g, g, indexing="ij")
    v = np.stack([np.full(yy.size, x), yy.reshape(-1), zz.reshape(-1)], axis=1)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(k), np.arange(k), indexing="ij"))
    p00, p10, p11, p01 = i * (k + 1) + j, (i + 1) * (k + 1) + j, (i + 1) * (k + 1) + j + 1, i * (k + 1) + j + 1
    return v, np.concatenate([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)])


def _centred_cube(k):
    v, f = cube(k)
    return (v - np.float32(0.5)).astype(np.float32), f


def _quads():
    vf, ff = _grid_quad(0.5, 0.5, 3)                              # the front quad: 18 faces
    vb, fb = _grid_quad(-0.5, 1.0, 4)                             # the back quad: 32 faces, twice as wide
    v = np.concatenate([vf, vb]).astype(np.float32)
    f = np.concatenate([ff, fb + len(vf)]).astype(np.int32)
    return v, f, np.concatenate([np.full(len(ff), 1), np.full(len(fb), 2)])


def _bad():
    v, f = _centred_cube(3)
    n = len(v)
    v = np.concatenate([v, np.array([[np.nan, 0.0, 0.0], [2.0, 2.0, 2.0]], np.float32)])
    extra = np.array([[0, 1, 1],                                  # zero area
                      [0, 1, n],                                  # a NaN vertex
                      [0, 1, n + 7],                              # an index past the vertices
                      [-1, 2, 3],                                 # a negative index
                      [5, 5, 5]], np.int32)                       # zero area again: 108 + 5 faces, an odd count
    return v, np.concatenate([f[:40], extra[:3], f[40:], extra[3:]]).astype(np.int32)


def _scene(v, f, paint=None):
    f = np.asarray(f, np.int32)
    return {"vertices": np.asarray(v, np.float32), "faces": f, "paint": np.zeros(len(f), np.int64) if paint is None else paint}


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> {vertices (n, 3) fp32, faces (m, 3) int32, paint (m,) index into PAINTS}."""
    return {"cube3": _scene(*_centred_cube(3)), "cube8": _scene(*_centred_cube(8)), "quads": _scene(*_quads()),
            "bad": _scene(*_bad()),
            "single": _scene(np.array([[0.5, -0.4, -0.3], [0.5, 0.5, -0.2], [0.4, 0.0, 0.6]], np.float32), [[0, 1, 2]])}


GROUND_TRUTH = ("cube3", "cube8", "quads")                         # the scenes whose baked colours are compared with the paint


def drawable_faces(scene):
    """(m,) bool: the faces a renderer can draw (indices in range, finite vertices, an area)."""
    v, f = scene["vertices"].astype(np.float64), scene["faces"].astype(np.int64)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    tri = v[np.where(ok[:, None], f, 0)]
    ok &= np.isfinite(tri).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    return ok & (area > 0)


@functools.lru_cache(maxsize=None)
def cameras():
    """N_CAMERAS cameras as (P (3, 4) fp32, (H, W)): on a ring of radius about 3 in the XY plane and 30 and 60 degrees above it,
    looking at the origin with Z up, no two alike."""
    out = []
    for k in range(N_CAMERAS):
        az = 0.4 + 2.399963 * k                                    # the golden angle: azimuths never repeat
        el = np.radians((0.0, 30.0, 60.0)[k % 3] + 2.0 * (k % 5))
        r = 3.0 + 0.1 * (k % 4)
        c = r * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        fwd = -c / np.linalg.norm(c)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])                           # world -> camera
        H, W = SIZES[k % 2]
        f = 1.05 * min(H, W)
        K = np.array([[f, 0.0, (W - 1) / 2 + 0.3], [0.0, f, (H - 1) / 2 - 0.2], [0.0, 0.0, 1.0]])
        out.append(((K @ np.concatenate([R, (-R @ c)[:, None]], axis=1)).astype(np.float32), (H, W)))
    return out


def ray_cast(scene, P, hw):
    """Brute force in float64: every pixel's ray against every drawable face (Moeller-Trumbore).  Returns {depth (H, W) z-depth of
    the nearest hit or 0, face (H, W) its index or -1, point (H, W, 3), edge (H, W) the smallest |barycentric| of any face whose
    plane the ray meets in front of the camera with the other two barycentrics >= -that: how near the ray passes to an edge}."""
    H, W = hw
    P = np.asarray(P, np.float64).reshape(3, 4)
    Minv = np.linalg.inv(P[:, :3])
    c = -Minv @ P[:, 3]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([xs.reshape(-1), ys.reshape(-1), np.ones(H * W)], axis=1) @ Minv.T            # X = c + z d has z-depth z
    keep = np.flatnonzero(drawable_faces(scene))
    tri = scene["vertices"].astype(np.float64)[scene["faces"][keep].astype(np.int64)]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(all="ignore"):
        pv = np.cross(d[:, None, :], e2[None, :, :])                                           # (pixels, faces, 3)
        det = (pv * e1[None]).sum(-1)
        tv = c[None, :] - a                                                                    # (faces, 3)
        u = (pv * tv[None]).sum(-1) / det
        qv = np.cross(tv, e1)                                                                  # (faces, 3)
        v = (d[:, None, :] * qv[None]).sum(-1) / det
        z = (qv * e2).sum(-1)[None, :] / det
        w = 1.0 - u - v
        front = np.isfinite(z) & (z > 0)
        lo = np.minimum(np.minimum(u, v), w)
        hit = front & (lo >= 0)
        mid = np.stack([u, v, w], axis=-1)
        second = np.sort(mid, axis=-1)[..., 1]
        near_edge = np.where(front & (second >= -np.abs(lo)), np.abs(lo), np.inf).min(axis=1)
    zz = np.where(hit, z, np.inf)
    best = zz.argmin(axis=1)
    depth = zz[np.arange(len(d)), best]
    found = np.isfinite(depth)
    depth = np.where(found, depth, 0.0)
    return {"depth": depth.reshape(H, W), "face": np.where(found, keep[best], -1).reshape(H, W),
            "point": (c[None, :] + depth[:, None] * d).reshape(H, W, 3), "edge": near_edge.reshape(H, W)}


@functools.lru_cache(maxsize=None)
def photograph(name, k):
    """(image (H, W, 3) fp32, depth (H, W) fp32, cast) of camera k looking at scene `name`: each hit pixel has the paint of its
    face at the hit point, every other pixel BACKGROUND."""
    scene = scenes()[name]
    P, hw = cameras()[k]
    cast = ray_cast(scene, P, hw)
    image = np.full(hw + (3,), BACKGROUND)
    for p, paint in enumerate(PAINTS):
        sel = (cast["face"] >= 0) & (scene["paint"][np.maximum(cast["face"], 0)] == p)
        image[sel] = paint(cast["point"][sel])
    return image.astype(np.float32), cast["depth"].astype(np.float32), cast


def views_of(name, count):
    """(TextureViews, mesh depth maps) of the first `count` cameras for scene `name`."""
    from surf_amd.mesh_texture import TextureView
    shots = [photograph(name, k) for k in range(count)]
    return [TextureView(cameras()[k][0], shots[k][0]) for k in range(count)], [s[1] for s in shots]


def vertex_colours(name):
    """(n, 3) uint8: a colour per vertex, from its index alone (a NaN vertex has one too)."""
    n = len(scenes()[name]["vertices"])
    i = np.arange(n)
    return np.stack([(37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256], axis=1).astype(np.uint8)
