"""Meshes shared by tests/test_mesh_denoise_host.py and tests/test_mesh_denoise_gpu.py: those of tests/mesh_smooth_scenes.py, fans
whose hub has just below, exactly and just above SURF_DENOISE_WAVE_ROW = 48 faces (the rows that the step kernels hand to the
whole wavefront), and the lattice cube with and without noise, on which the filter's claim is checked."""
import numpy as np

from tests.mesh_smooth_scenes import MESHES, big_sphere, fan            # noqa: F401  (re-exported)

WAVE_ROW = 48
FAN_DEGREES = (WAVE_ROW - 1, WAVE_ROW, WAVE_ROW + 1, 200)
BIG_CUBE = 74                                                           # 12 * 74^2 = 65,712 faces: more than 256 blocks of 256
LARGE = ("fan",)                                                        # MESHES too large for a plain-Python loop (hub of 5000)


def cube(k):
    """The surface of [0, k]^3 on the integer lattice, divided by k: every unit square is split along the diagonal from its (i, j)
    corner to its (i + 1, j + 1) corner, faces outward.  (vertices (6 k^2 + 2, 3) fp32 in lattice order, faces (12 k^2, 3) int32)."""
    idx = -np.ones((k + 1, k + 1, k + 1), np.int64)
    g = np.arange(k + 1)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    on = (x == 0) | (x == k) | (y == 0) | (y == k) | (z == 0) | (z == k)
    idx[on] = np.arange(int(on.sum()))
    v = (np.stack([x[on], y[on], z[on]], axis=1).astype(np.float64) / k).astype(np.float32)
    faces = []
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(k), np.arange(k), indexing="ij"))
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3                           # u x w points along +axis
        for side in (0, k):
            def at(di, dj):
                p = np.zeros((len(i), 3), np.int64)
                p[:, axis], p[:, u], p[:, w] = side, i + di, j + dj
                return idx[p[:, 0], p[:, 1], p[:, 2]]
            p00, p10, p11, p01 = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
            tri = np.concatenate([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)])
            faces.append(tri if side == k else tri[:, ::-1])
    return v, np.concatenate(faces).astype(np.int32)


def noisy_cube(k, sigma, seed):
    v, f = cube(k)
    return (v + np.random.default_rng(seed).normal(size=v.shape) * sigma / k).astype(np.float32), f


def cube_edge_vertices(k):
    """(6 k^2 + 2,) bool: the vertices of cube(k) on an edge of the cube (two or three coordinates at 0 or 1)."""
    v, _ = cube(k)
    return ((v == 0) | (v == 1)).sum(axis=1) >= 2


def face_normals(v, f):
    """(m, 3) fp64 unit normals (zero for a face without area)."""
    v = np.asarray(v, np.float64)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    length = np.linalg.norm(c, axis=1, keepdims=True)
    return np.divide(c, length, out=np.zeros_like(c), where=length > 0)


def mean_normal_error_deg(v, f, clean_v):
    """The mean angle, in degrees, between the face normals of (v, f) and of (clean_v, f)."""
    cos = np.clip(np.einsum("ij,ij->i", face_normals(v, f), face_normals(clean_v, f)), -1.0, 1.0)
    return float(np.degrees(np.arccos(cos)).mean())


def denoise_meshes():
    """name -> (vertices (n, 3) fp32, faces (m, 3) int32): MESHES and the meshes this module adds, the large ones excepted."""
    out = dict(MESHES)
    for d in FAN_DEGREES:
        out[f"fan{d}"] = fan(d)
    out["flat_fan"] = fan(40, flat=True)                                # every face degenerate
    out["cube8"] = cube(8)
    out["noisy_cube6"] = noisy_cube(6, 0.15, 0)
    out["noisy_cube8"] = noisy_cube(8, 0.2, 1)
    return out


SCENES = denoise_meshes()


def big_cube():
    return noisy_cube(BIG_CUBE, 0.15, 2)
