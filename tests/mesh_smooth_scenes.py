"""Meshes shared by tests/test_mesh_smooth_host.py and tests/test_mesh_smooth_gpu.py: the smallest that cross each edge of the
smoothing rule (include/surf_hip.h, surf_smooth_*) and of the step kernel (one vertex per lane, 256 per block, vertices of more
than SURF_SMOOTH_WAVE_DEGREE = 32 neighbours summed by the wave)."""
import numpy as np

from tests.test_mesh_simplify_host import grid_faces, uv_sphere

GRID = (17, 23)
GRID_Z = 0.37
HUB_DEGREE = 5000


def grid_mesh(nu=GRID[0], nv=GRID[1], z=GRID_Z):
    """An open nu x nv grid on the plane z, unevenly spaced so that the interior moves under a step."""
    g = np.random.default_rng(3)
    x = np.cumsum(g.uniform(0.5, 1.5, nu))
    y = np.cumsum(g.uniform(0.5, 1.5, nv))
    v = np.stack([np.repeat(x, nv), np.tile(y, nu), np.full(nu * nv, z)], axis=1).astype(np.float32)
    return v, grid_faces(nu, nv)


def grid_rim(nu=GRID[0], nv=GRID[1]):
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    return ((i == 0) | (i == nu - 1) | (j == 0) | (j == nv - 1)).reshape(-1)


def fan(degree=HUB_DEGREE, flat=False):
    """A closed fan: hub 0 at height 0.3 over a wavy ring of `degree` vertices.  flat: every vertex on one line (zero area)."""
    t = 2 * np.pi * np.arange(degree) / degree
    if flat:
        ring = np.stack([1.0 + np.arange(degree), np.zeros(degree), np.zeros(degree)], axis=1)
        hub = [[0.0, 0.0, 0.0]]
    else:
        r = 1.0 + 0.1 * np.cos(7 * t)
        ring = np.stack([r * np.cos(t), r * np.sin(t), 0.05 * np.sin(5 * t)], axis=1)
        hub = [[0.01, -0.02, 0.3]]
    v = np.concatenate([hub, ring]).astype(np.float32)
    k = np.arange(degree)
    f = np.stack([np.zeros(degree, np.int64), 1 + k, 1 + (k + 1) % degree], axis=1).astype(np.int32)
    return v, f


def strip(n_vertices):
    """A triangle strip of n_vertices vertices (n_vertices - 2 faces) that zigzags in all three axes."""
    k = np.arange(n_vertices)
    v = np.stack([0.5 * k, (k % 2) + 0.1 * np.sin(0.7 * k), 0.2 * np.cos(0.3 * k)], axis=1).astype(np.float32)
    f = np.stack([k[:-2], k[1:-1], k[2:]], axis=1)
    f[1::2] = f[1::2][:, [1, 0, 2]]
    return v, f.astype(np.int32)


def noisy_sphere(stacks=48, slices=64, sigma=0.01, seed=0):
    v, f = uv_sphere(stacks, slices)
    v = v.astype(np.float64)
    g = np.random.default_rng(seed)
    return (v + g.normal(0.0, sigma, (len(v), 1)) * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), f


def small_meshes():
    """name -> (vertices (n, 3) fp32, faces (m, 3) int32)."""
    g = np.random.default_rng(11)
    out = {}
    out["triangle"] = (g.standard_normal((3, 3)).astype(np.float32), np.array([[0, 1, 2]], np.int32))
    out["two_triangles"] = (g.standard_normal((4, 3)).astype(np.float32), np.array([[0, 1, 2], [2, 1, 3]], np.int32))
    out["tetrahedron"] = (np.array([[1, 1, 1], [1, -1, -1.5], [-1, 1.25, -1], [-1.75, -1, 1]], np.float32),
                          np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32))
    out["unreferenced"] = (g.standard_normal((6, 3)).astype(np.float32), np.array([[0, 1, 2], [2, 1, 5]], np.int32))     # 3 and 4
    out["degenerate"] = (g.standard_normal((5, 3)).astype(np.float32), np.array([[0, 1, 2], [3, 3, 4], [2, 1, 3]], np.int32))
    out["twice"] = (g.standard_normal((4, 3)).astype(np.float32), np.array([[0, 1, 2], [2, 1, 3], [0, 1, 2]], np.int32))
    out["triple_edge"] = (g.standard_normal((5, 3)).astype(np.float32), np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32))
    out["grid"] = grid_mesh()
    out["fan"] = fan()
    for k in (255, 256, 257):
        out[f"strip{k}"] = strip(k)
    out["sphere"] = uv_sphere(48, 64)
    out["noisy_sphere"] = noisy_sphere()
    return out


MESHES = small_meshes()


def big_sphere():
    """About 300 k faces with radial noise: 589 blocks of 256 vertices, several rounds of workgroups on the device."""
    return noisy_sphere(388, 388, 0.0005, 1)
