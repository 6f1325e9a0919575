"""The host path of mesh simplification (surf_amd/mesh_simplify.py, backend="host"; the rule is written in include/surf_hip.h
above the surf_simplify_* entry points) against a restatement written here in plain Python - dictionaries keyed by cell, face by
face, np.linalg.solve - and against bounds that follow from the rule.  tests/test_mesh_simplify_gpu.py compares the device path
with this one, array for array, on the meshes built here.

Tolerance of the restatement comparison: integer arrays and the set of surviving cells are equal; positions and normals differ by
at most one fp32 ulp.  The solve's conditioning is 2^20, so the two fp64 computations agree to about 2^-32 of a CELL and only
rounding-boundary flips of the fp32 cast can show.  The ulp is taken of the value, with one allowance: a position is the sum
centre + x cell of two terms of up to |centre| + cell / 2, and where they cancel (a vertex on the plane 0 of a lattice anchored
at 0 comes out as 3e-17 from one computation and 2e-16 from the other) the value's own ulp goes to nothing while the two fp64
computations still differ by their own error.  That error, 2^-32 (|centre| + cell) at the solve's conditioning, is subtracted
from the difference before it is measured in ulps: it is the restatement's own error, not a figure taken from the code under
test, and 2^-9 of an fp32 ulp wherever nothing cancels."""
import math

import numpy as np
import pytest
import torch

from surf_amd.mesh_simplify import HALF, cell_indices, simplify_mesh

BOX_LO, BOX_HI = (-0.31, -0.47, 0.12), (0.53, 0.29, 0.77)
BOX_CELLS = (0.05, 0.11, 0.23)
BOX_COUNTS = {0.05: (1344, 2684), 0.11: (240, 476), 0.23: (82, 160)}      # the issue's float64 prototype: vertices, faces


# ---- meshes -----------------------------------------------------------------------------------------------------------------

def grid_faces(nu, nv, base=0, flip=False):
    i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
    a = (base + i * nv + j).reshape(-1)
    quads = np.stack([a, a + nv, a + nv + 1, a + 1], axis=1)
    f = np.concatenate([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]])
    return (f[:, ::-1] if flip else f).astype(np.int32)


def tessellated_box(n=38, lo=BOX_LO, hi=BOX_HI):
    """Each side its own n x n grid (linspace in fp64, scaled, cast to fp32), seams unwelded, outward orientation."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    s = np.linspace(0.0, 1.0, n)
    verts, faces = [], []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            p = np.zeros((n, n, 3))
            p[..., axis] = hi[axis] if side else lo[axis]
            p[..., u] = (lo[u] + s * (hi[u] - lo[u]))[:, None]
            p[..., w] = (lo[w] + s * (hi[w] - lo[w]))[None, :]
            faces.append(grid_faces(n, n, base=len(verts) * n * n, flip=not side))
            verts.append(p.reshape(-1, 3))
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces)


def uv_sphere(stacks, slices, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """Welded UV sphere: two poles and stacks - 1 rings of `slices` vertices; 2 slices (stacks - 1) faces, outward."""
    th = np.pi * np.arange(1, stacks) / stacks
    ph = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None],
                     np.repeat(np.cos(th)[:, None], slices, 1)], axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + np.asarray(centre)
    south = 1 + (stacks - 1) * slices
    f = []
    for j in range(slices):
        k = (j + 1) % slices
        f.append((0, 1 + j, 1 + k))
        for i in range(stacks - 2):
            a, b = 1 + i * slices, 1 + (i + 1) * slices
            f += [(a + j, b + j, b + k), (a + j, b + k, a + k)]
        f.append((south, south - slices + k, south - slices + j))
    return v.astype(np.float32), np.asarray(f, np.int32)


def attributes(v, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal(v.shape).astype(np.float32), g.integers(0, 256, v.shape, dtype=np.uint8)


def case_meshes():
    """name -> (vertices, faces, cell): the inputs of the restatement case, shared with the device test."""
    g = np.random.default_rng(7)
    out = {}
    bv, bf = tessellated_box()
    out["box"] = (bv, bf, 0.11)
    sv, sf = uv_sphere(48, 96)
    out["sphere"] = (sv, sf, 0.2)
    # unreferenced vertices: some inside occupied cells (they pull the cell mean and the attributes), some in cells of their own
    extra = np.concatenate([sv[::37] * np.float32(0.999), g.uniform(-3, 3, (40, 3)).astype(np.float32)])
    out["unreferenced"] = (np.concatenate([extra[:20], sv, extra[20:]]), sf + 20, 0.2)
    # zero-area faces (collinear corners, coincident corners with different indices) and faces with a repeated index
    dv = np.concatenate([sv, sv[5:6], sv[5:6] + (sv[9:10] - sv[5:6]) * np.float32(2.0)])
    n0 = len(sv)
    df = np.concatenate([[(5, 9, 5), (3, 3, 3), (7, 7, 300)], sf[:700], [(5, n0, 200), (5, 9, n0 + 1), (100, 2000, 100)], sf[700:],
                         [(n0, 5, 9)]]).astype(np.int32)
    out["degenerate"] = (dv, df, 0.2)
    # two faces over the same three cells with opposite orientation, each cell holding two vertices
    ov = np.array([(0.1, 0.1, 0.1), (1.2, 0.1, 0.1), (0.1, 1.3, 0.2), (0.3, 0.2, 0.3), (1.4, 0.3, 0.2), (0.2, 1.1, 0.4),
                   (1.1, 1.2, 0.1), (2.5, 0.5, 0.5)], np.float32)
    out["opposite"] = (ov, np.array([(0, 1, 2), (5, 4, 3), (1, 6, 2), (4, 3, 5), (1, 7, 6), (2, 1, 0)], np.int32), 1.0)
    # vertices exactly on cell planes: two grids at right angles, coordinates multiples of 0.25 on both sides of 0
    t = np.arange(-4, 5) * 0.25
    p1 = np.stack(np.meshgrid(t, t, [-0.5], indexing="ij"), -1).reshape(-1, 3)
    p2 = np.stack(np.meshgrid([0.25], t, t, indexing="ij"), -1).reshape(-1, 3)
    out["planes"] = (np.concatenate([p1, p2]).astype(np.float32), np.concatenate([grid_faces(9, 9), grid_faces(9, 9, base=81)]), 0.25)
    for m in (0, 1, 255, 256, 257):
        out[f"m{m}"] = (sv, sf[1000:1000 + m], 0.1)
    cv, cf = uv_sphere(48, 96, 1.0, (2.0, 2.0, 2.0))
    out["one_cell"] = (cv, cf, 4.0)
    kv, kf = uv_sphere(8, 12)
    out["fine"] = (kv, kf, 0.02)
    return out


CASES = case_meshes()


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def restate(v32, faces, cell, normals, colors):
    """The issue's rule, face by face over dictionaries keyed by the cell's index triple."""
    v = np.asarray(v32, np.float32).astype(np.float64)
    cells = [tuple(int(math.floor(x / cell)) for x in p) for p in v]
    acc = {}
    for i, K in enumerate(cells):
        a = acc.setdefault(K, dict(A=np.zeros((3, 3)), b=np.zeros(3), n=0, u=np.zeros(3), col=np.zeros(3, np.int64), nrm=np.zeros(3)))
        centre = (np.array(K, np.float64) + 0.5) * cell
        a["n"] += 1
        a["u"] += (v[i] - centre) / cell
        a["col"] += colors[i].astype(np.int64)
        a["nrm"] += normals[i].astype(np.float64)
    for f in faces:
        if len({int(f[0]), int(f[1]), int(f[2])}) < 3:
            continue
        p0, p1, p2 = v[f[0]], v[f[1]], v[f[2]]
        c = np.cross(p1 - p0, p2 - p0)
        L = math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        if L == 0 or not math.isfinite(L):
            continue
        nrm, w = c / L, (L / 2) / (cell * cell)
        for k in range(3):
            K = cells[f[k]]
            q = (p0 - (np.array(K, np.float64) + 0.5) * cell) / cell
            acc[K]["A"] += w * np.outer(nrm, nrm)
            acc[K]["b"] += w * float(nrm @ q) * nrm
    kept, seen = [], set()
    for f in faces:
        tri = [cells[i] for i in f]
        if len(set(tri)) == 3 and frozenset(tri) not in seen:
            seen.add(frozenset(tri))
            kept.append(tri)
    used = sorted({K for tri in kept for K in tri})                      # ascending (ix, iy, iz) = ascending key
    number = {K: j for j, K in enumerate(used)}
    pos, nrm, col = [], [], []
    for K in used:
        a = acc[K]
        t, m = np.trace(a["A"]), a["u"] / a["n"]
        x = m if not t > 0 else np.linalg.solve(a["A"] + 2.0 ** -20 * t * np.eye(3), a["b"] + 2.0 ** -20 * t * m)
        pos.append(((np.array(K, np.float64) + 0.5) * cell + np.clip(x, -0.5, 0.5) * cell).astype(np.float32))
        ln = math.sqrt(float(a["nrm"] @ a["nrm"]))
        nrm.append((a["nrm"] / ln if ln > 0 and math.isfinite(ln) else np.zeros(3)).astype(np.float32))
        col.append(((2 * a["col"] + a["n"]) // (2 * a["n"])).astype(np.uint8))
    return {"vertices": np.array(pos, np.float32).reshape(-1, 3), "normals": np.array(nrm, np.float32).reshape(-1, 3),
            "colors": np.array(col, np.uint8).reshape(-1, 3),
            "faces": np.array([[number[K] for K in tri] for tri in kept], np.int32).reshape(-1, 3),
            "vertex_map": np.array([number.get(K, -1) for K in cells], np.int32), "keys": used}


def ulps32(a, b, slack=0.0):
    """max over the elements of max(|a - b| - slack, 0) in units of the fp32 ulp of the larger magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    mag = np.maximum(np.abs(a), np.abs(b)).astype(np.float32)
    return float((np.maximum(np.abs(a - b) - slack, 0.0) / np.spacing(mag).astype(np.float64)).max())


def output_keys(v32, cell, vmap, n_out):
    """The index triple of every output vertex's cell, from the input vertices that map to it."""
    idx, _ = cell_indices(v32, cell)
    keys = np.zeros((n_out, 3), np.int64)
    keys[vmap[vmap >= 0]] = idx[vmap >= 0]
    return keys


def run_host(name):
    v, f, cell = CASES[name]
    nrm, col = attributes(v, len(name))
    return (v, f, cell, nrm, col), simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True)


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_host_equals_the_restatement(name):
    (v, f, cell, nrm, col), got = run_host(name)
    want = restate(v, f, cell, nrm, col)
    gv, gf, gn, gc, gm = got
    assert gv.dtype == np.float32 and gf.dtype == np.int32 and gn.dtype == np.float32 and gc.dtype == np.uint8 and gm.dtype == np.int32
    assert gv.shape == want["vertices"].shape and gf.shape == want["faces"].shape, (gv.shape, gf.shape)
    assert np.array_equal(gf, want["faces"]) and np.array_equal(gm, want["vertex_map"]) and np.array_equal(gc, want["colors"])
    assert [tuple(k) for k in output_keys(v, cell, gm, len(gv))] == want["keys"]
    centre = (np.abs(np.asarray(want["keys"], np.float64).reshape(-1, 3)) + 1.5) * cell
    up, un = ulps32(gv, want["vertices"], slack=2.0 ** -32 * centre), ulps32(gn, want["normals"])
    print(f"{name}: {len(f)} -> {len(gf)} faces, {len(v)} -> {len(gv)} vertices; max ulps: position {up:.2f}, normal {un:.2f}, "
          f"position without the cancellation allowance {ulps32(gv, want['vertices']):.3g}")
    assert up <= 1.0 and un <= 1.0
    if name == "one_cell":
        assert len(gv) == 0 and len(gf) == 0 and (gm == -1).all()
    if name.startswith("m"):
        assert len(gf) <= int(name[1:])
    if name == "opposite":
        assert np.array_equal(gf, gm[f[[0, 2, 4]]])            # faces 1, 3 and 5 repeat face 0's cells: the lowest index stays
    if name == "fine":                                        # the input mesh up to renumbering
        assert len(gv) == len(v) and len(gf) == len(f) and sorted(gm) == list(range(len(v)))
        assert np.array_equal(gm[f], gf)
        assert ulps32(gv[gm], v, slack=2.0 ** -32 * (np.abs(v) + 2 * cell)) <= 1.0      # the same allowance where a coordinate is 0


def test_without_attributes_and_tuple_layout():
    v, f, cell = CASES["sphere"]
    nrm, col = attributes(v, 3)
    full = simplify_mesh(v, f, cell, normals=nrm, colors=col, return_map=True)
    bare = simplify_mesh(v, f.astype(np.int64), cell)
    assert len(bare) == 2 and np.array_equal(bare[0], full[0]) and np.array_equal(bare[1], full[1])
    only_c = simplify_mesh(torch.from_numpy(v).double(), torch.from_numpy(f), cell, colors=col)
    assert len(only_c) == 3 and np.array_equal(only_c[2], full[3]) and np.array_equal(only_c[0], full[0])
    with pytest.raises(ValueError, match="backend"):
        simplify_mesh(v, f, cell, backend="gpu")
    with pytest.raises(ValueError, match="return_tensors"):
        simplify_mesh(v, f, cell, return_tensors=True)
    with pytest.raises(ValueError, match="face indices"):
        simplify_mesh(v, np.array([[0, 1, len(v)]]), cell)


# ---- 2. edges stay edges ------------------------------------------------------------------------------------------------------

def box_distance(p, lo, hi):
    """Distance of points (k, 3) float64 to the SURFACE of the box [lo, hi]."""
    out = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inside = np.minimum(p - lo, hi - p).min(axis=1)
    return np.where(inside > 0, inside, out)


@pytest.mark.parametrize("cell", BOX_CELLS)
def test_edges_stay_edges(cell):
    """The counts equal the issue's float64 prototype (1344 / 2684, 240 / 476, 82 / 160)."""
    v, f = tessellated_box()
    assert v.shape == (8664, 3) and f.shape == (16428, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)          # the box as its fp32 vertices have it
    gv, gf, vmap = simplify_mesh(v, f, cell, return_map=True)
    d = box_distance(gv.astype(np.float64), lo, hi)
    # the cell-mean placement of the same clustering
    mean = np.zeros((len(gv), 3))
    np.add.at(mean, vmap[vmap >= 0], v[vmap >= 0].astype(np.float64))
    mean /= np.bincount(vmap[vmap >= 0], minlength=len(gv))[:, None]
    d_mean = box_distance(mean, lo, hi)
    print(f"cell {cell}: {len(gv)} vertices / {len(gf)} faces; max distance to the box: quadric {d.max():.3g}, cell mean {d_mean.max():.3g}")
    assert d.max() <= 4 * 2.0 ** -23
    assert d_mean.max() > 100 * max(d.max(), 1e-12)
    # closed 2-manifold of genus 0, outward faces
    e = np.sort(np.concatenate([gf[:, [0, 1]], gf[:, [1, 2]], gf[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all()
    assert len(gv) - len(counts) + len(gf) == 2
    p = gv.astype(np.float64)[gf]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((nrm * (p.mean(axis=1) - (lo + hi) / 2)).sum(axis=1) > 0).all()
    assert (len(gv), len(gf)) == BOX_COUNTS[cell]


# ---- 3. bounds that follow from the rule ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "sphere", "unreferenced", "degenerate", "planes", "fine"])
def test_bounds_of_the_rule(name):
    (v, f, cell, nrm, col), (gv, gf, gn, gc, gm) = run_host(name)
    idx = output_keys(v, cell, gm, len(gv)).astype(np.float64)
    lo, hi = (idx * cell).astype(np.float32), ((idx + 1.0) * cell).astype(np.float32)
    # inside the closed box of its cell, up to the fp32 rounding of the result (one ulp of the bound either way)
    assert (gv >= lo - np.spacing(np.abs(lo))).all() and (gv <= hi + np.spacing(np.abs(hi))).all()
    # hence within cell sqrt(3) of an input vertex (of one in its own cell)
    member = np.full(len(gv), -1)
    member[gm[gm >= 0]] = np.flatnonzero(gm >= 0)                # some input vertex of every output vertex's cell
    assert (member >= 0).all()
    assert (np.linalg.norm(gv - v[member].astype(np.float64), axis=1) <= cell * math.sqrt(3) * (1 + 1e-6)).all()
    assert (gf[:, 0] != gf[:, 1]).all() and (gf[:, 1] != gf[:, 2]).all() and (gf[:, 0] != gf[:, 2]).all()
    assert len(np.unique(np.sort(gf, axis=1), axis=0)) == len(gf)
    assert gf.min() == 0 and gf.max() == len(gv) - 1 and len(np.unique(gf)) == len(gv)       # every output vertex is referenced
    # vertex_map against faces: a kept face is the image of an input face, in input order
    mapped = gm[f]
    is_out = (mapped >= 0).all(axis=1)
    rows = {tuple(r): j for j, r in enumerate(gf.tolist())}
    first_seen = {}
    for position, r in enumerate(mapped[is_out].tolist()):
        j = rows.get(tuple(r))
        if j is not None:
            first_seen.setdefault(j, position)
    assert sorted(first_seen) == list(range(len(gf)))
    order = [first_seen[j] for j in range(len(gf))]
    assert order == sorted(order)
    n_len = np.linalg.norm(gn.astype(np.float64), axis=1)
    assert (np.abs(n_len - 1) < 1e-6).all()


def test_halves_simplified_apart_agree():
    """The lattice is anchored at the world origin, not at the mesh: a cell whose vertices (and so all their faces) belong to one
    half gets the same bits from the half alone as from the whole sphere."""
    v, f, cell = CASES["sphere"]
    whole_v, _, whole_map = simplify_mesh(v, f, cell, return_map=True)
    north = v[f].mean(axis=1)[:, 2] > 0
    in_half = [np.isin(np.arange(len(v)), f[sel]) for sel in (north, ~north)]
    _, key = cell_indices(v, cell)
    checked = 0
    for h, sel in enumerate((north, ~north)):
        ids = np.flatnonzero(in_half[h])
        renum = np.full(len(v), -1)
        renum[ids] = np.arange(len(ids))
        half_v, _, half_map = simplify_mesh(v[ids], renum[f[sel]].astype(np.int32), cell, return_map=True)
        mixed = np.unique(key[in_half[1 - h]])                       # cells that hold a vertex of the other half
        pure = in_half[h] & ~np.isin(key, mixed) & (whole_map >= 0)
        assert (half_map[renum[pure]] >= 0).all()
        assert np.array_equal(half_v[half_map[renum[pure]]], whole_v[whole_map[pure]])
        checked += len(np.unique(whole_map[pure]))
    print(f"{checked} of {len(whole_v)} output vertices lie in cells of one half")
    assert checked > len(whole_v) // 2


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------

def test_limits():
    v, f, _ = CASES["fine"]
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cell"):
            simplify_mesh(v, f, cell)
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite or lies outside"):
        simplify_mesh(bad, f, 0.1)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="not finite or lies outside"):
        simplify_mesh(bad, f, 0.1)
    far = v.copy()
    far[0, 0] = HALF * 0.5                                   # index 2^20: one past the last cell
    with pytest.raises(ValueError, match="not finite or lies outside"):
        simplify_mesh(far, f, 0.5)
    far[0, 0] = -HALF * 0.5 - 0.25                           # index -2^20 - 1
    with pytest.raises(ValueError, match="not finite or lies outside"):
        simplify_mesh(far, f, 0.5)
    far[0, 0] = -HALF * 0.5                                  # index -2^20: the first cell, allowed
    far[1, 0] = HALF * 0.5 - 0.25                            # index 2^20 - 1: the last
    simplify_mesh(far, f, 0.5)


# ---- 5. FusionVolume.extract_mesh(simplify_cell=...) -----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_extract_mesh_simplify_cell_host_backend(sparse):
    """Marching cubes runs on the GPU whatever the volume's backend, hence the mark; the simplification is the host path."""
    from surf_amd.fusion import FusionVolume
    from tests.test_fusion_sparse_host import sphere_scene
    axes, views, trunc = sphere_scene()
    vol = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=sparse)
    vol.integrate(views)
    v, t, c = vol.extract_mesh()
    cell = 3.0 / 128
    want = simplify_mesh(v, t, cell, colors=c)
    got = vol.extract_mesh(simplify_cell=cell)
    print(f"{len(t)} -> {len(got[1])} faces")
    assert 100 < len(got[1]) < len(t) // 3
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.uint8
    assert np.array_equal(got[0], want[0].astype(np.float64)) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- the scripts' flags and their shared step -------------------------------------------------------------------------------------

def test_scripts_accept_the_flags_and_share_one_step():
    import os
    import sys
    from surf_amd.mesh_simplify import simplify_step
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
    import dtu_chamfer
    import fuse_scene
    a = fuse_scene.parse_args(["--conf", "c", "--simplify_mm", "0.8", "--simplify_backend", "device"])
    assert a.simplify_mm == 0.8 and a.simplify_backend == "device"
    a = fuse_scene.parse_args(["--conf", "c"])
    assert a.simplify_mm is None and a.simplify_backend == "host"
    b = dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e", "--simplify_cell", "0.01"])
    assert b.simplify_cell == 0.01 and b.simplify_backend == "host"
    assert dtu_chamfer.parse_args(["--conf", "c", "--eval_dir", "e"]).simplify_cell is None
    v, f, cell = CASES["sphere"]
    nrm, col = attributes(v, 5)
    sv, sf, sn, sc, rec = simplify_step(v, f, cell, nrm, col)
    want = simplify_mesh(v, f, cell, normals=nrm, colors=col)
    assert all(np.array_equal(x, y) for x, y in zip((sv, sf, sn, sc), want))
    assert {k: rec[k] for k in rec if k != "ms"} == {"cell": cell, "vertices_in": len(v), "faces_in": len(f), "vertices_out": len(sv),
                                                     "faces_out": len(sf)} and rec["ms"] > 0
    sv2, sf2, sn2, sc2, _ = simplify_step(v, f, cell, colors=col)
    assert sn2 is None and np.array_equal(sc2, sc) and np.array_equal(sv2, sv)
    sv3, _, sn3, sc3, _ = simplify_step(v, f, cell, normals=nrm)
    assert sc3 is None and np.array_equal(sn3, sn)
