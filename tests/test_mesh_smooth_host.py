"""The host path of mesh smoothing (surf_amd.mesh_smooth, backend="host") against the rule of include/surf_hip.h (surf_smooth_*):
bit-equal to a plain-Python restatement that builds neighbour SETS face by face and sums them in ascending order (no keys, no
sort, no CSR), closed forms on a tetrahedron and a plane, the boundary rule case by case, the Taubin / Laplacian behaviour on a
noisy sphere, the displacement cap, the normals and every refusal.  Runs on the CPU."""
import numpy as np
import pytest

from surf_amd.mesh_smooth import (adjacency_host, boundary_flags, check_params, smooth_mesh, smooth_mesh_host, smooth_step,
                                  sum256_host, vertex_normals_host)
from tests.mesh_smooth_scenes import GRID_Z, MESHES, fan, grid_rim

SCHEDULES = {"laplacian": dict(lam=0.5, mu=None), "taubin": dict(lam=0.5, mu=-0.53)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def restate_topology(faces, n):
    """(neighbour sets, boundary flags): every face adds each of its DISTINCT undirected edges once."""
    nbrs, uses = [set() for _ in range(n)], {}
    for face in np.asarray(faces).tolist():
        a, b, c = face
        for edge in {frozenset(e) for e in ((a, b), (b, c), (c, a)) if e[0] != e[1]}:
            i, j = tuple(edge)
            nbrs[i].add(j)
            nbrs[j].add(i)
            uses[edge] = uses.get(edge, 0) + 1
    boundary = [False] * n
    for edge, count in uses.items():
        if count == 1:
            for i in edge:
                boundary[i] = True
    return nbrs, boundary


def restate(v32, faces, iterations, lam, mu, pin_boundary):
    """The issue's rule with Python floats (IEEE doubles, one rounding per operator) and np.float32 between the steps."""
    n = len(v32)
    nbrs, boundary = restate_topology(faces, n)
    order = [sorted(s) for s in nbrs]
    x = [[float(c) for c in p] for p in np.asarray(v32, np.float32).tolist()]
    for s in ([lam] * iterations if mu is None else [lam, mu] * iterations):
        new = []
        for i in range(n):
            if not order[i] or (pin_boundary and boundary[i]):
                new.append(x[i])
                continue
            row = []
            for a in range(3):
                S = 0.0
                for j in order[i]:
                    S = S + x[j][a]
                m = S / float(len(order[i]))
                row.append(float(np.float32(x[i][a] + s * (m - x[i][a]))))
            new.append(row)
        x = new
    return np.asarray(x, np.float64).astype(np.float32), np.asarray(boundary), np.asarray([len(s) for s in nbrs])


@pytest.mark.parametrize("pin", [True, False], ids=["pinned", "free"])
@pytest.mark.parametrize("kind", list(SCHEDULES))
@pytest.mark.parametrize("name", list(MESHES))
def test_host_equals_the_restatement(name, kind, pin):
    v, f = MESHES[name]
    want, boundary, degree = restate(v, f, 3, pin_boundary=pin, **SCHEDULES[kind])
    got, nrm, info = smooth_mesh(v, f, iterations=3, pin_boundary=pin, **SCHEDULES[kind])
    assert nrm is None and got.dtype == np.float32 and got.shape == v.shape
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).any(axis=1).sum())
    assert np.array_equal(boundary_flags(f, len(v)), boundary)
    assert np.array_equal(adjacency_host(f, len(v))[3], degree)
    assert info["vertices"] == len(v) and info["boundary_vertices"] == int(boundary.sum())
    assert info["isolated_vertices"] == int((degree == 0).sum()) and info["capped"] == 0
    moved = np.linalg.norm(got.astype(np.float64) - v.astype(np.float64), axis=1)
    assert abs(info["moved_max"] - moved.max()) <= 1e-12 * (1 + moved.max())
    assert abs(info["moved_rms"] - np.sqrt((moved ** 2).mean())) <= 1e-12 * (1 + moved.max())


def test_sum256_is_the_sequential_tree():
    g = np.random.default_rng(5)
    for count in (1, 2, 255, 256, 257, 256 * 256 + 3):
        q = g.uniform(0, 1, count)
        level = q.tolist()
        while len(level) > 1:
            nxt = []
            for lo in range(0, len(level), 256):
                s = 0.0
                for x in level[lo:lo + 256]:
                    s = s + x
                nxt.append(s)
            level = nxt
        assert sum256_host(q) == level[0], count


def test_zero_iterations_and_inputs_untouched():
    for name, (v, f) in MESHES.items():
        v_in, f_in = v.copy(), f.copy()
        got, _, info = smooth_mesh(v_in, f_in, iterations=0)
        assert np.array_equal(bits(got), bits(v)), name
        assert info["moved_max"] == 0.0 and info["moved_rms"] == 0.0
        smooth_mesh(v_in, f_in, iterations=2, normals=True, max_move=1e-3)
        assert np.array_equal(f_in, f) and f_in.dtype == f.dtype and np.array_equal(bits(v_in), bits(v)), name


def test_empty_meshes_return_the_input():
    v, f = MESHES["tetrahedron"]
    nrm = np.ones_like(v)
    got, n_out, info = smooth_mesh(v, f[:0], normals=nrm)
    assert np.array_equal(bits(got), bits(v)) and np.array_equal(n_out, nrm)
    assert info == {"vertices": 4, "boundary_vertices": 0, "isolated_vertices": 4, "moved_max": 0.0, "moved_rms": 0.0, "capped": 0}
    got, n_out, info = smooth_mesh(v[:0], f[:0])
    assert got.shape == (0, 3) and n_out is None and info["vertices"] == 0


def test_tetrahedron_lands_on_the_mean_of_the_other_three():
    v, f = MESHES["tetrahedron"]
    got, _, info = smooth_mesh(v, f, iterations=1, lam=1.0, mu=None)
    d = v.astype(np.float64)
    for i in range(4):
        others = [j for j in range(4) if j != i]
        mean = ((d[others[0]] + d[others[1]]) + d[others[2]]) / 3.0
        assert np.array_equal(bits(got[i]), bits(mean.astype(np.float32))), i
    assert info["boundary_vertices"] == 0 and info["isolated_vertices"] == 0


@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_plane_grid_keeps_its_plane(kind):
    """Sums of at most 2^29 equal fp32 values are exact in fp64, so the mean of equal z is that z and the step adds s * 0."""
    v, f = MESHES["grid"]
    rim = grid_rim()
    z = bits(np.full(len(v), GRID_Z, np.float32))
    free = smooth_mesh(v, f, iterations=10, pin_boundary=False, **SCHEDULES[kind])[0]
    pinned, _, info = smooth_mesh(v, f, iterations=10, pin_boundary=True, **SCHEDULES[kind])
    assert np.array_equal(bits(free[:, 2]), z) and np.array_equal(bits(pinned[:, 2]), z)
    assert np.array_equal(bits(pinned[rim]), bits(v[rim]))
    assert (bits(pinned[~rim])[:, :2] != bits(v[~rim])[:, :2]).any(axis=1).all()        # unevenly spaced: the interior moves
    assert (bits(free[rim])[:, :2] != bits(v[rim])[:, :2]).any(axis=1).all()
    assert info["boundary_vertices"] == int(rim.sum()) and info["isolated_vertices"] == 0


def test_boundary_flags():
    flags = lambda name: boundary_flags(MESHES[name][1], len(MESHES[name][0]))
    assert np.array_equal(flags("grid"), grid_rim())
    assert not flags("sphere").any() and not flags("tetrahedron").any()
    assert flags("triangle").all() and flags("two_triangles").all()           # the shared edge is interior, its ends are on the rim
    # faces (0,1,2), (2,1,3), (0,1,2): the edges of the face listed twice have two uses; 1-3 and 2-3 have one; 1-2 has three
    assert flags("twice").tolist() == [False, True, True, True]
    v, f = MESHES["twice"]
    assert not boundary_flags(f[[0, 2]], len(v)).any()
    # three faces on the edge 0-1: interior; every other edge has one face
    assert flags("triple_edge").tolist() == [True] * 5
    assert not boundary_flags(np.array([[0, 1, 2], [1, 0, 2], [0, 1, 2]], np.int32), 3).any()
    # (3,3,4) has the one edge 3-4, once; the unreferenced vertices are isolated, not boundary
    assert flags("degenerate").tolist() == [True] * 5
    assert flags("unreferenced").tolist() == [True, True, True, False, False, True]
    assert adjacency_host(MESHES["unreferenced"][1], 6)[3].tolist() == [2, 3, 3, 0, 0, 2]
    assert adjacency_host(MESHES["fan"][1], len(MESHES["fan"][0]))[3][0] == 5000 and not flags("fan")[0]


def volume(v, f):
    v = v.astype(np.float64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def test_taubin_denoises_without_shrinking_and_laplacian_shrinks():
    """The issue's table (uv_sphere(48, 64), sigma 0.01, seed 0, 10 iterations): Taubin radial std 0.00995 -> 0.0038 at 1.004 of
    the clean volume; Laplacian (lam 0.5) 0.0112 at 0.900.  The table's Laplacian row is what TWENTY steps give (0.0110 at 0.898
    here): its prototype ran two steps per iteration for both filters.  The rule's ten steps leave 0.0058 at 0.947, which still
    loses more than the 5 % the issue asserts."""
    clean, f = MESHES["sphere"]
    noisy, _ = MESHES["noisy_sphere"]
    std_in = np.linalg.norm(noisy.astype(np.float64), axis=1).std()
    assert 0.009 < std_in < 0.011
    taubin = smooth_mesh(noisy, f)[0]
    std_out = np.linalg.norm(taubin.astype(np.float64), axis=1).std()
    ratio = volume(taubin, f) / volume(clean, f)
    print(f"taubin: radial std {std_in:.5f} -> {std_out:.5f}, volume ratio {ratio:.4f}")
    assert std_out < 0.5 * std_in and abs(ratio - 1.0) < 0.02
    laplace = smooth_mesh(noisy, f, lam=0.5, mu=None)[0]
    ratio = volume(laplace, f) / volume(clean, f)
    print(f"laplacian: radial std {np.linalg.norm(laplace.astype(np.float64), axis=1).std():.5f}, volume ratio {ratio:.4f}")
    assert ratio < 0.95


def soup(n=200, m=400, seed=2):
    """Random triangles over random vertices in [-1, 1]^3: a Laplacian step moves a vertex by about the size of the mesh."""
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, (n, 3)).astype(np.float32), g.integers(0, n, (m, 3)).astype(np.int32)


def test_displacement_cap_bound():
    """|x - x0| <= M (1 + 2^-22) with M = 0.8 on vertices in [-1, 1]^3.  The capped position x0 + d r lies M (1 +- 2^-51) from x0 in
    fp64; its components are below 1 + M < 2 in magnitude, so rounding them to fp32 moves each by at most 2^-24, the position by
    at most sqrt(3) 2^-24 = 1.04e-7 < M 2^-22 = 1.9e-7.  (The rule rounds the POSITION to fp32, so the excess over M is
    2^-24 |x| per axis whatever M is: for M far below |x| it is not within M 2^-22 - test_displacement_cap_small_moves.)"""
    v, f = soup()
    M = 0.8
    free, _, info_free = smooth_mesh(v, f, iterations=3, lam=1.0, mu=None, pin_boundary=False)
    got, _, info = smooth_mesh(v, f, iterations=3, lam=1.0, mu=None, pin_boundary=False, max_move=M)
    d_free = np.linalg.norm(free.astype(np.float64) - v.astype(np.float64), axis=1)
    d = np.linalg.norm(got.astype(np.float64) - v.astype(np.float64), axis=1)
    print(f"largest move {d.max():.9f} = M (1 + {d.max() / M - 1:.3e}); without the cap {d_free.max():.4f}; capped {info['capped']}")
    assert d.max() <= M * (1 + 2.0 ** -22) and info["moved_max"] <= M * (1 + 2.0 ** -22)
    over = d_free > M
    assert 20 < info["capped"] == int(over.sum()) < len(v) and info_free["capped"] == 0
    assert np.array_equal(bits(got[~over]), bits(free[~over]))
    assert (d[over] >= M * (1 - 2.0 ** -22)).all()


def test_displacement_cap_small_moves():
    """M = 0.004 on the unit sphere: the cap holds to the fp32 rounding of the positions, sqrt(3) 2^-24 max |x| (see above), the
    count is that of the vertices the steps took further than M, and every other vertex keeps the uncapped run's bits."""
    v, f = MESHES["noisy_sphere"]
    M = 0.004
    free, _, info_free = smooth_mesh(v, f, lam=0.5, mu=None)
    got, _, info = smooth_mesh(v, f, lam=0.5, mu=None, max_move=M)
    d_free = np.linalg.norm(free.astype(np.float64) - v.astype(np.float64), axis=1)
    d = np.linalg.norm(got.astype(np.float64) - v.astype(np.float64), axis=1)
    assert info_free["moved_max"] > 2 * M and info_free["capped"] == 0
    slack = np.sqrt(3.0) * 2.0 ** -24 * float(np.abs(got).max())
    assert d.max() <= M * (1 + 2.0 ** -22) + slack and abs(info["moved_max"] - d.max()) < 1e-12
    over = d_free > M
    assert 0 < info["capped"] == int(over.sum()) < len(v)
    assert np.array_equal(bits(got[~over]), bits(free[~over]))
    assert (d[over] >= M * (1 - 2.0 ** -22) - slack).all()
    # capped vertices stay on the ray from where they started to where the steps took them
    ray = (free.astype(np.float64) - v.astype(np.float64))[over] / d_free[over, None]
    assert np.abs((got.astype(np.float64) - v.astype(np.float64))[over] - M * ray).max() < 1e-6
    assert smooth_mesh(v, f, lam=0.5, mu=None, max_move=10.0)[2]["capped"] == 0


def test_normals():
    v, f = MESHES["noisy_sphere"]
    x, nrm, _ = smooth_mesh(v, f, normals=True)
    assert nrm.dtype == np.float32 and nrm.shape == v.shape
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert np.abs(length - 1.0).max() <= 2.0 ** -22
    radial = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    outwards = np.einsum("ij,ij->i", nrm.astype(np.float64), radial)
    assert (outwards > 0).all() and outwards.mean() > 0.99
    assert np.array_equal(bits(nrm), bits(vertex_normals_host(x, f)))
    # given normals: the recomputed ones stay on their side
    same = smooth_mesh(v, f, normals=radial.astype(np.float32))[1]
    flipped = smooth_mesh(v, f, normals=(-radial).astype(np.float32))[1]
    assert np.array_equal(bits(same), bits(nrm)) and np.array_equal(bits(flipped), bits(-nrm))
    mixed = radial.astype(np.float32)
    mixed[::3] *= -1
    got = smooth_mesh(v, f, normals=mixed)[1]
    assert np.array_equal(bits(got[::3]), bits(-nrm[::3])) and np.array_equal(bits(got[1::3]), bits(nrm[1::3]))
    # a fan without area, and an unreferenced vertex
    fv, ff = fan(40, flat=True)
    assert not smooth_mesh(fv, ff, iterations=2, pin_boundary=False, normals=True)[1].any()
    uv, uf = MESHES["unreferenced"]
    un = smooth_mesh(uv, uf, normals=True)[1]
    assert not un[[3, 4]].any() and (np.abs(np.linalg.norm(un[[0, 1, 2, 5]].astype(np.float64), axis=1) - 1) <= 2.0 ** -22).all()


def test_refusals_name_the_value():
    v, f = MESHES["two_triangles"]
    for kwargs, match in ((dict(iterations=-1), "iterations.*-1"), (dict(iterations=10001), "iterations.*10001"),
                          (dict(iterations=2.5), "iterations.*2.5"), (dict(iterations=True), "iterations.*True"),
                          (dict(lam=0.0), "lam.*0.0"), (dict(lam=1.5), "lam.*1.5"), (dict(lam=float("nan")), "lam.*nan"),
                          (dict(mu=-0.5), "mu.*-0.5"), (dict(mu=0.3), "mu.*0.3"), (dict(mu=float("-inf")), "mu.*-inf"),
                          (dict(lam=0.9, mu=-0.53), "mu.*-0.53"),
                          (dict(max_move=0.0), "max_move.*0.0"), (dict(max_move=-1.0), "max_move.*-1.0"),
                          (dict(max_move=float("inf")), "max_move.*inf"), (dict(normals=np.zeros((3, 3), np.float32)), "normals")):
        with pytest.raises(ValueError, match=match):
            smooth_mesh(v, f, **kwargs)
    with pytest.raises(ValueError, match=r"face indices span \[0, 4\]"):
        smooth_mesh(v, np.array([[0, 1, 4]], np.int32))
    with pytest.raises(ValueError, match=r"face indices span \[-1, 2\]"):
        smooth_mesh(v, np.array([[0, -1, 2]], np.int32))
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="vertex 2 is not finite"):
            smooth_mesh(bad, f)
    with pytest.raises(ValueError, match="backend"):
        smooth_mesh(v, f, backend="gpu")
    with pytest.raises(ValueError, match="return_tensors"):
        smooth_mesh(v, f, return_tensors=True)
    with pytest.raises(ValueError, match="unknown key.*lambda"):
        check_params({"lambda": 0.5})
    assert check_params({}) == {"iterations": 10, "lam": 0.5, "mu": -0.53, "pin_boundary": True, "max_move": None}


def test_smooth_step_record():
    v, f = MESHES["sphere"]
    x, nrm, rec = smooth_step(v, f, {"iterations": 2, "max_move": 0.5})
    want, _, info = smooth_mesh_host(v, f, iterations=2, max_move=0.5)
    assert nrm is None and np.array_equal(bits(x), bits(want))
    assert set(rec) == {"iterations", "lam", "mu", "pin_boundary", "max_move", "ms"} | set(info)
    assert {k: rec[k] for k in info} == info and rec["iterations"] == 2 and rec["mu"] == -0.53 and rec["ms"] > 0
