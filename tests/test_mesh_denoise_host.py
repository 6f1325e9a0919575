"""The host path of mesh denoising (surf_amd.mesh_denoise, backend="host") against the rule of include/surf_hip.h (surf_denoise_*):
bit-equal to a plain-Python restatement of rules 1 to 6 (Python floats are IEEE doubles, one rounding per operator; np.float32
where the rule rounds), the neighbour rule against brute force, the fixed points that the umbrella operator does not have, the
denoising claim on noisy cubes against smooth_mesh, the cap, the pinned boundary and every refusal.  Runs on the CPU."""
import itertools
import math

import numpy as np
import pytest

from surf_amd.mesh_denoise import (check_params, denoise_mesh, denoise_mesh_host, denoise_step, face_neighbours_host)
from surf_amd.mesh_smooth import smooth_mesh
from tests.mesh_denoise_scenes import (LARGE, SCENES, cube, cube_edge_vertices, mean_normal_error_deg, noisy_cube)
from tests.mesh_smooth_scenes import MESHES, grid_rim
from tests.test_mesh_smooth_host import restate_topology, soup

SMALL = [name for name in SCENES if name not in LARGE]
ITERATIONS = [(0, 0), (0, 3), (3, 0), (3, 3)]
GIVEN_SIGMA_S = 0.3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f32(x):
    return float(np.float32(x))


def tree256(values):
    level = list(values)
    while len(level) > 1:
        nxt = []
        for lo in range(0, len(level), 256):
            s = 0.0
            for x in level[lo:lo + 256]:
                s = s + x
            nxt.append(s)
        level = nxt
    return level[0]


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def restate_neighbours(faces):
    """Rule 3, face by face: N(f) as a list, from per-vertex corner lists in (face, corner) order."""
    corners = {}
    for g, face in enumerate(faces):
        for j, v in enumerate(face):
            corners.setdefault(v, []).append((g, j))
    out = []
    for face in faces:
        row = []
        for k in range(3):
            v = face[k]
            if v in face[:k]:
                continue
            for g, j in corners[v]:
                if any(u in faces[g] for u in face[:k]) or v in faces[g][:j]:
                    continue
                row.append(g)
        out.append(row)
    return out


class Restatement:
    """Rules 1 to 6 with Python floats for one mesh; the stages are kept so that the settings that share one pay for it once."""

    def __init__(self, v32, faces):
        self.n = len(v32)
        self.x0 = [[float(c) for c in p] for p in np.asarray(v32, np.float32).tolist()]
        self.faces = np.asarray(faces).tolist()
        self.boundary = restate_topology(faces, self.n)[1]
        self.records, sides = [], []
        for a, b, c in self.faces:
            p0, p1, p2 = self.x0[a], self.x0[b], self.x0[c]
            e1 = [p1[t] - p0[t] for t in range(3)]
            e2 = [p2[t] - p0[t] for t in range(3)]
            F = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            L2 = (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2]
            if L2 == 0 or not math.isfinite(L2):
                self.records.append(None)                               # degenerate
            else:
                L = math.sqrt(L2)
                self.records.append(([f32(F[t] / L) for t in range(3)], f32(0.5 * L),
                                     [f32(((p0[t] + p1[t]) + p2[t]) / 3.0) for t in range(3)]))
            for s, e in ((p0, p1), (p1, p2), (p2, p0)):
                d = [e[t] - s[t] for t in range(3)]
                sides.append(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        self.mean_side = tree256(sides) / float(3 * len(self.faces))
        self.neighbours = restate_neighbours(self.faces)
        self._normals = {}

    def normals(self, iterations, sigma_r, sigma_s):
        key = (iterations, sigma_r, sigma_s)
        if key not in self._normals:
            i_s, i_r = 1.0 / (9.0 * sigma_s * sigma_s), 1.0 / (9.0 * sigma_r * sigma_r)
            nrm = [None if r is None else r[0] for r in self.records]
            for _ in range(iterations):
                new = []
                for f, row in enumerate(self.neighbours):
                    if self.records[f] is None:
                        new.append(None)
                        continue
                    S = [0.0, 0.0, 0.0]
                    for g in row:
                        if self.records[g] is None:                     # weight 0 through its area: adds +0 to a sum that is not -0
                            continue
                        d = [self.records[g][2][t] - self.records[f][2][t] for t in range(3)]
                        us = 1.0 - ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * i_s
                        e = [nrm[g][t] - nrm[f][t] for t in range(3)]
                        ur = 1.0 - ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * i_r
                        if us <= 0 or ur <= 0:
                            continue
                        w = (self.records[g][1] * ((us * us) * (us * us))) * ((ur * ur) * (ur * ur))
                        S = [S[t] + w * nrm[g][t] for t in range(3)]
                    L2 = (S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]
                    if L2 == 0 or not math.isfinite(L2):
                        new.append(nrm[f])
                    else:
                        L = math.sqrt(L2)
                        new.append([f32(S[t] / L) for t in range(3)])
                nrm = new
            self._normals[key] = nrm
        return self._normals[key]

    def run(self, normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary, max_move):
        sigma_s = self.mean_side if sigma_s is None else sigma_s
        nrm = self.normals(normal_iterations, sigma_r, sigma_s)
        corners = [[] for _ in range(self.n)]
        for g, face in enumerate(self.faces):
            for v in face:
                if nrm[g] is not None:
                    corners[v].append(g)
        x = self.x0
        for _ in range(vertex_iterations):
            new = []
            for i in range(self.n):
                if not corners[i] or (pin_boundary and self.boundary[i]):
                    new.append(x[i])
                    continue
                T = [0.0, 0.0, 0.0]
                for g in corners[i]:
                    a, b, c = self.faces[g]
                    cen = [((x[a][t] + x[b][t]) + x[c][t]) / 3.0 for t in range(3)]
                    n = nrm[g]
                    d = ((cen[0] - x[i][0]) * n[0] + (cen[1] - x[i][1]) * n[1]) + (cen[2] - x[i][2]) * n[2]
                    T = [T[t] + n[t] * d for t in range(3)]
                new.append([f32(x[i][t] + T[t] / float(len(corners[i]))) for t in range(3)])
            x = new
        q, capped = [], 0
        out = []
        for i in range(self.n):
            p = x[i]
            d = [p[t] - self.x0[i][t] for t in range(3)]
            qi = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if max_move is not None and qi > max_move * max_move:
                r = max_move / math.sqrt(qi)
                p = [f32(self.x0[i][t] + d[t] * r) for t in range(3)]
                d = [p[t] - self.x0[i][t] for t in range(3)]
                qi = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                capped += 1
            out.append(p)
            q.append(qi)
        info = {"vertices": self.n, "faces": len(self.faces), "degenerate_faces": sum(r is None for r in self.records),
                "boundary_vertices": sum(self.boundary), "sigma_s": sigma_s, "sigma_r": sigma_r, "moved_max": math.sqrt(max(q)),
                "moved_rms": math.sqrt(tree256(q) / float(self.n)), "capped": capped}
        return np.asarray(out, np.float64).astype(np.float32), info


def a_cap(v, f):
    """A cap that some vertices hit and others do not: the median movement of the free run without one (1e-3 if nothing moves)."""
    ref = denoise_mesh(v, f, normal_iterations=3, vertex_iterations=3, pin_boundary=False)[0]
    return float(np.median(np.linalg.norm(ref.astype(np.float64) - v.astype(np.float64), axis=1))) or 1e-3


@pytest.mark.parametrize("name", SMALL)
def test_host_equals_the_restatement(name):
    v, f = SCENES[name]
    restated = Restatement(v, f)
    cap = a_cap(v, f)
    for (ni, vi), pin, max_move, sigma_s in itertools.product(ITERATIONS, (True, False), (None, cap), (None, GIVEN_SIGMA_S)):
        kw = dict(normal_iterations=ni, vertex_iterations=vi, sigma_r=0.35, sigma_s=sigma_s, pin_boundary=pin, max_move=max_move)
        want, want_info = restated.run(**kw)
        got, nrm, info = denoise_mesh(v, f, **kw)
        what = (name, kw)
        assert nrm is None and got.dtype == np.float32 and got.shape == v.shape, what
        assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).any(axis=1).sum()))
        assert info == want_info, (what, info, want_info)               # the floats compare with ==: the same bits
        if vi == 0:
            assert np.array_equal(bits(got), bits(v)) and info["moved_max"] == 0.0, what


def test_every_face_degenerate_leaves_the_positions():
    v, f = SCENES["flat_fan"]
    got, nrm, info = denoise_mesh(v, f, pin_boundary=False, normals=True)
    assert np.array_equal(bits(got), bits(v)) and not nrm.any()
    assert info["degenerate_faces"] == len(f) and info["moved_max"] == 0.0 and info["sigma_s"] > 0


@pytest.mark.parametrize("name", ["triangle", "two_triangles", "tetrahedron", "unreferenced", "degenerate", "twice", "triple_edge",
                                  "grid", "strip257", "fan47", "flat_fan", "cube8"])
def test_neighbour_rule(name):
    """N(f) as a set is the brute-force vertex-sharing set, it has no duplicates, and its order is the rule's."""
    v, f = SCENES[name]
    rows, nbr = face_neighbours_host(f, len(v))
    faces = f.tolist()
    assert rows.shape == (len(f) + 1,) and rows[0] == 0 and rows[-1] == len(nbr) and nbr.dtype == np.int32
    sets = [set(face) for face in faces]
    want_order = restate_neighbours(faces)
    for i in range(len(faces)):
        got = nbr[rows[i]:rows[i + 1]].tolist()
        assert len(got) == len(set(got)), (name, i)
        assert set(got) == {g for g in range(len(faces)) if sets[g] & sets[i]}, (name, i)
        assert i in got and got == want_order[i], (name, i)
    # the order in words, on a face of the grid: first the faces at slot 0 ascending, then the new ones at slot 1, then at slot 2
    if name == "grid":
        i = len(faces) // 2
        got = nbr[rows[i]:rows[i + 1]].tolist()
        at = [sorted(g for g in range(len(faces)) if faces[i][k] in faces[g]) for k in range(3)]
        assert got == at[0] + [g for g in at[1] if g not in at[0]] + [g for g in at[2] if g not in at[0] and g not in at[1]]


@pytest.mark.parametrize("name", ["cube8", "grid"])
def test_fixed_points_that_taubin_moves(name):
    """A clean cube and a planar, unevenly spaced grid come back bit for bit, with free boundaries too; smooth_mesh(iterations=10)
    of the same inputs moves them by more than 1e-2 (the existing code's movement, asserted so that the fixed point says
    something)."""
    v, f = SCENES[name]
    for pin in (True, False):
        got, _, info = denoise_mesh(v, f, pin_boundary=pin)
        assert np.array_equal(bits(got), bits(v)), (name, pin)
        assert info["moved_max"] == 0.0 and info["moved_rms"] == 0.0 and info["degenerate_faces"] == 0
    taubin = smooth_mesh(v, f, iterations=10)[2]
    print(f"{name}: smooth_mesh(iterations=10) moves it by {taubin['moved_max']:.4f}")
    assert taubin["moved_max"] > 1e-2


@pytest.mark.parametrize("k,sigma,seed", [(6, 0.15, 0), (8, 0.2, 1)])
def test_denoises_a_cube_and_keeps_its_edges(k, sigma, seed):
    """Defaults against smooth_mesh(iterations=10) on a noisy cube: the mean face-normal error against the clean cube below half of
    Taubin's (the prototype's ratios were 0.15 and 0.20: a margin of 2.5 for roundings fixed differently), and the RMS distance of
    the cube-edge vertices from where they belong below Taubin's."""
    clean, f = cube(k)
    noisy, _ = noisy_cube(k, sigma, seed)
    edge = cube_edge_vertices(k)
    taubin = smooth_mesh(noisy, f, iterations=10)[0]
    got = denoise_mesh(noisy, f)[0]
    err = {name: mean_normal_error_deg(x, f, clean) for name, x in (("noisy", noisy), ("taubin", taubin), ("bilateral", got))}
    rms = {name: float(np.sqrt((np.linalg.norm(x[edge].astype(np.float64) - clean[edge], axis=1) ** 2).mean()))
           for name, x in (("noisy", noisy), ("taubin", taubin), ("bilateral", got))}
    print(f"cube({k}), sigma {sigma}/k, seed {seed}: normal error (deg) {err}; edge RMS {rms}")
    assert err["bilateral"] < 0.5 * err["taubin"]
    assert rms["bilateral"] < rms["taubin"]


def test_displacement_cap_bound():
    """As tests/test_mesh_smooth_host.py::test_displacement_cap_bound, where the bound M (1 + 2^-22) can be asserted: vertices in
    [-1, 1]^3, M = 0.8, so that rounding the capped position to fp32 moves it by at most sqrt(3) 2^-24 < M 2^-22.  The soup is
    denoised with a wide sigma_r so that its vertices travel; the vertices the cap did not take keep the free run's bits."""
    v, f = soup()
    M = 0.8
    kw = dict(normal_iterations=2, vertex_iterations=20, sigma_r=2.0, sigma_s=2.0, pin_boundary=False)
    free, _, info_free = denoise_mesh(v, f, **kw)
    got, _, info = denoise_mesh(v, f, max_move=M, **kw)
    d_free = np.linalg.norm(free.astype(np.float64) - v.astype(np.float64), axis=1)
    d = np.linalg.norm(got.astype(np.float64) - v.astype(np.float64), axis=1)
    print(f"largest move {d.max():.9f} = M (1 + {d.max() / M - 1:.3e}); without the cap {d_free.max():.4f}; capped {info['capped']}")
    assert d.max() <= M * (1 + 2.0 ** -22) and info["moved_max"] <= M * (1 + 2.0 ** -22)
    over = d_free > M
    assert 0 < info["capped"] == int(over.sum()) < len(v) and info_free["capped"] == 0
    assert np.array_equal(bits(got[~over]), bits(free[~over]))
    assert (d[over] >= M * (1 - 2.0 ** -22)).all()


def test_pinned_boundary_keeps_its_bits():
    v, f = MESHES["grid"]
    noisy = v.copy()
    noisy[:, 2] += np.random.default_rng(4).normal(0.0, 0.05, len(v)).astype(np.float32)
    rim = grid_rim()
    pinned, _, info = denoise_mesh(noisy, f)
    free = denoise_mesh(noisy, f, pin_boundary=False)[0]
    assert np.array_equal(bits(pinned[rim]), bits(noisy[rim])) and info["boundary_vertices"] == int(rim.sum())
    assert (bits(pinned[~rim]) != bits(noisy[~rim])).any(axis=1).all()
    assert (bits(free[rim]) != bits(noisy[rim])).any(axis=1).mean() > 0.9
    assert np.abs(pinned[~rim, 2] - v[~rim, 2]).std() < 0.5 * np.abs(noisy[~rim, 2] - v[~rim, 2]).std()


def test_normals_inputs_and_empty_meshes():
    from surf_amd.mesh_smooth import vertex_normals_host
    v, f = SCENES["noisy_cube8"]
    v_in, f_in = v.copy(), f.copy()
    x, nrm, _ = denoise_mesh(v_in, f_in, normals=True)
    assert np.array_equal(f_in, f) and np.array_equal(bits(v_in), bits(v))              # inputs untouched
    assert nrm.dtype == np.float32 and np.array_equal(bits(nrm), bits(vertex_normals_host(x, f)))
    flipped = denoise_mesh(v, f, normals=-nrm)[1]
    assert np.array_equal(bits(flipped), bits(-nrm))
    got, n_out, info = denoise_mesh(v, f[:0], normals=nrm, sigma_s=0.25)
    assert np.array_equal(bits(got), bits(v)) and np.array_equal(n_out, nrm)
    assert info == {"vertices": len(v), "faces": 0, "degenerate_faces": 0, "boundary_vertices": 0, "sigma_s": 0.25, "sigma_r": 0.35,
                    "moved_max": 0.0, "moved_rms": 0.0, "capped": 0}
    got, n_out, info = denoise_mesh(v[:0], f[:0])
    assert got.shape == (0, 3) and n_out is None and info["vertices"] == 0 and info["sigma_s"] is None


def test_refusals_name_the_value():
    v, f = MESHES["two_triangles"]
    for kwargs, match in ((dict(normal_iterations=-1), "normal_iterations.*-1"), (dict(normal_iterations=10001), "normal_iterations.*10001"),
                          (dict(vertex_iterations=2.5), "vertex_iterations.*2.5"), (dict(vertex_iterations=True), "vertex_iterations.*True"),
                          (dict(sigma_r=0.0), "sigma_r.*0.0"), (dict(sigma_r=float("nan")), "sigma_r.*nan"),
                          (dict(sigma_r=None), "sigma_r.*None"), (dict(sigma_s=-1.0), "sigma_s.*-1.0"),
                          (dict(sigma_s=float("inf")), "sigma_s.*inf"), (dict(sigma_s=1e-200), "sigma_s.*1e-200"),
                          (dict(max_move=0.0), "max_move.*0.0"), (dict(max_move=float("inf")), "max_move.*inf"),
                          (dict(normals=np.zeros((3, 3), np.float32)), "normals")):
        with pytest.raises(ValueError, match=match):
            denoise_mesh(v, f, **kwargs)
    with pytest.raises(ValueError, match=r"face indices span \[0, 4\]"):
        denoise_mesh(v, np.array([[0, 1, 4]], np.int32))
    for bad_value in (np.nan, np.inf):
        bad = v.copy()
        bad[2, 1] = bad_value
        with pytest.raises(ValueError, match="denoise_mesh: vertex 2 is not finite"):
            denoise_mesh(bad, f)
    with pytest.raises(ValueError, match="mean side length.*0.0"):
        denoise_mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match="backend"):
        denoise_mesh(v, f, backend="gpu")
    with pytest.raises(ValueError, match="return_tensors"):
        denoise_mesh(v, f, return_tensors=True)
    with pytest.raises(ValueError, match="unknown key.*iterations"):
        check_params({"iterations": 5})
    assert check_params({}) == {"normal_iterations": 10, "vertex_iterations": 10, "sigma_r": 0.35, "sigma_s": None,
                                "pin_boundary": True, "max_move": None}


def test_denoise_step_record():
    v, f = SCENES["noisy_cube6"]
    x, nrm, rec = denoise_step(v, f, {"normal_iterations": 2, "max_move": 0.5})
    want, _, info = denoise_mesh_host(v, f, normal_iterations=2, max_move=0.5)
    assert nrm is None and np.array_equal(bits(x), bits(want))
    assert set(rec) == {"normal_iterations", "vertex_iterations", "sigma_r", "pin_boundary", "max_move", "ms"} | set(info)
    assert {k: rec[k] for k in info} == info and rec["normal_iterations"] == 2 and rec["vertex_iterations"] == 10 and rec["ms"] > 0
    assert rec["sigma_s"] == info["sigma_s"] > 0


# ---- the scripts' flags (no GPU: the flag parsing and the order of the mesh steps) ------------------------------------------------

def _script(name):
    import os
    import sys
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    return __import__(name)


def test_script_flags_become_the_argument_dict():
    import argparse
    fuse_scene, dtu_chamfer = _script("fuse_scene"), _script("dtu_chamfer")
    base = ["--conf", "x.conf", "--scan", "24"]
    assert fuse_scene.denoise_params(fuse_scene.parse_args(base)) is None
    got = fuse_scene.denoise_params(fuse_scene.parse_args(base + ["--denoise_iters", "5"]))
    assert got == {**check_params({}), "normal_iterations": 5}
    got = fuse_scene.denoise_params(fuse_scene.parse_args(base + [
        "--denoise_iters", "4", "--denoise_vertex_iters", "7", "--denoise_sigma_r", "0.5", "--denoise_sigma_s_mm", "0.8",
        "--denoise_max_move_mm", "1.5", "--denoise_free_boundary"]))
    assert got == {"normal_iterations": 4, "vertex_iterations": 7, "sigma_r": 0.5, "sigma_s": 0.8, "pin_boundary": False, "max_move": 1.5}
    with pytest.raises(SystemExit, match="fuse_scene: denoise_mesh: sigma_r.*0.0"):
        fuse_scene.denoise_params(fuse_scene.parse_args(base + ["--denoise_iters", "4", "--denoise_sigma_r", "0"]))
    chamfer = ["--conf", "x.conf", "--eval_dir", "e", "--scan", "24"]
    assert dtu_chamfer.denoise_params(dtu_chamfer.parse_args(chamfer)) is None
    got = dtu_chamfer.denoise_params(dtu_chamfer.parse_args(chamfer + [
        "--denoise_iters", "4", "--denoise_vertex_iters", "7", "--denoise_sigma_r", "0.5", "--denoise_sigma_s", "0.01",
        "--denoise_max_move", "0.02", "--denoise_free_boundary", "--denoise_backend", "device"]))
    assert got == {"normal_iterations": 4, "vertex_iterations": 7, "sigma_r": 0.5, "sigma_s": 0.01, "pin_boundary": False, "max_move": 0.02}
    with pytest.raises(SystemExit, match="dtu_chamfer: denoise_mesh: normal_iterations.*-1"):
        dtu_chamfer.denoise_params(dtu_chamfer.parse_args(chamfer + ["--denoise_iters", "-1"]))
    # a Namespace built by hand may lack every flag but the one that asks for the step
    for module in (fuse_scene, dtu_chamfer):
        assert module.denoise_params(argparse.Namespace()) is None
        assert module.denoise_params(argparse.Namespace(denoise_iters=2)) == {**check_params({}), "normal_iterations": 2}


def test_fuse_scene_mesh_steps_denoise_then_smooth_then_simplify():
    """The order of scripts/fuse_scene.py's mesh steps and the `denoise` block of its record, on host arrays: the result is
    simplify(smooth(denoise(mesh))), and each step alone leaves the others' records absent."""
    import argparse
    from surf_amd.mesh_simplify import simplify_mesh
    fuse_scene = _script("fuse_scene")
    v, f = SCENES["noisy_cube8"]
    colors = np.random.default_rng(0).integers(0, 256, v.shape).astype(np.uint8)
    denoise, smooth = check_params({"normal_iterations": 3, "vertex_iterations": 4}), {"iterations": 2}
    from surf_amd.mesh_smooth import check_params as check_smooth
    args = argparse.Namespace(simplify_mm=0.2, simplify_backend="host")
    got = fuse_scene.mesh_steps(v, f, colors, args, denoise, check_smooth(smooth), "cpu")
    step1, _, info = denoise_mesh(v, f, **denoise)
    step2 = smooth_mesh(step1, f, iterations=2)[0]
    want = simplify_mesh(step2, f, 0.2, colors=colors)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    swapped = simplify_mesh(denoise_mesh(smooth_mesh(v, f, iterations=2)[0], f, **denoise)[0], f, 0.2, colors=colors)
    assert swapped[0].shape != want[0].shape or not np.array_equal(bits(swapped[0]), bits(want[0]))      # the order matters here
    block = got[3]
    assert set(block) == set(denoise) | set(info) | {"ms"} and {k: block[k] for k in info} == info
    assert (block["normal_iterations"], block["vertex_iterations"], block["pin_boundary"]) == (3, 4, True)
    assert got[4]["iterations"] == 2 and got[5]["faces_out"] == len(want[1])
    only = fuse_scene.mesh_steps(v, f, colors, argparse.Namespace(simplify_mm=None), denoise, None, "cpu")
    assert np.array_equal(bits(only[0]), bits(step1)) and only[1] is f and only[2] is colors and only[4] is None and only[5] is None
    none = fuse_scene.mesh_steps(v, f, colors, argparse.Namespace(simplify_mm=None), None, None, "cpu")
    assert none[0] is v and none[3:] == (None, None, None)
