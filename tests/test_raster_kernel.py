"""raster_kernel (csrc/raster.hip, behind surf_raster_first_hit) per sample against float64, fed directly.

Part A (no GPU): a float64 reference of the rasterisation (`reference`), its anchor to a float64 Moeller-Trumbore ray caster, a
numpy restatement of the kernel's fp32 arithmetic with one rounding per operator (`restate32`, the library is built without
FMA contraction) and a switch per planted mistake, the conditions the scenes have to meet, and the sensitivity of the comparator.
Parts B-C (gpu): the kernel through the C entry point into buffers the test owns, and the two cleaner backends on top of it.

The rule.  The reference takes exactly what the kernel receives (tests/raster_scenes.py) and does everything in float64: the
projection, the sample lattice x (w-1)/(Wup-1), y (h-1)/(Hup-1) (in sample units: the screen coordinates are scaled by the
inverse and the samples are the integers), three edge functions e_k = (s_{k+1} - p) x (s_{k+2} - p) per (sample, face), the
perspective-correct depth 1 / sum(b_k / cz_k), b_k = e_k / sum(e).  Coverage is inclusive, the nearest depth wins, an exact tie
goes to the smaller face id.  Near rule (a stated deviation from ray casting, pinned here): a face with any vertex at
cz <= 1e-6 is not drawn at all, no clipping.  A face with a non-finite vertex is not drawn.

How a sample is compared.  Nothing is chosen: E_edge of a (face, edge) is the largest |e32 - e64| of that edge function, e32 from
restate32's arithmetic (one value per undirected edge, the larger of the faces that share it, so that both sides call the same
samples clear), and E_z the largest relative |z32 - z64| over the covering pairs of the case.  An edge is CLEAR at a
sample when |e64| > 8 E_edge; a face SURELY COVERS when its three edges are clear and inside, SURELY MISSES when one is clear and
outside, MAY COVER otherwise (always, at most, when the sign of its area is not clear by the same measure).  Two depths are
APART when they differ by more than 8 E_z relative.  The candidates of a sample are the faces that surely or may cover it and
do not lie apart-behind the sample's sure depth; -1 is a candidate only when the sample has no sure depth.  A sample is
DECIDED when it has one candidate; the kernel has to return that one there and some candidate everywhere else.  The 8 stands for
operation order and the device's division, as in the sibling tests.

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest):
    generic scenes      E_EDGE_GENERIC = 8.58e-05 (relative to the face's largest |e64|)    E_Z_GENERIC = 2.87e-06    UNDECIDED_GENERIC = 3.17e-03 (cap 1e-2)
    adversarial scenes  E_EDGE_ADVERSARIAL = 1.57e-05    E_Z_ADVERSARIAL = 3.86e-06    MAX_CANDIDATES = 8 (cap 8)
    parent arithmetic (third barycentric by subtraction) on lattice-t0..5: SEEN_THROUGH = 13 of 3024 samples return a back-layer face
    (per front depth 1, 3, 1, 1, 3, 4; none with the third edge function), and 9 of 1512 on the second image shape

Statements of the issue that could not hold as worded, and what stands in their place:
  * "-1 / the nearest surely-covering face bound the candidates": on `lattice` every sample sits on (or within 1e-6 of) a vertex
    of the front layer, so no single front face surely covers any sample and by that wording every back-layer face under it
    would be a candidate.  Watertightness is stated instead: a may-cover face is CLOSED at a sample when each of its unclear
    edges is shared (same two vertex ids) with a covering face on the other side of that edge that is sure or closed itself
    (a fixed point over the fan).  A closed fan surely covers the sample jointly; its sure depth is the largest float64 depth
    in the fan (connected through the shared edges), and the sample's sure depth is the smallest of these and of the surely
    covering faces.  With that, lattice's candidates are front-layer faces only, which the issue requires.
  * "E_edge over the case's samples": taken over the samples of the face's float64 bounding box grown by 2 samples plus 8 x the
    fp32 error of its screen coordinates, the only samples at which the face is examined at all (beyond it the face surely
    misses: a kernel that draws there returns a non-candidate).  The error grows with the distance from the face, so this E is
    the smaller, stricter one; and the cost stays at seconds.
  * "the largest |e - e64| / (8 E_edge) the kernel reached": the kernel returns no edge function.  What it returns besides the
    id is the depth; |z - z64| / z64 / (8 E_z) of every returned (sample, face) is asserted <= 1 and reported.
  * "the smaller id must win, exactly": both copies of a duplicate have the same float64 depth, so the candidate rule cannot
    tell them apart; the later copy is listed as `banned` by the scene and is never a candidate (so are non-finite faces).
  * lattice "10 of 3,024 samples see through": the order in which one default_rng(0) is consumed is not fully fixed by the
    text (here: per front depth, front jitter, front rotations, back jitter, back rotations); the count on this construction
    is the SEEN_THROUGH line above.

Seen on an MI355X (the [raster] lines of part B):
  * undecided samples, all resolved by the candidate rule: blob 48x64x2 0, 3, 1, 2 of 12,288 per camera; blob-5x7x3-c0 1 of 315
    (0.32 %, the largest generic share); every other generic case 0; lattice 504 of 504 and 252 of 252 in each of the twelve
    cases (every sample a closed fan, every returned id in the front layer); edges 60 of 720 (8.3 %); near 27 of 720; nonfinite
    14 of 720.
  * largest |z - z64| / z64 / (8 E_z): 0.125 (blob, edges, nonfinite), i.e. the restatement's own error; lattice 0.00 .. 0.12.
  * the parent commit's kernel, run on the same scenes: 22 rule violations over the twelve lattice cases (13 of 3,024 and 9 of
    1,512 samples return a back-layer face, none returns -1), bit-equal to restate32(plant="sub"); after the fix 0.
  * the non-finite case failed before the fix: the face with a vertex at z = +inf was returned at 18 samples that the mesh
    without it leaves empty (the six other bad faces and the unreferenced vertices changed nothing); after the fix 0.
  * tests/test_evaluation.py, test_clean_mesh_gpu.py, test_ray_cast_gpu.py and test_end_to_end_dtu.py pass unchanged: no golden
    moved.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from tests import raster_scenes as S

gpu = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FACTOR = 8.0
NEAR = 1e-6
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
PLANTS = ("sub", "linear_depth", "scale", "half_sample", "strict", "cull", "farthest", "tie_larger", "bbox_short", "partial_behind")


# ------------------------------------------------------------------------------------------------------------------
# A.1  projection, edge functions and depth, written once with a dtype: float64 is the reference, float32 the kernel
# ------------------------------------------------------------------------------------------------------------------


def project(c, dt, plant=None):
    """Per face: screen coordinates in sample units sx, sy (3, nf), camera depth cz (3, nf), area, drawn."""
    with np.errstate(all="ignore"):
        v, K, Mx = c["v"].astype(dt), c["K"].astype(dt), c["w2c"].astype(dt)
        X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
        cx = Mx[0, 0] * X + Mx[0, 1] * Y + Mx[0, 2] * Z + Mx[0, 3]
        cy = Mx[1, 0] * X + Mx[1, 1] * Y + Mx[1, 2] * Z + Mx[1, 3]
        cz = Mx[2, 0] * X + Mx[2, 1] * Y + Mx[2, 2] * Z + Mx[2, 3]
        u = (K[0, 0] * cx + K[0, 1] * cy + K[0, 2] * cz) / cz
        w_ = (K[1, 0] * cx + K[1, 1] * cy + K[1, 2] * cz) / cz
        if plant == "scale":
            kx, ky = dt(c["Wup"]) / dt(c["w"]), dt(c["Hup"]) / dt(c["h"])
        else:
            kx, ky = dt(c["Wup"] - 1) / dt(c["w"] - 1), dt(c["Hup"] - 1) / dt(c["h"] - 1)
        f = c["f"].astype(np.int64).T
        sx, sy, czf = (u * kx)[f], (w_ * ky)[f], cz[f]
        front = czf > dt(NEAR)
        drawn = front.any(0) if plant == "partial_behind" else front.all(0)
        drawn &= np.isfinite(sx).all(0) & np.isfinite(sy).all(0)
        area = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sx[2] - sx[0]) * (sy[1] - sy[0])
        iz = dt(1) / czf
    return dict(sx=sx, sy=sy, cz=czf, iz=iz, area=area, drawn=drawn, dt=dt)


def edge_functions(P, fi, x, y, plant=None):
    dt = P["dt"]
    off = dt(0.5) if plant == "half_sample" else dt(0)
    px, py = x.astype(dt) + off, y.astype(dt) + off
    with np.errstate(all="ignore"):
        dx = [P["sx"][k][fi] - px for k in range(3)]
        dy = [P["sy"][k][fi] - py for k in range(3)]
        return np.stack([dx[1] * dy[2] - dx[2] * dy[1], dx[2] * dy[0] - dx[0] * dy[2], dx[0] * dy[1] - dx[1] * dy[0]])


def depth(P, fi, e):
    with np.errstate(all="ignore"):
        iz = P["iz"][:, fi]
        return (e[0] + e[1] + e[2]) / (e[0] * iz[0] + e[1] * iz[1] + e[2] * iz[2])


def box_pairs(x0, x1, y0, y1):
    """(face, x, y) of every sample of every face's inclusive integer box."""
    wb, hb = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = wb * hb
    fi = np.repeat(np.arange(len(cnt)), cnt)
    loc = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return fi, x0[fi] + loc % np.maximum(wb[fi], 1), y0[fi] + loc // np.maximum(wb[fi], 1)


def _clamped_int(a, lo, hi):
    return np.clip(np.nan_to_num(a, nan=lo, posinf=hi, neginf=lo), lo, hi).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# A.3  the kernel's arithmetic in numpy, one fp32 rounding per operator, with the planted mistakes
# ------------------------------------------------------------------------------------------------------------------


def restate32(c, plant=None):
    """(ids (Hup, Wup) int64 with -1 = no hit, zbuf (Hup, Wup) uint64) as raster_kernel computes them."""
    assert plant is None or plant in PLANTS
    Hup, Wup = c["Hup"], c["Wup"]
    P = project(c, F32, plant)
    with np.errstate(all="ignore"):
        ok = P["drawn"] & ((P["area"] > 0) | ((P["area"] < 0) & (plant != "cull")))
        short = 1 if plant == "bbox_short" else 0
        x0 = _clamped_int(np.ceil(P["sx"].min(0)), 0, Wup)
        x1 = _clamped_int(np.floor(P["sx"].max(0)), -1, Wup - 1) - short
        y0 = _clamped_int(np.ceil(P["sy"].min(0)), 0, Hup)
        y1 = _clamped_int(np.floor(P["sy"].max(0)), -1, Hup - 1) - short
        x1[~ok] = -1
        fi, x, y = box_pairs(x0, x1, y0, y1)
        e = edge_functions(P, fi, x, y, plant)
        pos = P["area"][fi] > 0
        if plant == "sub":                                             # the parent commit's coverage and depth
            inv = F32(1) / P["area"][fi]
            b0, b1 = e[0] * inv, e[1] * inv
            b2 = F32(1) - b0 - b1
            inside = ~((b0 < 0) | (b1 < 0) | (b2 < 0))
            iz = P["iz"][:, fi]
            z = F32(1) / (b0 * iz[0] + b1 * iz[1] + b2 * iz[2])
        else:
            if plant == "strict":
                inside = np.where(pos, (e > 0).all(0), (e < 0).all(0))
            else:
                inside = np.where(pos, (e >= 0).all(0), (e <= 0).all(0))
            if plant == "linear_depth":
                cz = P["cz"][:, fi]
                z = (e[0] * cz[0] + e[1] * cz[1] + e[2] * cz[2]) / (e[0] + e[1] + e[2])
            else:
                z = depth(P, fi, e)
        keep = inside & (z > 0)
    fi, x, y, z = fi[keep], x[keep], y[keep], z[keep].astype(F32)
    zb = z.view(np.uint32).astype(np.uint64)
    low = fi.astype(np.uint64)
    if plant == "tie_larger":
        low = np.uint64(0xFFFFFFFF) - low
    key = (zb << np.uint64(32)) | low
    if plant == "farthest":
        key = ((np.uint64(0xFFFFFFFF) - zb) << np.uint64(32)) | low
    zbuf = np.full(Hup * Wup, EMPTY, np.uint64)
    np.minimum.at(zbuf, y * Wup + x, key)
    ids = decode(zbuf)
    if plant == "tie_larger":
        ids = np.where(ids >= 0, 0xFFFFFFFF - ids, -1)
    return ids.reshape(Hup, Wup), zbuf.reshape(Hup, Wup)


def decode(zbuf):
    """-1 / the low 32 bits, as ops.raster_first_hit decodes the z-buffer."""
    zbuf = np.asarray(zbuf).view(np.uint64)
    return np.where(zbuf == EMPTY, np.int64(-1), (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64))


# ------------------------------------------------------------------------------------------------------------------
# A.1 / A.4  the float64 reference and the candidate sets
# ------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(None)
def reference(name):
    c = S.case(name)
    Hup, Wup, nf = c["Hup"], c["Wup"], len(c["f"])
    nv = len(c["v"])
    P, Q = project(c, F64), project(c, F32)
    drawn = P["drawn"]
    with np.errstate(all="ignore"):
        err = np.maximum(np.abs(Q["sx"].astype(F64) - P["sx"]), np.abs(Q["sy"].astype(F64) - P["sy"])).max(0)
        pad = np.where(drawn, 2 + np.ceil(FACTOR * np.nan_to_num(err, nan=0.0, posinf=0.0)), 0)
        x0 = _clamped_int(np.floor(P["sx"].min(0)) - pad, 0, Wup)
        x1 = _clamped_int(np.ceil(P["sx"].max(0)) + pad, -1, Wup - 1)
        y0 = _clamped_int(np.floor(P["sy"].min(0)) - pad, 0, Hup)
        y1 = _clamped_int(np.ceil(P["sy"].max(0)) + pad, -1, Hup - 1)
        x1[~drawn] = -1
        fi, x, y = box_pairs(x0, x1, y0, y1)
        smp = y * Wup + x
        e64 = edge_functions(P, fi, x, y)
        e32 = edge_functions(Q, fi, x, y).astype(F64)
        E = np.zeros((3, nf))
        scale = np.zeros(nf)
        for k in range(3):
            np.maximum.at(E[k], fi, np.abs(e32[k] - e64[k]))
            np.maximum.at(scale, fi, np.abs(e64[k]))
        fv = c["f"].astype(np.int64)                                  # one E per undirected edge: the faces on its two sides
        ek = np.stack([np.minimum(fv[:, (k + 1) % 3], fv[:, (k + 2) % 3]) * nv + np.maximum(fv[:, (k + 1) % 3], fv[:, (k + 2) % 3])
                       for k in range(3)])                            # have to call the same samples clear
        _, einv = np.unique(ek.reshape(-1), return_inverse=True)
        emax = np.zeros(einv.max() + 1)
        np.maximum.at(emax, einv, E.reshape(-1))
        E = emax[einv].reshape(3, nf)
        Ea = np.abs(Q["area"].astype(F64) - P["area"])
        area_clear = drawn & (np.abs(P["area"]) > FACTOR * Ea)
        sgn = np.sign(P["area"])
        thr = FACTOR * E[:, fi]
        se = sgn[fi] * e64
        ac = area_clear[fi]
        sure = ac & (se > thr).all(0)
        may = np.where(ac, ~(se < -thr).any(0), ~(e64 < -thr).any(0) | ~(e64 > thr).any(0)) & ~sure
        unclear = ~(se > thr) & ~(se < -thr)                          # (3, n) per edge; meaningful where ac
        inside64 = np.where(sgn[fi] > 0, (e64 >= 0).all(0), (e64 <= 0).all(0)) & (sgn[fi] != 0)
        keep = sure | may
        fi, x, y, smp, e64, e32 = fi[keep], x[keep], y[keep], smp[keep], e64[:, keep], e32[:, keep]
        sure, may, unclear, ac, inside64 = sure[keep], may[keep], unclear[:, keep], ac[keep], inside64[keep]
        z64 = depth(P, fi, e64)
        z32 = depth(Q, fi, e32.astype(F32)).astype(F64)
        rel = np.abs(z32 - z64) / np.abs(z64)
        Ez = float(rel[inside64].max()) if inside64.any() else 0.0
    n = len(fi)
    # closed fans: records (pair, edge) keyed by (sample, the edge's two vertex ids); side = on which side of the min -> max
    # direction the face lies
    f = c["f"].astype(np.int64)
    rp = np.tile(np.arange(n), 3)
    a = np.concatenate([f[fi, (k + 1) % 3] for k in range(3)])
    b = np.concatenate([f[fi, (k + 2) % 3] for k in range(3)])
    side = np.concatenate([sgn[fi]] * 3) * np.where(a < b, 1.0, -1.0) * np.concatenate([ac] * 3)
    side[a == b] = 0
    key = (smp[rp] * nv + np.minimum(a, b)) * nv + np.maximum(a, b)
    _, inv = np.unique(key, return_inverse=True)
    G = int(inv.max()) + 1 if n else 0
    need = np.concatenate([unclear[k] for k in range(3)]) & may[rp]
    alive = sure | (may & ac)
    for _ in range(64):
        ra = alive[rp]
        has_pos, has_neg = np.zeros(G, bool), np.zeros(G, bool)
        has_pos[inv[ra & (side > 0)]] = True
        has_neg[inv[ra & (side < 0)]] = True
        matched = np.where(side > 0, has_neg[inv], has_pos[inv]) & (side != 0)
        bad = np.zeros(n, bool)
        bad[rp[need & ~matched]] = True
        new = alive & ~bad
        if (new == alive).all():
            break
        alive = new
    closed = alive & may
    lab = np.where(alive, z64, -np.inf)
    ra = alive[rp]
    link = np.zeros(G, bool)
    link[inv[need & ra]] = True
    sel = ra & link[inv]
    for _ in range(16):                                                # the largest depth of a fan, through its shared edges
        gmax = np.full(G, -np.inf)
        np.maximum.at(gmax, inv[sel], lab[rp[sel]])
        new = lab.copy()
        np.maximum.at(new, rp[sel], gmax[inv[sel]])
        if (new == lab).all():
            break
        lab = new
    D = np.full(Hup * Wup, np.inf)
    np.minimum.at(D, smp[sure], z64[sure])
    np.minimum.at(D, smp[closed], lab[closed])
    banned = np.zeros(nf, bool)
    banned[np.asarray(c.get("banned", []), np.int64)] = True
    cand = (z64 <= D[smp] * (1 + FACTOR * Ez)) & ~banned[fi]
    ncand = np.bincount(smp[cand], minlength=Hup * Wup) + np.isinf(D)
    ckey = smp[cand] * nf + fi[cand]
    order = np.argsort(ckey)
    return dict(case=c, P=P, E=E, scale=scale, Ez=Ez, D=D, ncand=ncand, decided=ncand == 1, ckey=ckey[order], cz=z64[cand][order],
                cand_smp=smp[cand], cand_face=fi[cand], sure_smp=smp[sure], sure_face=fi[sure], drawn=drawn,
                box=(x0, x1, y0, y1), n_closed=int(np.unique(smp[closed]).size))


def check(name, ids):
    """The samples at which ids is no candidate: [] when the rule holds."""
    r = reference(name)
    c = r["case"]
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    assert ids.shape == (c["Hup"] * c["Wup"],)
    nf = len(c["f"])
    wrong = np.where(ids < 0, ~np.isinf(r["D"]), ~np.isin(np.arange(len(ids)) * nf + ids, r["ckey"]) | (ids >= nf))
    return [(int(s) // c["Wup"], int(s) % c["Wup"], int(ids[s])) for s in np.nonzero(wrong)[0]]


def depth_ratio(name, zbuf):
    """Largest |z - z64| / z64 / (8 E_z) over the returned (sample, face) pairs that are candidates."""
    r = reference(name)
    zbuf = np.asarray(zbuf).reshape(-1).view(np.uint64)
    ids = decode(zbuf)
    hit = np.nonzero(ids >= 0)[0]
    k = hit * len(r["case"]["f"]) + ids[hit]
    pos = np.searchsorted(r["ckey"], k)
    pos[pos >= len(r["ckey"])] = 0
    okk = r["ckey"][pos] == k if len(r["ckey"]) else np.zeros(len(k), bool)
    z = (zbuf[hit] >> np.uint64(32)).astype(np.uint32).view(F32).astype(F64)[okk]
    z64 = r["cz"][pos[okk]]
    if not len(z) or r["Ez"] == 0:
        return 0.0
    return float((np.abs(z - z64) / z64).max() / (FACTOR * r["Ez"]))


def first_decided(name):
    """The float64 answer on decided samples, -2 elsewhere."""
    r = reference(name)
    out = np.full(len(r["D"]), -2, np.int64)
    out[r["decided"] & np.isinf(r["D"])] = -1
    one = r["decided"][r["cand_smp"]]
    out[r["cand_smp"][one]] = r["cand_face"][one]
    return out


# ------------------------------------------------------------------------------------------------------------------
# A.2  anchor: an independent float64 Moeller-Trumbore caster (test_evaluation.py's)
# ------------------------------------------------------------------------------------------------------------------


def ray_cast(c):
    from tests.test_evaluation import _first_hit_bruteforce
    cz = reference_cz(c)
    f = c["f"][(cz > NEAR).all(1)]                                     # the near rule is the rasteriser's, not the caster's
    back = np.nonzero((cz > NEAR).all(1))[0]
    ids = _first_hit_bruteforce(c["v"].astype(F64), f.astype(np.int64), c["intr"], c["c2w"], c["h"], c["w"], c["up"]).numpy().reshape(-1)
    return np.where(ids >= 0, back[np.maximum(ids, 0)], -1)


def reference_cz(c):
    v, Mx = c["v"].astype(F64), c["w2c"].astype(F64)
    return (v @ Mx[2, :3] + Mx[2, 3])[c["f"].astype(np.int64)]


ANCHORED = ["blob-48x64x2-c3"] + [f"blob-5x7x3-c{k}" for k in range(4)] + ["blob-2x7x3-c0", "blob-5x7x5-c2", "closed"]


@pytest.mark.parametrize("name", ANCHORED)
def test_reference_agrees_with_ray_casting_where_decided(name):
    want = first_decided(name)
    got = ray_cast(S.case(name))
    d = want != -2
    assert d.mean() > 0.99 and (want[d] >= 0).any()
    assert np.array_equal(got[d], want[d]), np.nonzero(got[d] != want[d])[0][:10]


# ------------------------------------------------------------------------------------------------------------------
# A.5  conditions on the inputs, from the reference alone
# ------------------------------------------------------------------------------------------------------------------


def undecided_share(name):
    return float(1.0 - reference(name)["decided"].mean())


@pytest.mark.parametrize("name", S.GENERIC)
def test_generic_scenes_are_decided(name):
    r = reference(name)
    assert undecided_share(name) <= 0.01
    hits = first_decided(name)
    if "-n" not in name and not name.startswith("blob-2x7"):
        assert (hits >= 0).any() and (hits == -1).any()                # the prefixes may hit nothing at all: stated
    assert np.isfinite(r["E"]).all() and np.isfinite(r["Ez"])


def test_generic_scenes_use_the_last_vertex_and_both_area_signs():
    c = S.case("blob-48x64x2-c0")
    assert (c["f"] == len(c["v"]) - 1).any()
    a = reference("blob-48x64x2-c0")["P"]["area"]
    assert (a > 0).sum() > 100 and (a < 0).sum() > 100
    assert S.case("blob-48x64x2-c3")["K"][0, 1] != 0
    assert [len(S.case(n)["f"]) for n in S.SIZES[4:]] == [1, 255, 256, 257, 513]


@pytest.mark.parametrize("name", S.ADVERSARIAL)
def test_adversarial_candidate_sets_are_small(name):
    r = reference(name)
    c = r["case"]
    assert r["ncand"].max() <= 8
    if name.startswith("lattice"):
        assert (r["cand_face"] < c["front"]).all()                     # candidates lie entirely in the front layer
        assert not np.isinf(r["D"]).any()                              # and -1 is nowhere a candidate
        assert (~r["decided"]).mean() > 0.9                            # built to be undecided
    else:
        assert np.isinf(r["D"]).sum() == 0                             # the huge triangle lies behind everything
        t = c["tags"]
        keys = set(r["cand_face"].tolist())
        assert set(t["dup_first"]) <= keys and not set(t["dup_second"]) & keys
        assert set(t["before"]) <= keys and not set(t["behind"]) & keys
        assert not set(t["repeated"]) & set(r["sure_face"].tolist())


def test_every_skip_reason_fires():
    r = reference("edges")
    c, P = r["case"], r["P"]
    x0, x1, y0, y1 = r["box"]
    t = c["tags"]
    assert (P["sx"][:, t["off_left"]].max(0) < -2).all() and (P["sx"][:, t["off_right"]].min(0) > c["Wup"] + 1).all()
    assert (P["sy"][:, t["off_top"]].max(0) < -2).all() and (P["sy"][:, t["off_bottom"]].min(0) > c["Hup"] + 1).all()
    assert (P["area"][t["repeated"]] == 0).all() and (project(c, F32)["area"][t["repeated"]] == 0).all()      # zero area
    sub = t["subsample"][0]                                            # empty bounding box: no integer inside
    assert np.ceil(P["sx"][:, sub].min()) > np.floor(P["sx"][:, sub].max())
    n = reference("near")
    cz = reference_cz(n["case"])
    behind = (cz <= NEAR).any(1)
    assert sorted(np.nonzero(behind)[0].tolist()) == sorted(n["case"]["tags"]["behind"])
    assert sorted((cz[behind] <= NEAR).sum(1).tolist()) == [1, 1, 1, 2, 3]
    assert (np.abs(cz - NEAR) > 1e-7).all()                            # no vertex near the threshold itself
    assert not n["drawn"][behind].any() and n["drawn"][~behind].all()
    assert np.abs(n["P"]["sx"][:, n["case"]["tags"]["huge_near"]]).max() > 5e6
    assert (first_decided("near") == n["case"]["tags"]["huge_near"][0]).any() and not np.isin(first_decided("near"), n["case"]["tags"]["hidden"]).any()
    nfin = reference("nonfinite")
    assert not nfin["drawn"][nfin["case"]["tags"]["bad"]].any() and nfin["drawn"].sum() == 3
    assert (first_decided("nonfinite") == -1).any()


def test_closed_silhouette_has_no_far_side_candidate():
    r = reference("closed")
    assert not np.isin(r["cand_face"], r["case"]["far"]).any()
    assert len(r["case"]["far"]) > 50 and (~np.isinf(r["D"])).sum() > 300


# ------------------------------------------------------------------------------------------------------------------
# A.6  sensitivity: the comparator accepts the restatement and rejects every planted mistake
# ------------------------------------------------------------------------------------------------------------------

CPU_CASES = S.GENERIC + S.ADVERSARIAL + ["near", "nonfinite"]


@pytest.mark.parametrize("name", CPU_CASES)
def test_comparator_accepts_the_restatement(name):
    ids, zbuf = restate32(S.case(name))
    assert check(name, ids) == []
    assert depth_ratio(name, zbuf) <= 1.0


WHERE = {"sub": S.LATTICE, "linear_depth": ["edges"], "scale": ["blob-48x64x2-c0", "lattice-t0"], "half_sample": ["blob-48x64x2-c1", "lattice-t0"],
         "strict": ["lattice-t0", "lattice9-t1"], "cull": ["blob-48x64x2-c2", "closed"], "farthest": ["blob-48x64x2-c0", "closed"],
         "tie_larger": ["edges"], "bbox_short": ["lattice-t1", "blob-48x64x2-c3"], "partial_behind": ["near"]}


@pytest.mark.parametrize("plant", PLANTS)
def test_comparator_rejects(plant):
    caught = [n for n in WHERE[plant] if check(n, restate32(S.case(n), plant)[0]) != []]
    if plant == "sub":
        assert caught, "the parent's arithmetic passes every lattice case"
    else:
        assert caught == WHERE[plant], (plant, caught)


def seen_through():
    n = 0
    for t in range(6):
        c = S.case(f"lattice-t{t}")
        ids = restate32(c, "sub")[0]
        assert (ids >= 0).all()
        n += int((ids >= c["front"]).sum())
    return n


# ------------------------------------------------------------------------------------------------------------------
# the measured lines of the docstring
# ------------------------------------------------------------------------------------------------------------------


def _recorded(label):
    return float(re.search(label + r"\s*=\s*([0-9.e+-]+)", __doc__).group(1))


def _rel_edge(name):
    r = reference(name)
    with np.errstate(all="ignore"):
        q = r["E"] / r["scale"][None]
    return float(np.nan_to_num(q, nan=0.0, posinf=0.0).max())


@functools.lru_cache(None)
def measured():
    return {
        "E_EDGE_GENERIC": max(_rel_edge(n) for n in S.GENERIC),
        "E_Z_GENERIC": max(reference(n)["Ez"] for n in S.GENERIC),
        "UNDECIDED_GENERIC": max(undecided_share(n) for n in S.GENERIC),
        "E_EDGE_ADVERSARIAL": max(_rel_edge(n) for n in S.ADVERSARIAL),
        "E_Z_ADVERSARIAL": max(reference(n)["Ez"] for n in S.ADVERSARIAL),
        "MAX_CANDIDATES": max(int(reference(n)["ncand"].max()) for n in S.ADVERSARIAL),
        "SEEN_THROUGH": seen_through(),
    }


def test_measured_margins_are_recorded():
    """The numbers of the module docstring are the ones these inputs give.  The counts are exact (lattice's camera is the
    identity).  The E lines are maxima over a few near-degenerate pairs and depend on the last bit of the host's fp32
    inverse(c2w), which differs between hosts (seen: 2.13e-06 and 3.15e-06 for the same case): they are held within a factor 2;
    the share of undecided samples is a count over the same inputs and is held to its cap."""
    m = measured()
    for label, v in m.items():
        rec = _recorded(label)
        if label in ("MAX_CANDIDATES", "SEEN_THROUGH"):
            assert v == rec, (label, v, rec)
        elif label != "UNDECIDED_GENERIC":
            assert rec / 2 <= v <= rec * 2, (label, v, rec)
    assert m["UNDECIDED_GENERIC"] <= 0.01 and m["MAX_CANDIDATES"] <= 8 and m["SEEN_THROUGH"] > 0


# ------------------------------------------------------------------------------------------------------------------
# B. the kernel through the C entry point
# ------------------------------------------------------------------------------------------------------------------

GUARD = 3                                                              # patterned rows before and behind zbuf


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _pattern(n):
    return (torch.arange(n, dtype=torch.int64) * 0x9E3779B97F4A7C15 % (1 << 62)) | (1 << 40)


def _raster(c, faces=None, over=()):
    """surf_raster_first_hit into the middle of a patterned int64 buffer; (zbuf as uint64 numpy (Hup, Wup), status)."""
    from surf_amd import _lib
    d = dev()
    over = dict(over)
    a = dict(h=c["h"], w=c["w"], Hup=c["Hup"], Wup=c["Wup"])
    a.update({k: v for k, v in over.items() if k in a})
    Hup, Wup = c["Hup"], c["Wup"]
    v = torch.from_numpy(c["v"]).to(d)
    f = torch.from_numpy(c["f"] if faces is None else np.ascontiguousarray(faces, np.int32)).to(d)
    buf = _pattern((Hup + 2 * GUARD) * Wup)
    buf[GUARD * Wup:(GUARD + Hup) * Wup] = -1
    before = buf.clone()
    buf = buf.to(d)
    K, w2c = np.ascontiguousarray(c["K"]), np.ascontiguousarray(c["w2c"])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    args = dict(vertices=ptr(v), faces=ptr(f), n_faces=f.shape[0], h_K=K.ctypes.data_as(ctypes.c_void_p),
                h_w2c=w2c.ctypes.data_as(ctypes.c_void_p), zbuf=ctypes.c_void_p(buf.data_ptr() + 8 * GUARD * Wup))
    args.update({k: v for k, v in over.items() if k in args})
    fn = _lib.lib().surf_raster_first_hit
    status = 0
    try:
        fn(args["vertices"], args["faces"], args["n_faces"], args["h_K"], args["h_w2c"], a["h"], a["w"], a["Hup"], a["Wup"], args["zbuf"],
           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    except _lib.SurfHipError as e:
        status = str(e)
    torch.cuda.synchronize()
    got = buf.cpu()
    lo, hi = GUARD * Wup, (GUARD + Hup) * Wup
    assert torch.equal(got[:lo], before[:lo]) and torch.equal(got[hi:], before[hi:]), "the guard rows changed"
    return got[lo:hi].numpy().view(np.uint64).reshape(Hup, Wup), status, torch.equal(got, before)


def _report(name, zbuf):
    r = reference(name)
    und = ~r["decided"]
    print(f"[raster] {name} undecided={und.mean():.4f} resolved_by_candidates={int(und.sum())} closed_fans={r['n_closed']} "
          f"depth_ratio={depth_ratio(name, zbuf):.3f} E_z={r['Ez']:.2e}")


@gpu
@pytest.mark.parametrize("name", S.GENERIC + S.ADVERSARIAL + ["near"])
def test_raster_kernel_matches_float64(name):
    c = S.case(name)
    zbuf, status, _ = _raster(c)
    assert status == 0
    ids = decode(zbuf)
    _report(name, zbuf)
    assert np.array_equal(zbuf == EMPTY, ids == -1) and ids.max() < len(c["f"])
    bad = check(name, ids)
    assert bad == [], (len(bad), bad[:10])
    assert depth_ratio(name, zbuf) <= 1.0
    again, _, _ = _raster(c)
    assert np.array_equal(again, zbuf)                                 # two launches, bit-equal
    if name.startswith("lattice"):
        assert (ids >= 0).all() and (ids < c["front"]).all()
    if name == "closed":
        r = reference(name)
        inside = ~np.isinf(r["D"])
        assert (ids.reshape(-1)[inside] >= 0).all() and not np.isin(ids.reshape(-1)[inside], c["far"]).any()
    if name == "edges":
        assert not np.isin(ids, c["tags"]["dup_second"]).any() and np.isin(ids, c["tags"]["dup_first"]).any()


@gpu
def test_raster_kernel_matches_the_ops_decode():
    from surf_amd import ops
    c = S.case("blob-5x7x3-c3")
    d = dev()
    ids = ops.raster_first_hit(torch.from_numpy(c["v"]).to(d), torch.from_numpy(c["f"]).to(d), c["intr"], c["c2w"], (c["h"], c["w"]), c["up"])
    assert ids.dtype == torch.int64 and np.array_equal(ids.cpu().numpy(), decode(_raster(c)[0]))


@gpu
def test_raster_kernel_ignores_non_finite_vertices():
    c, base = S.case("nonfinite"), S.case("nonfinite-base")
    zbuf, status, _ = _raster(c)
    want, _, _ = _raster(base)
    ids = decode(zbuf)
    _report("nonfinite", zbuf)
    assert status == 0 and not np.isin(ids, c["tags"]["bad"]).any()
    assert np.array_equal(zbuf, want)                                  # every sample as without the bad faces
    assert check("nonfinite", ids) == [] and check("nonfinite-base", decode(want)) == []


@gpu
@pytest.mark.parametrize("name", ["blob-48x64x2-c3", "lattice-t3", "edges"])
def test_raster_kernel_under_a_face_permutation(name):
    c = S.case(name)
    r = reference(name)
    perm = np.random.default_rng(5).permutation(len(c["f"]))           # new face k is old face perm[k]
    ids = decode(_raster(c)[0]).reshape(-1)
    pids = decode(_raster(c, faces=c["f"][perm])[0]).reshape(-1)
    back = np.where(pids >= 0, perm[np.maximum(pids, 0)], -1)
    for later, first in c.get("alias", {}).items():                    # the copies of an exact duplicate are one face here
        back[back == later] = first
    assert check(name, back) == []
    # the depths are those of the same arithmetic: where the ids differ, the two faces tie exactly in the kernel's own depth
    z, pz = _raster(c)[0].reshape(-1) >> np.uint64(32), _raster(c, faces=c["f"][perm])[0].reshape(-1) >> np.uint64(32)
    assert np.array_equal(z, pz)
    d = r["decided"]
    assert np.array_equal(back[d], ids[d])


@gpu
def test_raster_kernel_refuses_what_it_cannot_hold():
    c = S.case("blob-5x7x3-c0")
    null = ctypes.c_void_p(0)
    for over in ({"vertices": null}, {"faces": null}, {"h_K": null}, {"h_w2c": null}, {"zbuf": null}, {"n_faces": 0}, {"n_faces": -3},
                 {"h": 1}, {"w": 1}, {"Hup": 1}, {"Wup": 1}, {"h": 0}, {"Wup": -2}):
        _, status, untouched = _raster(c, over=over)
        assert "invalid argument" in str(status), (over, status)       # SURF_E_ARG
        assert untouched, over


# ------------------------------------------------------------------------------------------------------------------
# C. what the cleaner makes of it: must <= got <= may
# ------------------------------------------------------------------------------------------------------------------


def _holed_mask(nv, h, w):
    g = np.random.default_rng(11)
    m = g.random((nv, h, w)) < 0.8
    m[:, h // 3:h // 2, w // 4:w // 2] = False
    return m


CLEAN_IDS = [f"{k}-{v[0].split('-', 1)[1]}" for k, vs in S.CLEANER.items() for v in vs]


@gpu
@pytest.mark.parametrize("names", [v for vs in S.CLEANER.values() for v in vs], ids=CLEAN_IDS)
def test_cleaner_keeps_between_must_and_may(names):
    from surf_amd import ops
    from surf_amd.evaluation import clean_mesh
    c0 = S.case(names[0])
    h, w, up, nf = c0["h"], c0["w"], c0["up"], len(c0["f"])
    mask = _holed_mask(len(names), h, w)
    must, may = np.zeros(nf, bool), np.zeros(nf, bool)
    for i, n in enumerate(names):
        r = reference(n)
        yy, xx = np.divmod(np.arange(c0["Hup"] * c0["Wup"]), c0["Wup"])
        masked = mask[i][yy // up, xx // up]                          # sample (i, j) -> mask texel (i // up, j // up)
        fd = first_decided(n)
        must[fd[masked & (fd >= 0)]] = True
        may[r["cand_face"][masked[r["cand_smp"]]]] = True
    intrs = torch.stack([S.case(n)["intr"] for n in names])
    c2ws = torch.stack([S.case(n)["c2w"] for n in names])
    d = dev()
    tm = torch.from_numpy(mask)
    host = clean_mesh.visible_faces(c0["v"], c0["f"], tm, intrs, c2ws, upscale=up, device=d)
    device = ops.clean_visible_faces(torch.from_numpy(c0["v"]).to(d), torch.from_numpy(c0["f"]).to(d), tm.to(torch.uint8).to(d), intrs, c2ws, up).cpu().numpy()
    assert may.sum() > 10 and (must.sum() > 10 or "front" in c0)       # lattice has no decided sample: `may` binds there
    for got in (host, device):
        assert not (must & ~got).any(), np.nonzero(must & ~got)[0][:10]
        assert not (got & ~may).any(), np.nonzero(got & ~may)[0][:10]
    assert np.array_equal(host, device)
    if "front" in c0:
        assert not host[c0["front"]:].any()                            # no back-layer face is kept
