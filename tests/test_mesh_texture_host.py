"""Texture baking on the host (surf_amd/mesh_texture.py, the rule of include/surf_hip.h above surf_texture_*): the entry points and
their status codes; the atlas layout; the numpy-fp32 mirror per texel against a float64 restatement of rules 2-5 written here; the
baked colours against the paint of the scenes; the fill rule; the OBJ writer and reader; the scripts' flags.  Everything runs
without a GPU: the depth maps are given (tests/mesh_texture_scenes.py renders them)."""
import ctypes
import functools
import importlib
import os
import re
import sys

import numpy as np
import pytest

from surf_amd import _lib, mesh_io
from surf_amd import mesh_texture as MT
from tests import mesh_texture_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = (4, 5, 8, 16)
MS = (1, 2, 3, 7)
# fp32 rounding bands of the restatement's decisions.  A texel's projection is a quotient of sums of four products of magnitude up
# to 150 (focal length and principal point times coordinates up to 3): 4 * 150 * 2^-24 / z with z >= 2 gives 2e-5 pixels; depths
# and cosines are sums of a few terms of magnitude <= 4 and <= 1: 2e-5 covers ten roundings of each with room to spare.
BAND_PX, BAND_Z, BAND_COS = 5e-5, 2e-5, 2e-5
EXCLUDED_CAP = 0.01


def _script(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


# ---- 1, 2: the C ABI ----

def test_entry_points_declared_bound_exported():
    with open(_lib.HEADER_PATH) as f:
        hdr = f.read()
    assert "#define SURF_ABI_VERSION 41" in hdr and _lib.ABI_VERSION == 41
    L = _lib.lib()
    assert L.surf_abi_version() == 41
    for name, nargs in (("surf_texture_pack_view", 6), ("surf_texture_bake", 21), ("surf_texture_finish", 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(L, name).restype is ctypes.c_int
    assert hdr.index("THE RULE.  vertices (n,3) fp32, faces (m,3) int32, T = texels_per_edge") < hdr.index("int surf_texture_pack_view(")
    from surf_amd import ops
    for name in ("raster_depth", "texture_pack_view", "bake_texture"):
        assert callable(getattr(ops, name))
    for name in ("TextureView", "view_from_item", "atlas_layout", "face_uv", "mesh_depth_maps", "check_args", "check_params",
                 "bake_texture", "texture_step"):
        assert hasattr(MT, name)
    assert callable(mesh_io.write_obj) and callable(mesh_io.read_obj)


def test_limits_and_null_pointers_before_any_launch():
    """No GPU is needed to be refused: every check precedes the launch and the first read of a host array."""
    L = _lib.lib()
    one = ctypes.c_void_p(64)                                       # never dereferenced
    f = ctypes.c_float

    def bake(vertices=one, faces=one, sums=one, host=one, n=3, m=1, T=4, cols=1, rows=1, n_views=1, power=4):
        return L.surf_texture_bake(vertices, n, faces, m, T, cols, rows, host, host, host, host, n_views, f(0.0), f(0.1), f(0.2),
                                   power, 0, 1, sums, None, None)

    for bad in (dict(vertices=None), dict(faces=None), dict(sums=None), dict(host=None), dict(m=0), dict(n=-1), dict(T=3),
                dict(T=65), dict(cols=0), dict(rows=0), dict(m=3), dict(n_views=-1), dict(power=0), dict(power=17)):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            bake(**bad)
    for big in (dict(n_views=17), dict(T=64, cols=10000, rows=10000), dict(m=1 << 31, cols=1 << 15, rows=1 << 15)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            bake(**big)
    with pytest.raises(_lib.SurfHipError, match="invalid argument"):
        L.surf_texture_bake(one, 3, one, 1, 4, 1, 1, one, one, one, one, 1, f(float("nan")), f(0.1), f(0.2), 4, 0, 1, one, None, None)
    for bad in (dict(sums=None), dict(faces=None), dict(atlas=None), dict(T=2), dict(m=0)):
        a = dict(sums=one, faces=one, atlas=one, T=4, m=1)
        a.update(bad)
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            L.surf_texture_finish(a["sums"], 3, a["faces"], a["m"], a["T"], 1, 1, None, f(0.5), a["atlas"], None)
    with pytest.raises(_lib.SurfHipError, match="limit"):
        L.surf_texture_finish(one, 3, one, 1, 64, 10000, 10000, None, f(0.5), one, None)
    for args in ((None, one, 4, 4, one), (one, None, 4, 4, one), (one, one, 4, 4, None), (one, one, 1, 4, one), (one, one, 4, 1, one)):
        with pytest.raises(_lib.SurfHipError, match="invalid argument"):
            L.surf_texture_pack_view(args[0], args[1], args[2], args[3], args[4], None)
    with pytest.raises(_lib.SurfHipError, match="limit"):
        L.surf_texture_pack_view(one, one, 1 << 15, 1 << 14, one, None)


def test_arguments_are_refused_by_name():
    for kw, word in ((dict(texels_per_edge=3), "texels_per_edge.*3"), (dict(texels_per_edge=65), "texels_per_edge.*65"),
                     (dict(texels_per_edge=8.0), "texels_per_edge.*8.0"), (dict(power=0), "power.*0"), (dict(power=17), "power.*17"),
                     (dict(depth_tol=None), "depth_tol.*None"), (dict(depth_tol=-1.0), "depth_tol.*-1.0"),
                     (dict(depth_tol=float("nan")), "depth_tol.*nan"), (dict(min_cos=1.5), "min_cos.*1.5"),
                     (dict(z_min=-1), "z_min.*-1"), (dict(fill=2), "fill.*2")):
        with pytest.raises(ValueError, match=word):
            MT.check_args(**{"depth_tol": 0.1, **kw})
    assert MT.check_args(depth_tol=1) == (8, 1.0, 0.2, 4, False, 0.0, 0.5)
    with pytest.raises(ValueError, match="unknown key.*'texels'"):
        MT.check_params({"texels": 8, "depth_tol": 1.0})
    assert MT.check_params({"depth_tol": 2.0, "power": 2})["power"] == 2
    with pytest.raises(ValueError, match="texels_per_edge.*--simplify_mm"):
        MT.atlas_layout(2 * 300 * 300, 64)                          # 300 cells of 65 texels across
    v, f = S.scenes()["single"]["vertices"], S.scenes()["single"]["faces"]
    with pytest.raises(ValueError, match="backend.*'gpu'"):
        MT.bake_texture(v, f, [], depth_tol=0.1, backend="gpu")
    with pytest.raises(ValueError, match="vertex_colors"):
        MT.bake_texture(v, f, [], depth_tol=0.1, vertex_colors=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="1 mesh_depths for 0 views"):
        MT.bake_texture(v, f, [], depth_tol=0.1, mesh_depths=[np.zeros((4, 4), np.float32)])


# ---- 3: the layout ----

def _layout(m, T):
    """Rule 1's sizes from its text: (ncell, cols, rows, Ha, Wa)."""
    ncell = (m + 1) // 2
    cols = 1
    while cols * cols < ncell:                                      # ceil(sqrt(ncell)) without a square root
        cols += 1
    rows = -(-ncell // cols)
    return ncell, cols, rows, rows * T, cols * (T + 1)


def _owner_loop(m, T):
    """Rule 1 texel by texel, in plain Python: (owner (Ha, Wa) face or -1, corner texels (m, 3, 2) as (x, y))."""
    ncell, cols, rows, _, _ = _layout(m, T)
    owner =-np.ones((rows * T, cols * (T + 1)), np.int64)
    claims = np.zeros(owner.shape, np.int64)
    corners = np.zeros((m, 3, 2), np.int64)
    for k in range(rows * cols):
        x0, y0 = (k % cols) * (T + 1), (k // cols) * T
        for j in range(T):
            for i in range(T + 1):
                for face, mine in ((2 * k, i + j <= T - 1), (2 * k + 1, i + j >= T)):
                    if mine and face < m:
                        owner[y0 + j, x0 + i] = face
                        claims[y0 + j, x0 + i] += 1
        for face, cs in ((2 * k, ((0, 0), (T - 2, 0), (0, T - 2))), (2 * k + 1, ((T, T - 1), (2, T - 1), (T, 1)))):
            if face < m:
                corners[face] = [(x0 + i, y0 + j) for i, j in cs]
    return owner, claims, corners, (ncell, cols, rows, rows * T, cols * (T + 1))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("m", MS)
def test_layout(m, T):
    owner, claims, corners, layout = _owner_loop(m, T)
    assert MT.atlas_layout(m, T) == layout
    Ha, Wa = layout[3:]
    assert claims.max() == 1                                        # at most one owner
    assert (np.bincount(owner[owner >= 0], minlength=m) == T * (T + 1) // 2).all()
    face, _, _ = MT.texel_faces(np.arange(Ha * Wa), m, T, layout[1], Wa)
    assert np.array_equal(np.where(face < m, face, -1).reshape(Ha, Wa), owner)
    uv = MT.face_uv(m, T)
    assert uv.dtype == np.float32 and uv.shape == (3 * m, 2)
    want = np.stack([(corners[..., 0] + 0.5) / Wa, 1.0 - (corners[..., 1] + 0.5) / Ha], axis=-1).reshape(-1, 2)
    assert np.array_equal(uv, want.astype(np.float32))
    # the bilinear footprint of any point of a triangle: the taps with a weight lie in texels of the triangle's own face
    rng = np.random.default_rng(m * 100 + T)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=(m, 2000))              # (m, samples, 3) barycentrics, inside the triangle
    xy = np.einsum("msc,mcd->msd", w, corners.astype(np.float64))   # texel-centre coordinates
    x0, y0 = np.floor(xy[..., 0]).astype(np.int64), np.floor(xy[..., 1]).astype(np.int64)
    fx, fy = xy[..., 0] - x0, xy[..., 1] - y0
    mine = np.arange(m)[:, None]
    for dx, wx in ((0, 1.0 - fx), (1, fx)):
        for dy, wy in ((0, 1.0 - fy), (1, fy)):
            used = wx * wy > 0
            X, Y = np.where(used, x0 + dx, corners[:, :1, 0]), np.where(used, y0 + dy, corners[:, :1, 1])
            assert (X >= 0).all() and (X < Wa).all() and (Y >= 0).all() and (Y < Ha).all()
            assert (owner[Y, X] == mine).all()


# ---- 4: the host path per texel against float64 ----

def restate64(scene, views, depths, T, depth_tol, min_cos, power, two_sided=False, z_min=0.0, fill=0.5, vertex_colors=None):
    """Rules 2-5 in float64 on the fp32 inputs, written from the header's text and sharing no code with the module.  Per texel of the
    atlas: owned, seen, value (3,) before quantisation, excluded (some decision lies inside its fp32 rounding band), point (3,),
    inside (the texel's centre lies in its triangle)."""
    v, f = scene["vertices"].astype(np.float64), scene["faces"].astype(np.int64)
    n, m = len(v), len(f)
    _, cols, rows, Ha, Wa = _layout(m, T)
    Y, X = np.meshgrid(np.arange(Ha), np.arange(Wa), indexing="ij")
    i, j = X % (T + 1), Y % T
    k = (Y // T) * cols + X // (T + 1)
    B = i + j >= T
    face = 2 * k + B
    owned = face < m
    beta = np.where(B, T - i, i) / (T - 2.0)
    gamma = np.where(B, T - 1 - j, j) / (T - 2.0)
    idx = f[np.where(owned, face, 0)]
    in_range = owned & ((idx >= 0) & (idx < n)).all(axis=-1)
    idx = np.where(in_range[..., None], idx, 0)
    a, b, c = v[idx[..., 0]], v[idx[..., 1]], v[idx[..., 2]]
    with np.errstate(all="ignore"):
        p = a + beta[..., None] * (b - a) + gamma[..., None] * (c - a)
        nrm = np.cross(b - a, c - a)
        length = np.linalg.norm(nrm, axis=-1)
        live = in_range & np.isfinite(a).all(-1) & np.isfinite(b).all(-1) & np.isfinite(c).all(-1) & np.isfinite(length) & (length > 0)
        sum_c, sum_w = np.zeros((Ha, Wa, 3)), np.zeros((Ha, Wa))
        excluded = np.zeros((Ha, Wa), bool)
        for view, D in zip(views, depths):
            P = np.asarray(view.P, np.float64).reshape(3, 4)
            image, D = np.asarray(view.image, np.float64), np.asarray(D, np.float64)
            H, W = D.shape
            centre = -np.linalg.inv(P[:, :3]) @ P[:, 3]
            q = p @ P[:, :3].T + P[:, 3]
            z = q[..., 2]
            go = live & (z > z_min)
            excluded |= live & (np.abs(z - z_min) < BAND_Z)
            x, y = q[..., 0] / z, q[..., 1] / z
            border = np.minimum(np.minimum(np.abs(x), np.abs(x - (W - 1))), np.minimum(np.abs(y), np.abs(y - (H - 1))))
            excluded |= go & (border < BAND_PX)
            go &= (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
            d = centre - p
            cos = (nrm * d).sum(-1) / (length * np.linalg.norm(d, axis=-1))
            if two_sided:
                cos = np.abs(cos)
            excluded |= go & (np.abs(cos - min_cos) < BAND_COS)
            go &= cos >= min_cos
            # which four pixels: a projection within the band of a pixel row or column may take the neighbouring footprint in fp32
            excluded |= go & ((np.abs(x - np.rint(x)) < BAND_PX) | (np.abs(y - np.rint(y)) < BAND_PX))
            x0 = np.minimum(np.floor(np.where(go, x, 0)).astype(np.int64), W - 2)
            y0 = np.minimum(np.floor(np.where(go, y, 0)).astype(np.int64), H - 2)
            u, t = x - x0, y - y0
            vis = go.copy()
            for dy in (0, 1):
                for dx in (0, 1):
                    Dt = D[y0 + dy, x0 + dx]
                    excluded |= go & (Dt > 0) & (np.abs(np.abs(z - Dt) - depth_tol) < BAND_Z * np.maximum(1.0, np.abs(z)))
                    vis &= (Dt > 0) & (np.abs(z - Dt) <= depth_tol)
            top = (1 - u)[..., None] * image[y0, x0] + u[..., None] * image[y0, x0 + 1]
            bot = (1 - u)[..., None] * image[y0 + 1, x0] + u[..., None] * image[y0 + 1, x0 + 1]
            col = (1 - t)[..., None] * top + t[..., None] * bot
            w = np.where(vis, cos ** power, 0.0)
            sum_c += np.where(vis[..., None], w[..., None] * col, 0.0)
            sum_w += w
        seen = owned & (sum_w > 0)
        value = np.full((Ha, Wa, 3), float(fill))
        value = np.where(seen[..., None], sum_c / np.where(seen, sum_w, 1.0)[..., None], value)
        if vertex_colors is not None:
            s = beta + gamma
            bc, gc = np.where(s > 1, beta / s, beta), np.where(s > 1, gamma / s, gamma)
            vc = vertex_colors.astype(np.float64) / 255.0
            mix = (1 - bc - gc)[..., None] * vc[idx[..., 0]] + bc[..., None] * vc[idx[..., 1]] + gc[..., None] * vc[idx[..., 2]]
            value = np.where((in_range & ~seen)[..., None], mix, value)
    inside = owned & (beta + gamma <= 1 + 1e-12)
    return {"owned": owned, "seen": seen, "value": value, "excluded": excluded & owned, "point": p, "inside": inside, "face": face}


HOST_CASES = [("cube3", 33, 4), ("cube3", 3, 5), ("cube8", 17, 8), ("cube8", 1, 4), ("quads", 33, 8), ("quads", 16, 5),
              ("bad", 17, 5), ("bad", 3, 16), ("single", 16, 8), ("single", 33, 16)]
SETTINGS = {"default": dict(power=4, two_sided=False), "two_sided": dict(power=1, two_sided=True)}


@functools.lru_cache(maxsize=None)
def baked(name, count, T, setting="default", colours=False):
    """(host result with sums, float64 restatement) of a case, computed once."""
    scene = S.scenes()[name]
    views, depths = S.views_of(name, count)
    vc = S.vertex_colours(name) if colours else None
    kw = dict(depth_tol=S.DEPTH_TOL, min_cos=S.MIN_COS, **SETTINGS[setting])
    st = {}
    got = MT.bake_texture(scene["vertices"], scene["faces"], views, texels_per_edge=T, vertex_colors=vc, mesh_depths=depths,
                          stats=st, return_sums=True, **kw)
    return got, restate64(scene, views, depths, T, vertex_colors=vc, **kw), st


def _compare(name, count, T, setting="default", colours=False):
    (uv, atlas, sum_rgb, sum_w), ref, st = baked(name, count, T, setting, colours)
    owned, keep = ref["owned"], ref["owned"] & ~ref["excluded"]
    share = ref["excluded"].sum() / owned.sum()
    assert share <= EXCLUDED_CAP, f"scene condition: {share:.4f} of the owned texels lie inside a rounding band"
    assert np.array_equal((sum_w > 0) & keep, ref["seen"] & keep)
    want = np.minimum(np.maximum(ref["value"] * 256.0, 0.0), 255.0)
    levels = np.abs(atlas.astype(np.float64) - np.floor(want)).max(axis=-1)
    assert levels[keep].max() <= 1, f"{levels[keep].max()} levels apart"
    assert (atlas[~owned] == 128).all()                             # texels of no face: fill = 0.5
    assert st["texels_owned"] == int(owned.sum()) and st["texels_seen"] == int((sum_w > 0)[owned].sum())
    assert st["faces"] == len(S.scenes()[name]["faces"]) and st["views"] == count and st["atlas"] == list(atlas.shape[:2])
    return share, float(ref["seen"].sum() / owned.sum())


@pytest.mark.parametrize("name,count,T", HOST_CASES)
def test_host_equals_float64_restatement(name, count, T):
    share, seen = _compare(name, count, T)
    print(f"[texture] {name} K={count} T={T}: excluded {share:.4%}, seen {seen:.2%}")
    if name != "bad" and count >= 16:
        assert seen > 0.2                                           # the scene shows something


@pytest.mark.parametrize("name,count,T", [("cube3", 17, 8), ("quads", 17, 4), ("bad", 16, 8)])
def test_host_equals_float64_restatement_two_sided_with_vertex_colours(name, count, T):
    _compare(name, count, T, "two_sided", True)


# ---- 5: ground truth ----

@pytest.mark.parametrize("name,count,T", [("cube3", 33, 4), ("cube8", 17, 8), ("quads", 33, 8)])
def test_baked_colour_is_the_paint(name, count, T):
    """The baked colour of the in-triangle seen texels against the paint at the texel's point.  Tolerance: 1.5 x the largest
    deviation of the float64 restatement from the paint on the scene (its bilinear interpolation of the 23 x 31 and 37 x 53
    photographs) + 1/256.  Measured (largest |baked - paint|, restatement's deviation, tolerance):
        cube3 K=33 T=4: 0.0110, 0.0096, 0.0183      cube8 K=17 T=8: 0.0159, 0.0140, 0.0248      quads K=33 T=8: 0.0039, 0.0002, 0.0042
    (the quads are flat and their paint is nearly linear across a pixel, so bilinear interpolation is nearly exact there and what
    is left is the quantiser's floor)."""
    (uv, atlas, sum_rgb, sum_w), ref, _ = baked(name, count, T)
    scene = S.scenes()[name]
    sel = ref["inside"] & ref["seen"] & (sum_w > 0) & ~ref["excluded"]
    assert sel.sum() > 0.2 * ref["inside"].sum()
    paint = np.zeros(sel.shape + (3,))
    group = scene["paint"][np.where(ref["owned"], ref["face"], 0)]
    for p, fn in enumerate(S.PAINTS):
        paint = np.where((group == p)[..., None], fn(np.nan_to_num(ref["point"])), paint)
    own = np.abs(ref["value"] - paint)[sel].max()
    assert own < 0.05, f"scene condition: the restatement itself is {own:.4f} off the paint, the photographs are too coarse"
    tol = 1.5 * own + 1.0 / 256.0
    got = np.abs(atlas.astype(np.float64) / 256.0 - paint)[sel].max()
    print(f"[texture] {name} K={count} T={T}: baked {got:.4f}, restatement {own:.4f}, tolerance {tol:.4f}")
    assert got <= tol, f"baked colour {got:.4f} off the paint, restatement {own:.4f}, tolerance {tol:.4f}"
    if name == "quads":
        # occlusion: the back quad lies in the front quad's shadow for the cameras that face it; what is seen of it is blue
        back = sel & (group == 2)
        hidden = back & (np.abs(ref["point"][..., 1]) < 0.4) & (np.abs(ref["point"][..., 2]) < 0.4)
        assert back.sum() > 0 and hidden.sum() > 0
        rgb = atlas.astype(np.float64) / 256.0
        assert (rgb[back][:, 2] > 0.6).all() and (rgb[back][:, 0] < 0.4).all()
        front = sel & (group == 1)
        assert (rgb[front][:, 0] > 0.6).all() and (rgb[front][:, 2] < 0.4).all()


# ---- 6: fill ----

def test_unseen_texels_are_filled_and_nothing_raises():
    scene = S.scenes()["bad"]
    v, f = scene["vertices"], scene["faces"]
    views, depths = S.views_of("bad", 3)
    vc = S.vertex_colours("bad")
    T = 5
    _, cols, _, Ha, Wa = MT.atlas_layout(len(f), T)
    poisoned = np.full((Ha, Wa, 4), np.nan, np.float32)
    uv, atlas, sum_rgb, sum_w = MT.bake_texture(v, f, views, texels_per_edge=T, depth_tol=S.DEPTH_TOL, mesh_depths=depths,
                                                return_sums=True, sums=poisoned, fill=0.25)
    assert np.isfinite(poisoned).all() and np.array_equal(poisoned[..., 3], sum_w)          # fully written, in place
    face, bi, gi = MT.texel_faces(np.arange(Ha * Wa), len(f), T, cols, Wa)
    face = face.reshape(Ha, Wa)
    drawable = S.drawable_faces(scene)
    dead = (face < len(f)) & ~drawable[np.minimum(face, len(f) - 1)]
    assert dead.sum() == 5 * T * (T + 1) // 2
    assert (sum_w[dead] == 0).all() and (atlas[dead] == 64).all() and (atlas[face >= len(f)] == 64).all()
    assert (atlas[(face < len(f)) & (sum_w == 0)] == 64).all() and (sum_w > 0).any()
    # with vertex colours: the mix where the indices allow one, the constant for the two faces with an index out of range
    _, mixed, _, sum_w2 = MT.bake_texture(v, f, views, texels_per_edge=T, depth_tol=S.DEPTH_TOL, mesh_depths=depths, vertex_colors=vc,
                                          return_sums=True, fill=0.25)
    assert np.array_equal(sum_w2, sum_w) and np.array_equal(mixed[sum_w > 0], atlas[sum_w > 0])
    in_range = ((f >= 0) & (f < len(v))).all(axis=1)
    outside = (face < len(f)) & ~in_range[np.minimum(face, len(f) - 1)]
    assert outside.sum() == 2 * T * (T + 1) // 2 and (mixed[outside] == 64).all()
    corner = np.zeros((Ha, Wa), bool)                               # corner 0 of every A face: beta = gamma = 0, its vertex's colour
    ks = np.arange((len(f) + 1) // 2)
    corner[(ks // cols) * T, (ks % cols) * (T + 1)] = True
    sel = corner & (sum_w == 0) & ~outside
    assert sel.sum() > 0
    assert np.array_equal(mixed[sel], vc[f[face[sel], 0]])
    # no view at all: everything is filled
    _, none = MT.bake_texture(v, f, [], depth_tol=0.1, mesh_depths=[])
    assert (none == 128).all()
    uv0, empty = MT.bake_texture(v, np.zeros((0, 3), np.int32), views, depth_tol=0.1, mesh_depths=depths)
    assert uv0.shape == (0, 2) and empty.shape == (0, 0, 3)


# ---- 7: OBJ ----

def test_obj_round_trip(tmp_path):
    scene = S.scenes()["cube3"]
    (uv, atlas, _, _), _, _ = baked("cube3", 3, 5)
    v = (scene["vertices"] * np.float32(1234.567) + np.float32(1e-3)).astype(np.float32)
    paths = mesh_io.write_obj(str(tmp_path / "out" / "mesh_textured.obj"), v, scene["faces"], uv, atlas)
    assert [os.path.basename(p) for p in paths] == ["mesh_textured.obj", "mesh_textured.mtl", "mesh_textured.png"]
    assert all(os.path.exists(p) for p in paths)
    text = open(paths[0]).read()
    assert "mtllib mesh_textured.mtl" in text and re.search(r"\nf \d+/1 \d+/2 \d+/3\n", text) and "\nvt " in text and "\nv " in text
    assert "map_Kd mesh_textured.png" in open(paths[1]).read()
    back = mesh_io.read_obj(paths[0])
    assert np.array_equal(back["vertices"], v) and np.array_equal(back["faces"], scene["faces"])
    assert np.array_equal(back["uv"], uv) and back["normals"] is None
    assert np.array_equal(back["atlas"], atlas)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(paths[2])), atlas)
    nrm = np.random.default_rng(0).normal(size=v.shape).astype(np.float32)
    back = mesh_io.read_obj(mesh_io.write_obj(str(tmp_path / "n.obj"), v, scene["faces"], uv, atlas, normals=nrm)[0])
    assert np.array_equal(back["normals"], nrm) and np.array_equal(back["faces"], scene["faces"]) and np.array_equal(back["uv"], uv)
    with pytest.raises(ValueError, match="uv"):
        mesh_io.write_obj(str(tmp_path / "bad.obj"), v, scene["faces"], uv[:-1], atlas)
    with pytest.raises(ValueError, match="out of range"):
        mesh_io.write_obj(str(tmp_path / "bad.obj"), v[:5], scene["faces"], uv, atlas)


# ---- 8: the scripts ----

def test_script_flags_and_view_from_item():
    import torch
    fuse_scene, dtu_chamfer = _script("fuse_scene"), _script("dtu_chamfer")
    base = ["--conf", "c"]
    a = fuse_scene.parse_args(base)
    assert a.texture is False and fuse_scene.texture_params(a, 1.5) is None
    a = fuse_scene.parse_args(base + ["--texture"])
    assert a.texture_backend == "device"
    assert fuse_scene.texture_params(a, 1.5) == dict(texels_per_edge=8, depth_tol=3.0, min_cos=0.2, power=4, two_sided=False,
                                                     z_min=0.0, fill=0.5)
    a = fuse_scene.parse_args(base + ["--texture", "--texture_texels", "5", "--texture_depth_tol_mm", "0.7", "--texture_min_cos",
                                      "0.4", "--texture_power", "2", "--texture_two_sided", "--texture_backend", "host"])
    assert fuse_scene.texture_params(a, 1.5) == dict(texels_per_edge=5, depth_tol=0.7, min_cos=0.4, power=2, two_sided=True,
                                                     z_min=0.0, fill=0.5)
    with pytest.raises(SystemExit, match="fuse_scene: bake_texture: texels_per_edge.*3"):
        fuse_scene.texture_params(fuse_scene.parse_args(base + ["--texture", "--texture_texels", "3"]), 1.0)
    chamfer = base + ["--eval_dir", "e"]
    assert dtu_chamfer.parse_args(chamfer).texture is False and dtu_chamfer.texture_params(dtu_chamfer.parse_args(chamfer), 1.0) is None
    got = dtu_chamfer.texture_params(dtu_chamfer.parse_args(chamfer + ["--texture", "--texture_power", "16"]), 0.5)
    assert got["depth_tol"] == 1.0 and got["power"] == 16
    with pytest.raises(SystemExit, match="dtu_chamfer: bake_texture: power.*17"):
        dtu_chamfer.texture_params(dtu_chamfer.parse_args(chamfer + ["--texture", "--texture_power", "17"]), 1.0)
    # view_from_item: the world-frame projection of photograph k at the photograph's own size
    rng = np.random.default_rng(3)
    H, W = 6, 8
    S_mat = np.eye(4)
    S_mat[:3, :3] *= 2.5
    S_mat[:3, 3] = [10.0, -4.0, 3.0]
    c2w = np.tile(np.eye(4), (2, 1, 1))
    c2w[1, :3, 3] = [0.3, 0.1, -2.0]
    K = np.tile(np.eye(4), (2, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 7.0, 7.5, 3.5, 2.5
    item = {"imgs": torch.from_numpy(rng.random((1, 2, 3, H, W)).astype(np.float32)), "scale_mat": torch.from_numpy(S_mat)[None],
            "intrs": torch.from_numpy(K)[None], "c2ws": torch.from_numpy(c2w)[None]}
    view = MT.view_from_item(item, 1)
    assert view.P.dtype == np.float32 and view.P.shape == (3, 4) and view.image.shape == (H, W, 3)
    assert np.array_equal(view.image, item["imgs"][0, 1].permute(1, 2, 0).numpy())
    Xn = np.array([0.2, -0.1, 0.4, 1.0])                            # a point of the normalised frame
    q = view.P.astype(np.float64) @ (S_mat @ Xn)
    cam = np.linalg.inv(c2w[1]) @ Xn
    assert np.allclose(q[:2] / q[2], (K[1, :3, :3] @ cam[:3])[:2] / cam[2], atol=1e-5)
    assert np.isclose(q[2], 2.5 * cam[2], rtol=1e-6)                # z in world units
