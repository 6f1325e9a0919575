"""The device path of the mesh cleaner (csrc/mesh_clean.hip, surf_amd.evaluation.clean_mesh backend="device") against the
host path, stage by stage, and against the reference's golden keep-masks (tests/golden/clean_mesh.npz).  Nothing here compares
the device path with itself.

The visual-hull kernel evaluates a fixed sequence of fp32 operations (written out in mesh_clean.hip's header); `_mirror_seen`
below is that sequence in numpy fp32 and the kernel must equal it for EVERY vertex.  The host function's matmuls have no defined
summation order, so host and golden are compared on the faces none of whose vertices is near a decision boundary
(`_near_boundary`, float64): within EPS = 1e-3 px of an integer pixel line in x or y while within one pixel of the image, or
depth within EPS of 0.  EPS is set against the fp32 rounding of a pixel coordinate near 800 (one ulp is 6e-5, the projection
accumulates a handful); at most 10 % of the faces may be excluded (the host code alone gives 4.2 % on the golden inputs and
5.8 % on the 1 M-face sphere with 5 views of 576x800).  Measured on an MI355X: 4.167 % and 5.679 % excluded, and of the excluded
faces none differed from the host function or the golden (the tests print the counts)."""
import math
import os

import numpy as np
import pytest
import torch

from surf_amd import _lib
from surf_amd.evaluation import clean_mesh as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-3
NEW_SYMBOLS = ["surf_clean_dilate", "surf_clean_hull_count", "surf_clean_face_keep", "surf_clean_mark_visible",
               "surf_clean_components_slots", "surf_clean_components", "surf_clean_mark_used", "surf_clean_compact_faces",
               "surf_clean_compact_rows"]


# ---- helpers ----------------------------------------------------------------------------------------------------------------

def _ring(azimuths, H, W, radius=2.5):
    """surf_amd.synthetic.ring_cameras for any list of azimuths."""
    c2ws, intrs = [], []
    for a in azimuths:
        o = torch.tensor([radius * math.sin(a), 0.0, -radius * math.cos(a)], dtype=torch.float32)
        z = -o / o.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), z)
        x = x / x.norm()
        y = torch.linalg.cross(z, x)
        c2w = torch.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, o
        K = torch.eye(4)
        K[0, 0] = K[1, 1] = 1.6 * W
        K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
        c2ws.append(c2w)
        intrs.append(K)
    return torch.stack(intrs), torch.stack(c2ws)


def _mirror_seen(vertices, masks, intrs, c2ws):
    """mesh_clean.hip's hull_kernel in numpy fp32, operation for operation: per-vertex number of seeing views (int32)."""
    f32 = np.float32
    v = np.asarray(vertices, dtype=f32)
    X, Y, Z = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
    masks = np.asarray(masks) > 0
    n_seen = np.zeros(len(v), dtype=np.int32)
    with np.errstate(all="ignore"):
        for m, K, c2w in zip(masks, intrs, c2ws):
            h, w = m.shape
            K = K.detach().to("cpu", torch.float32)[:3, :3].numpy()
            W = torch.inverse(c2w.detach().to("cpu", torch.float32))[:3, :4].numpy()
            cx = ((W[0, 0] * X + W[0, 1] * Y) + W[0, 2] * Z) + W[0, 3]
            cy = ((W[1, 0] * X + W[1, 1] * Y) + W[1, 2] * Z) + W[1, 3]
            cz = ((W[2, 0] * X + W[2, 1] * Y) + W[2, 2] * Z) + W[2, 3]
            u = (K[0, 0] * cx + K[0, 1] * cy) + K[0, 2] * cz
            vv = (K[1, 0] * cx + K[1, 1] * cy) + K[1, 2] * cz
            d = (K[2, 0] * cx + K[2, 1] * cy) + K[2, 2] * cz
            dc = np.maximum(d, f32(1e-8))
            px, py = u / dc, vv / dc
            inside = (px >= f32(0)) & (px <= f32(w - 1)) & (py >= f32(0)) & (py <= f32(h - 1)) & (d > f32(1e-8))
            far = f32(10.0) * f32(max(h, w))
            qx, qy = np.minimum(np.maximum(px, -far), far), np.minimum(np.maximum(py, -far), far)
            x0, y0 = np.floor(qx), np.floor(qy)
            fx, fy = qx - x0, qy - y0
            xi, yi = x0.astype(np.int64), y0.astype(np.int64)
            total = np.zeros(len(v), dtype=f32)
            for dy, wy in ((0, f32(1.0) - fy), (1, fy)):
                for dx, wx in ((0, f32(1.0) - fx), (1, fx)):
                    xx, yy = xi + dx, yi + dy
                    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                    tex = m[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(f32)
                    total = total + np.where(ok, (tex * wx) * wy, f32(0))
            assert px.dtype == f32 and total.dtype == f32
            n_seen += (inside & (total > 0)).astype(np.int32)
    return n_seen


def _near_boundary(vertices, intrs, c2ws, hw, eps=EPS):
    """(V,) bool, float64: in some view the vertex projects within eps px of an integer pixel line (x or y) while within one
    pixel of the image, or its depth is within eps of 0."""
    h, w = hw
    xyz1 = np.concatenate([np.asarray(vertices, dtype=np.float64), np.ones((len(vertices), 1))], axis=1)
    near = np.zeros(len(xyz1), dtype=bool)
    with np.errstate(all="ignore"):
        for K, c2w in zip(intrs, c2ws):
            uvw = (xyz1 @ np.linalg.inv(c2w.double().numpy()).T)[:, :3] @ K.double().numpy()[:3, :3].T
            d = uvw[:, 2]
            px, py = uvw[:, 0] / d, uvw[:, 1] / d
            close = (px >= -1) & (px <= w) & (py >= -1) & (py <= h)
            line = (np.abs(px - np.rint(px)) < eps) | (np.abs(py - np.rint(py)) < eps)
            near |= (close & line) | (np.abs(d) < eps) | ~np.isfinite(px) | ~np.isfinite(py)
    return near


def _face_keep(n_seen, faces, min_nb_visible):
    return (n_seen > min_nb_visible)[np.asarray(faces)].all(axis=-1)


def _golden():
    from tests.conftest import load_npz
    g = load_npz("clean_mesh.npz")
    return g["vertices"].numpy(), g["faces"].numpy(), g["masks"], g["intrs"], g["c2ws"], g


def _sphere_oracle(radius=0.5, n=36, centre=(0.0, 0.0, 0.0)):
    from oracle import mcubes_oracle as M
    ax = np.linspace(-1.2, 1.2, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = (1.0 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, t = M.marching_cubes(u, 0.0)
    return (v / (n - 1) * 2.4 - 1.2) * radius + np.asarray(centre)[None], t


def _sphere_gpu(res, radius=0.39, half=0.6):
    """Marching-cubes sphere from the project's own kernel: (vertices float64 (V,3), faces int64 (F,3)) numpy; res = 512 gives
    about 1.04 M faces."""
    from surf_amd import ops
    dev = torch.device("cuda:0")
    ax = torch.linspace(-half, half, res, device=dev)
    u = torch.empty(res, res, res, dtype=torch.float32, device=dev)
    y, z = torch.meshgrid(ax, ax, indexing="ij")
    for i in range(res):
        u[i] = radius - torch.sqrt(ax[i] * ax[i] + y * y + z * z)
    v, t = ops.marching_cubes(u, 0.0)
    del u
    v = v / (res - 1) * (2 * half) - half
    return v.cpu().numpy(), t.long().cpu().numpy()


def _holed_masks(nv, h, w, seed=0):
    """Masks with a border margin that differs per view, a rectangular hole each and a few random specks."""
    g = np.random.default_rng(seed)
    m = np.zeros((nv, h, w), dtype=bool)
    for i in range(nv):
        m[i, h // 12 + i:h - h // 10 - i, w // 14 + 2 * i:w - w // 16 - i] = True
        y0, x0 = int(g.integers(h // 4, h // 2)), int(g.integers(w // 4, w // 2))
        m[i, y0:y0 + h // 8, x0:x0 + w // 9] = False
        m[i][g.random((h, w)) < 0.002] ^= True
    return torch.from_numpy(m)


def _big_scene():
    v, t = _sphere_gpu(512)
    assert 0.9e6 < len(t) < 1.3e6
    intrs, c2ws = _ring([0.0, 0.25, -0.25, 0.5, -0.5], 576, 800)
    return v, t, _holed_masks(5, 576, 800), intrs, c2ws


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_new_entry_points_are_declared_bound_and_exported():
    """Fails on the parent commit: the surf_clean_* group is new.  The ABI version stays 41 (entry points added, none changed)."""
    with open(os.path.join(ROOT, "include", "surf_hip.h")) as f:
        header = f.read()
    assert "#define SURF_ABI_VERSION 41" in header and _lib.ABI_VERSION == 41
    L = _lib.lib()
    assert L.surf_abi_version() == 41
    for name in NEW_SYMBOLS:
        assert f" {name}(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name


def test_limits_are_reported_not_faulted():
    """Oversized requests come back as SURF_E_LIMIT through _lib.check before anything is launched or dereferenced."""
    L = _lib.lib()
    assert L.surf_clean_components_slots(1000) == 4096 and L.surf_clean_components_slots(1 << 20) == 1 << 22
    for n in (1 << 31, (1 << 31) + 5, 1 << 40):
        assert L.surf_clean_components_slots(n) == -2
        with pytest.raises(_lib.SurfHipError, match="limit"):
            _lib.check(int(L.surf_clean_components_slots(n)), "surf_clean_components_slots")
    assert L.surf_clean_components_slots((1 << 29) + 1) == -2           # the table would need 2^32 slots
    assert L.surf_clean_components_slots(1 << 29) == 1 << 31
    for call in (lambda: L.surf_clean_components(None, 1 << 31, 500, None, None, None, 0, None, None, None, None, None, None),
                 lambda: L.surf_clean_hull_count(None, 1 << 31, None, None, 1, 4, 4, None, None),
                 lambda: L.surf_clean_face_keep(None, None, 1 << 31, 1, None, None),
                 lambda: L.surf_clean_mark_used(None, None, 1 << 31, 10, None, None),
                 lambda: L.surf_clean_compact_faces(None, None, None, None, 10, 1 << 31, None, None),
                 lambda: L.surf_clean_compact_rows(None, 4, None, None, 1 << 31, None, None)):
        with pytest.raises(_lib.SurfHipError, match="limit"):
            _lib.check(call(), "surf_clean")
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        _lib.check(L.surf_clean_components(None, 10, 500, None, None, None, 0, None, None, None, None, None, None), "surf_clean")


def test_mirror_reproduces_the_reference_golden():
    """The numpy fp32 mirror of the kernel's operation order against the REFERENCE's keep-masks, on every face away from a
    decision boundary: pins the mirror before the kernel is compared with the mirror."""
    v, f, masks, intrs, c2ws, g = _golden()
    n_seen = _mirror_seen(v, masks.numpy(), intrs, c2ws)
    far_faces = ~_near_boundary(v, intrs, c2ws, masks.shape[1:])[f].any(axis=-1)
    excluded = 1.0 - far_faces.mean()
    print(f"golden: {excluded:.3%} of the faces excluded")
    assert excluded <= 0.10
    for m in (0, 1, 2):
        ref = g[f"keep{m}"].numpy().astype(bool)
        mine = _face_keep(n_seen, f, m)
        print(f"golden keep{m}: {int((mine != ref)[~far_faces].sum())} of the excluded faces differ")
        assert np.array_equal(mine[far_faces], ref[far_faces]), (m, int((mine != ref)[far_faces].sum()))


def test_host_path_is_the_default_and_rejects_unknown_backends():
    v, f, masks, intrs, c2ws, _ = _golden()
    with pytest.raises(ValueError):
        C.clean_mesh(v, f, masks, intrs, c2ws, backend="nowhere")
    with pytest.raises(ValueError):
        C.clean_mesh(v, f, masks, intrs, c2ws, return_tensors=True)


# ---- GPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_dilation_equals_dilate_disk():
    g = np.random.default_rng(0)
    h, w = 61, 83
    cases = [g.random((h, w)) < 0.01, g.random((h, w)) < 0.3, np.zeros((h, w), bool), np.ones((h, w), bool)]
    border = np.zeros((h, w), bool)
    border[0, 5] = border[h - 1, 40] = border[17, 0] = border[30, w - 1] = border[0, 0] = border[h - 1, w - 1] = True
    frame = np.zeros((h, w), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    cases += [border, frame]
    stack = np.stack(cases)
    for r in (0, 1, 3, 11):
        ref = np.stack([C.dilate_disk(m, r) for m in cases])
        got = C.dilate_disk_device(stack, r)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), ref), r
        assert np.array_equal(C.dilate_disk_device(cases[0], r).cpu().numpy(), ref[0])
    big = g.random((2, 576, 800)) < 0.001
    assert np.array_equal(C.dilate_disk_device(big, 11).cpu().numpy(), np.stack([C.dilate_disk(m, 11) for m in big]))


@pytest.mark.gpu
def test_visual_hull_count_equals_the_mirror_everywhere():
    """Every vertex, no exclusions: golden inputs, special positions, and the 1 M-face mesh."""
    v, f, masks, intrs, c2ws, _ = _golden()
    got = C.vertex_seen_count_device(v, masks, intrs, c2ws).cpu().numpy()
    ref = _mirror_seen(v, masks.numpy(), intrs, c2ws)
    assert got.dtype == np.int32 and np.array_equal(got, ref) and 0 < (ref > 1).sum() < len(ref)
    # vertices behind the camera, at depth 0, far outside, exactly on integer pixels and on the image border (view 0's frame)
    h, w = masks.shape[1:]
    K, c2w = intrs[0].double().numpy()[:3, :3], c2ws[0].double().numpy()
    pix = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, 17), (40, h - 1), (12, 30), (6, 4), (73, 55), (5.5, 3.5),
           (-1, 10), (w, 10), (10, -1), (10, h), (-0.5, -0.5), (w - 0.5, h - 0.5), (1e6, 1e6), (-1e7, 3), (30, 26), (41.999, 35.999)]
    special = []
    for depth in (2.5, 1.0, 0.0, 1e-9, -1.0, -2.5, 1e-7):
        for x, y in pix:
            cam = np.linalg.inv(K) @ np.array([x, y, 1.0]) * depth
            special.append(c2w[:3, :3] @ cam + c2w[:3, 3])
    special = np.array(special + [[1e8, -1e8, 1e8], [0.0, 0.0, 0.0], c2w[:3, 3]])
    got = C.vertex_seen_count_device(special, masks, intrs, c2ws).cpu().numpy()
    assert np.array_equal(got, _mirror_seen(special, masks.numpy(), intrs, c2ws))
    v, t, masks, intrs, c2ws = _big_scene()
    got = C.vertex_seen_count_device(v, masks, intrs, c2ws).cpu().numpy()
    ref = _mirror_seen(v, masks.numpy(), intrs, c2ws)
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert len(np.unique(ref)) >= 4                                   # the holed masks make the count vary


def _hull_against_host(v, f, masks, intrs, c2ws, label, golden=None):
    far_faces = ~_near_boundary(v, intrs, c2ws, masks.shape[1:])[f].any(axis=-1)
    excluded = 1.0 - far_faces.mean()
    print(f"{label}: {excluded:.3%} of the faces excluded (near a decision boundary)")
    assert excluded <= 0.10
    proper = False
    for m in (0, 1, 2):
        host = C.clean_mesh_by_mask(v, f, masks, intrs, c2ws, m)
        dev = C.clean_mesh_by_mask_device(v, f, masks, intrs, c2ws, m)
        assert dev.dtype == torch.bool
        dev = dev.cpu().numpy()
        print(f"{label} min_nb_visible={m}: {int((dev != host)[~far_faces].sum())} of {int((~far_faces).sum())} excluded faces differ "
              f"from the host function")
        assert np.array_equal(dev[far_faces], host[far_faces]), (label, m, int((dev != host)[far_faces].sum()))
        assert host.sum() > 0
        proper = proper or host.sum() < len(host)
        if golden is not None:
            ref = golden[f"keep{m}"].numpy().astype(bool)
            print(f"{label} min_nb_visible={m}: {int((dev != ref)[~far_faces].sum())} excluded faces differ from the golden")
            assert np.array_equal(dev[far_faces], ref[far_faces]), (label, m)
    assert proper, "the masks should make the hull test drop some face for some min_nb_visible"


@pytest.mark.gpu
def test_visual_hull_keep_equals_host_and_golden_off_the_boundary_band():
    v, f, masks, intrs, c2ws, g = _golden()
    _hull_against_host(v, f, masks, intrs, c2ws, "golden", g)
    v, t, masks, intrs, c2ws = _big_scene()
    _hull_against_host(v, t, masks, intrs, c2ws, "1M-face sphere")


@pytest.mark.gpu
def test_visible_faces_equal_the_host_function():
    v, t = _sphere_oracle(0.5, 40)
    v2, t2 = _sphere_oracle(0.12, 12, centre=(0.15, 0.1, -0.8))
    vv, ff = np.concatenate([v, v2]), np.concatenate([t, t2 + len(v)])
    h, w = 96, 128
    intrs, c2ws = _ring([0.0, 0.25, -0.25, math.pi], h, w)
    c2ws[3, :3, 2] *= -1                                              # the fourth camera looks away: nothing is hit
    c2ws[3, :3, 0] *= -1
    masks = _holed_masks(4, h, w, seed=3)
    for up in (1, 2, 3, 4):
        host = C.visible_faces(vv, ff, masks, intrs, c2ws, up, "cuda")
        dev = C.visible_faces_device(vv, ff, masks, intrs, c2ws, up)
        assert dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), host), up
        assert 0 < host.sum() < len(host)
        alone = C.visible_faces(vv, ff, masks[3:], intrs[3:], c2ws[3:], up, "cuda")
        assert not alone.any() and not C.visible_faces_device(vv, ff, masks[3:], intrs[3:], c2ws[3:], up).any()
    fm = masks.float() * 0.3                                           # float masks: "set" is > 0, as on the host
    assert np.array_equal(C.visible_faces_device(vv, ff, fm, intrs, c2ws, 2).cpu().numpy(), C.visible_faces(vv, ff, fm, intrs, c2ws, 2))


def _floaters(n, faces_each_res, seed, offset):
    """n small spheres (marching cubes at faces_each_res^3) as one face array with vertex ids from `offset`."""
    v, t = _sphere_oracle(0.02, faces_each_res)
    fs = [t + offset + i * len(v) for i in range(n)]
    return np.concatenate(fs), n * len(v), len(t)


def _cc_check(faces, min_lens):
    for ml in min_lens:
        host = C.face_components(faces, ml)
        dev = C.face_components_device(faces, ml)
        assert dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), host), (ml, int((dev.cpu().numpy() != host).sum()))


@pytest.mark.gpu
def test_components_equal_face_components():
    _, t = _sphere_oracle(0.5, 40)
    nv_sphere = int(t.max()) + 1
    small, nvs, n_small = _floaters(7, 8, 0, nv_sphere)
    medium, _, n_medium = _floaters(3, 16, 1, nv_sphere + nvs)
    assert n_small < 500 < n_medium < len(t)
    faces = np.concatenate([t, small, medium])
    _cc_check(faces, (1, 2, 500, n_medium, n_medium + 1, len(t), len(t) + 1, len(faces) + 10, 1 << 40))
    host = C.face_components(faces, 500)
    assert host[:len(t)].all() and not host[len(t):len(t) + len(small)].any() and host[len(t) + len(small):].all()
    # isolated faces: no neighbour, dropped even at min_len = 1
    iso = np.arange(30).reshape(10, 3)
    _cc_check(iso, (1, 2))
    assert not C.face_components_device(iso, 1).any()
    # a fan of four faces on one edge (0, 1), plus one isolated face
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 1, 0], [6, 7, 8]])
    _cc_check(fan, (1, 2, 4, 5))
    assert C.face_components_device(fan, 4).cpu().numpy().tolist() == [True, True, True, True, False]
    # two components that touch in one vertex only are not joined
    touch = np.array([[0, 1, 2], [1, 2, 3], [3, 4, 5], [4, 5, 6]])
    _cc_check(touch, (1, 2, 3, 4))
    assert not C.face_components_device(touch, 3).any() and C.face_components_device(touch, 2).all()
    # degenerate faces (an edge listed twice by one face) and duplicates
    odd = np.array([[0, 0, 1], [2, 3, 2], [4, 5, 6], [4, 5, 6], [7, 7, 7], [8, 9, 10]])
    _cc_check(odd, (1, 2, 3))
    # random triangle soup, as tests/golden/make_golden_clean.py draws its faces
    g = torch.Generator().manual_seed(5)
    soup = torch.randint(0, 4000, (9000, 3), generator=g).numpy()
    _cc_check(soup, (1, 2, 5, 500, 9001))
    soup2 = torch.randint(0, 300, (2000, 3), generator=g).numpy()     # dense: most edges shared by several faces
    _cc_check(soup2, (1, 2, 500, 1999, 2001))
    assert C.face_components_device(np.zeros((0, 3), dtype=np.int64), 1).shape == (0,)


@pytest.mark.gpu
def test_components_of_a_permuted_1m_face_mesh_are_deterministic():
    v, t = _sphere_gpu(512)
    small, nvs, n_small = _floaters(200, 8, 0, len(v))
    faces = np.concatenate([t, small])
    faces = faces[np.random.default_rng(1).permutation(len(faces))]
    host = C.face_components(faces, 500)
    assert host.sum() == len(t) and n_small < 500
    from surf_amd import ops
    f = torch.from_numpy(faces).to("cuda", torch.int32).contiguous()
    outs = [ops.clean_components(f, 500, return_labels=True) for _ in range(3)]   # a plain repeat: determinism under atomics
    for keep, root, size in outs:
        assert np.array_equal(keep.cpu().numpy(), host)
        assert torch.equal(root, outs[0][1]) and torch.equal(size.gather(0, root.long()), outs[0][2].gather(0, outs[0][1].long()))
    root = outs[0][1].cpu().numpy()
    assert (root <= np.arange(len(faces))).all() and len(np.unique(root)) == 201
    first = np.full(len(faces), len(faces))
    np.minimum.at(first, root, np.arange(len(faces)))
    assert np.array_equal(first[root], root)                          # a component's label is its smallest face id


@pytest.mark.gpu
def test_compaction_equals_update_faces():
    v, t = _sphere_oracle(0.5, 30)
    g = np.random.default_rng(2)
    for keep in (g.random(len(t)) < 0.3, g.random(len(t)) < 0.97, np.ones(len(t), bool), np.arange(len(t)) == 7):
        for dt in (np.float32, np.float64):
            hv, hf = C.update_faces(v.astype(dt), t, keep)
            dv, df = C.update_faces_device(v.astype(dt), t, keep)
            assert dv.dtype == {np.float32: torch.float32, np.float64: torch.float64}[dt] and df.dtype == torch.int64
            assert np.array_equal(dv.cpu().numpy(), hv) and np.array_equal(df.cpu().numpy(), hf)
    hv, hf = C.update_faces(v, t, np.zeros(len(t), bool))
    dv, df = C.update_faces_device(v, t, np.zeros(len(t), bool))
    assert dv.shape == (0, 3) == hv.shape and df.shape == (0, 3) == hf.shape and dv.dtype == torch.float64
    dv, df = C.update_faces_device(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(keep).cuda())
    assert np.array_equal(dv.cpu().numpy(), C.update_faces(v, t, keep)[0])


def _both_backends(vv, ff, masks, intrs, c2ws, **kw):
    hv, hf = C.clean_mesh(vv, ff, masks, intrs, c2ws, **kw)
    dv, df = C.clean_mesh(vv, ff, masks, intrs, c2ws, backend="device", **kw)
    assert isinstance(dv, np.ndarray) and dv.dtype == hv.dtype and df.dtype == hf.dtype
    assert np.array_equal(dv, hv) and np.array_equal(df, hf), (hv.shape, dv.shape, hf.shape, df.shape)
    tv, tf = C.clean_mesh(torch.from_numpy(vv).cuda(), torch.from_numpy(ff).cuda(), masks.cuda(), intrs, c2ws, backend="device",
                          return_tensors=True, **kw)
    assert tv.is_cuda and tf.is_cuda and tv.dtype == torch.from_numpy(vv).dtype
    assert np.array_equal(tv.cpu().numpy(), hv) and np.array_equal(tf.cpu().numpy(), hf)
    return hv, hf


@pytest.mark.gpu
def test_clean_mesh_device_equals_host_on_the_full_mask_scene():
    """The scene of tests/test_evaluation.py::test_clean_mesh_drops_hidden_faces_and_small_components."""
    from surf_amd import synthetic
    v, t = _sphere_oracle(0.5, 40)
    v2, t2 = _sphere_oracle(0.06, 8, centre=(0.0, 0.62, 0.0))
    vv, ff = np.concatenate([v, v2]), np.concatenate([t, t2 + len(v)])
    intrs, c2ws, _ = synthetic.ring_cameras(3, 96, 128)
    masks = torch.ones(3, 96, 128)
    # The float64 rule of _near_boundary, on the pixel lines that decide anything here: with full masks every texel is set, so
    # an interior pixel line separates nothing, and the only decision boundaries are the image frame (px = 0 and w-1 of the
    # inside test, px = -1 and w of the bilinear footprint; likewise in y: the floater straddles the lower frame) and depth 0.
    # (The literal rule also flags the ~1 % of vertices that happen to lie within EPS of an interior line.)
    xyz1 = np.concatenate([vv, np.ones((len(vv), 1))], axis=1)
    for K, c2w in zip(intrs, c2ws):
        uvw = (xyz1 @ np.linalg.inv(c2w.double().numpy()).T)[:, :3] @ K.double().numpy()[:3, :3].T
        px, py = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
        assert uvw[:, 2].min() > 1.0
        for line in (-1, 0, 127, 128):
            assert np.abs(px - line).min() >= EPS
        for line in (-1, 0, 95, 96):
            assert np.abs(py - line).min() >= EPS
    print("full-mask scene: vertices within EPS of some interior pixel line:", int(_near_boundary(vv, intrs, c2ws, (96, 128)).sum()))
    kw = dict(dilation_radius=3, min_nb_visible=1, upscale=2, min_component=500)
    hv, hf = _both_backends(vv, ff, masks, intrs, c2ws, **kw)
    assert 0.2 * len(t) < len(hf) < 0.8 * len(t)
    hv32, _ = _both_backends(vv.astype(np.float32), ff, masks, intrs, c2ws, **kw)
    assert hv32.dtype == np.float32


@pytest.mark.gpu
def test_clean_mesh_device_equals_host_on_an_8_view_holed_scene():
    v, t = _sphere_oracle(0.5, 48)
    parts, off = [(v, t)], len(v)
    for i, c in enumerate([(0.0, 0.62, 0.0), (0.3, -0.6, -0.2), (-0.62, 0.1, -0.1), (0.1, 0.2, -0.7)]):
        v2, t2 = _sphere_oracle(0.05, 8 + 2 * i, centre=c)
        parts.append((v2, t2 + off))
        off += len(v2)
    vv, ff = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    h, w = 96, 128
    intrs, c2ws = _ring([0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0], h, w)
    masks = _holed_masks(8, h, w, seed=4).float()
    # move the near-boundary vertices off the band (the dilated masks' edges make the decisions band-dependent there)
    g = np.random.default_rng(9)
    for _ in range(50):
        near = _near_boundary(vv, intrs, c2ws, (h, w))
        if not near.any():
            break
        vv[near] += g.normal(0.0, 2e-4, (int(near.sum()), 3))
    assert not _near_boundary(vv, intrs, c2ws, (h, w)).any()
    kw = dict(dilation_radius=2, min_nb_visible=1, upscale=2, min_component=500)
    hv, hf = _both_backends(vv, ff, masks, intrs, c2ws, **kw)
    assert 0 < len(hf) < len(t) and len(hv) < len(v)
    stage1 = C.clean_mesh_by_mask(vv, ff, torch.stack([torch.from_numpy(C.dilate_disk(m.numpy() > 0.5, 2)) for m in masks]),
                                  intrs, c2ws, 1)
    assert 0 < stage1.sum() < len(ff)                                  # the hull stage removes something by itself
    # the frustum stage on its own, numpy in and tensors in
    hv2, hf2 = C.clean_mesh_outside_frustum(vv, ff, masks, intrs, c2ws, 3, 100, "cuda")
    dv2, df2 = C.clean_mesh_outside_frustum_device(vv, ff, masks, intrs, c2ws, 3, 100)
    assert np.array_equal(dv2.cpu().numpy(), hv2) and np.array_equal(df2.cpu().numpy(), hf2)


@pytest.mark.gpu
def test_dtu_chamfer_clean_backend_device_equals_host(tmp_path):
    """scripts/dtu_chamfer.py --clean_mesh --clean_backend device on the synthetic DTU scene of tests/test_end_to_end_dtu.py:
    the same mesh file and the same numbers as --clean_backend host."""
    import json
    import sys

    from scipy.io import savemat
    from bench import surf_conf
    from surf_amd import conf, mesh_io, synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.evaluation import dtu_eval as E
    from surf_amd.surf import SuRF
    from tests.test_end_to_end_dtu import _write_scene
    dev = torch.device("cuda:0")
    H, W = 96, 128
    root = tmp_path / "dtu"
    _write_scene(root, H, W)
    dconf = conf.from_dict({"dataset_name": "DTUDataset", "data_dir": str(root), "scene": ["scan24"], "ref_view": [1], "light_idx": [3],
                            "num_src_view": 2, "val_res_level": 2, "factor": 1.0, "interval_scale": 1, "num_interval": 192,
                            "img_hw": [H, W], "total_views": 4})
    loader, _, _ = get_loader(dconf, "val", False, num_workers=0)
    np.random.seed(0)
    item = next(iter(loader))
    inputs = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in item.items()}
    inputs["mesh_resolution"] = 128
    torch.manual_seed(0)
    mcfg = surf_conf(base_dim=16)
    model = SuRF(conf.from_dict(mcfg)).to(dev).eval()
    model.logit_override = synthetic.sphere_logit
    with torch.no_grad():
        out = model("val", inputs, cos_anneal_ratio=1.0, step=0)
    vw = mesh_io.export_mesh(str(tmp_path / "mesh.ply"), out["vertices"], out["triangles"], item["scale_mat"])
    centre_w = item["scale_mat"].double().numpy()[:3, 3]
    r_world = float(np.linalg.norm(vw - centre_w[None], axis=1).mean())
    density = r_world / 60.0
    ev = tmp_path / "dtu_eval"
    os.makedirs(ev / "ObsMask")
    os.makedirs(ev / "Points" / "stl")
    surf = E.sample_mesh_points(vw, out["triangles"], density)
    radial = (surf - centre_w[None]) / np.linalg.norm(surf - centre_w[None], axis=1, keepdims=True)
    stl = surf + 6.0 * radial
    with open(ev / "Points" / "stl" / "stl024_total.ply", "wb") as f:
        f.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {len(stl)}\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n").encode())
        f.write(np.ascontiguousarray(stl, dtype="<f4").tobytes())
    lo, hi = centre_w - 2 * r_world, centre_w + 2 * r_world
    savemat(ev / "ObsMask" / "ObsMask24_10.mat", {"ObsMask": np.ones((64, 64, 64), np.uint8), "BB": np.stack([lo, hi]).astype(np.float32),
                                                  "Res": np.float32(4.0 * r_world / 63)})
    savemat(ev / "ObsMask" / "Plane24.mat", {"P": np.array([[0.0, 0.0, 1.0, -centre_w[2]]])})
    conf_path = tmp_path / "surf_synth.conf"
    conf_path.write_text(json.dumps({"model": mcfg, "val_dataset": {k: dconf[k] for k in dconf}}, indent=1))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import dtu_chamfer
    recs = {}
    for where in ("host", "device"):
        recs[where] = dtu_chamfer.run(dtu_chamfer.parse_args([
            "--conf", str(conf_path), "--eval_dir", str(ev), "--scan", "24", "--ref_view", "1", "--out_dir", str(tmp_path / where),
            "--mesh_resolution", "128", "--downsample_density", str(density), "--logit_override", "sphere", "--clean_mesh",
            "--clean_backend", where]))
        assert recs[where]["cleaned"] and recs[where]["clean_backend"] == where and recs[where]["seconds"]["clean"] > 0
    a, b = recs["host"], recs["device"]
    print("dtu_chamfer --clean_mesh: input triangles", len(out["triangles"]), "cleaned", a["triangles"], "seconds",
          a["seconds"]["clean"], b["seconds"]["clean"])
    assert 500 <= a["triangles"] < len(out["triangles"]) and a["vertices"] > 0          # a proper, non-empty subset
    for key in ("vertices", "triangles", "d2s", "s2d", "chamfer"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert np.isfinite(a["chamfer"])
    with open(a["mesh"], "rb") as fa, open(b["mesh"], "rb") as fb:
        assert fa.read() == fb.read()
