"""Scenes of tests/test_raster_kernel.py: what surf_raster_first_hit receives (fp32 vertices, int32 faces, the fp32 K and
inverse(c2w)[:3, :4] that ops.raster_first_hit forms on the host, h, w, Hup, Wup), plus the camera they came from.

A case is a dict: v (nv, 3) float32, f (nf, 3) int32, intr / c2w (4, 4) torch float32, K (3, 3) / w2c (3, 4) float32, h, w, up,
Hup, Wup, and per scene: `front` (lattice: number of front-layer faces), `banned` (faces that may never be returned: the later
copy of an exact duplicate, faces with a non-finite vertex), `alias` (later copy -> first copy), `base` (nonfinite: the name of
the case without the bad faces), `far` (closed: far-side faces), `tags` (builder scenes: face ids by what they are there for)."""
import functools
import math

import numpy as np
import torch

from oracle import mcubes_oracle as M


def host_camera(intr, c2w):
    """K and w2c exactly as ops.raster_first_hit forms them."""
    K = np.ascontiguousarray(intr.detach().to("cpu", torch.float32)[:3, :3].contiguous().numpy())
    w2c = np.ascontiguousarray(torch.inverse(c2w.detach().to("cpu", torch.float32))[:3, :4].contiguous().numpy())
    return K, w2c


def make(v, f, intr, c2w, h, w, up, **meta):
    K, w2c = host_camera(intr, c2w)
    return dict(v=np.ascontiguousarray(v, dtype=np.float32), f=np.ascontiguousarray(f, dtype=np.int32), intr=intr.float(), c2w=c2w.float(),
                K=K, w2c=w2c, h=h, w=w, up=up, Hup=h * up, Wup=w * up, **meta)


def _intr(f, cx, cy, skew=0.0):
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 1], K[0, 2], K[1, 2] = skew, cx, cy
    return K


def _sphere_mesh(radius, n, centre=(0.0, 0.0, 0.0)):
    ax = np.linspace(-1.2, 1.2, n)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    u = (1.0 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, t = M.marching_cubes(u, 0.0)
    return (v / (n - 1) * 2.4 - 1.2) * radius + np.asarray(centre)[None], t


# ---- blob: the sphere-plus-blob scene of test_evaluation.py ------------------------------------------------------------


@functools.lru_cache(None)
def blob_mesh():
    v, t = _sphere_mesh(0.5, 22)
    v2, t2 = _sphere_mesh(0.15, 10, centre=(0.2, 0.1, -0.9))
    t = np.concatenate([t, t2 + len(v)]).astype(np.int64)
    v = np.concatenate([v, v2])
    t[::5] = t[::5][:, [0, 2, 1]]                                      # both signs of the screen area
    return v, t


def blob_cameras(h, w):
    """Three ring cameras and a fourth with a skewed K and a rolled rotation."""
    from surf_amd import synthetic
    intrs, c2ws, _ = synthetic.ring_cameras(3, h, w)
    if h < 48:              # the ring looks down the mesh's symmetry planes: at a few dozen samples the centre row and column,
        intrs[:, 0, 2] += 0.137           # which run along mesh edges, would be several per cent of the image
        intrs[:, 1, 2] -= 0.093
    K = intrs[0].clone()
    K[0, 1] = 0.11 * w
    a = 0.4
    roll = torch.eye(4)
    roll[0, 0], roll[0, 1], roll[1, 0], roll[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    return torch.cat([intrs, K[None]]), torch.cat([c2ws, (c2ws[0] @ roll)[None]])


def _blob(h, w, up, cam, nf=None):
    v, t = blob_mesh()
    intrs, c2ws = blob_cameras(h, w)
    return make(v, t if nf is None else t[:nf], intrs[cam], c2ws[cam], h, w, up)


# ---- lattice: a closed front layer whose vertices sit on (or within 1e-6 of) the samples ------------------------------

LATTICE_K = ((11.3, 0.0, 3.37), (0.0, 11.3, 2.9), (0.0, 0.0, 1.0))


def _lift(sx, sy, d, h, w, Hup, Wup, K=LATTICE_K):
    """Sample coordinates -> camera-space points at depth d (float64; the caller casts to fp32)."""
    u = np.asarray(sx, np.float64) / ((Wup - 1) / (w - 1))
    v = np.asarray(sy, np.float64) / ((Hup - 1) / (h - 1))
    d = np.broadcast_to(np.asarray(d, np.float64), u.shape)
    return np.stack([(u - K[0][2]) * d / K[0][0], (v - K[1][2]) * d / K[1][1], d], -1)


def _layer(g, depth, jitter, h, w, Hup, Wup):
    n = 27
    jj, ii = np.meshgrid(np.arange(n), np.arange(n))                   # ii: row (y), jj: column (x)
    sx, sy = jj - 1.0, ii - 1.0
    if jitter > 0:
        sx = sx + g.normal(0.0, jitter, sx.shape)
        sy = sy + g.normal(0.0, jitter, sy.shape)
    v = _lift(sx.reshape(-1), sy.reshape(-1), depth, h, w, Hup, Wup)
    idx = lambda i, j: i * n + j
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = idx(i, j), idx(i, j + 1), idx(i + 1, j + 1), idx(i + 1, j)
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    tris = np.asarray(tris, np.int64)
    rot = g.integers(0, 3, len(tris))
    tris = np.stack([tris[np.arange(len(tris)), (rot + k) % 3] for k in range(3)], 1)
    return v, tris


@functools.lru_cache(None)
def _lattice_meshes(w, up):
    h = 7
    g = np.random.default_rng(0)
    out = []
    for t in range(6):
        vf, tf = _layer(g, 2.0 + 0.37 * t, 0.0 if t <= 2 else 1e-6, h, w, h * up, w * up)
        vb, tb = _layer(g, 5.0, 0.3, h, w, h * up, w * up)
        out.append((np.concatenate([vf, vb]), np.concatenate([tf, tb + len(vf)]), len(tf)))
    return out


def _lattice(t, w=8, up=3, run_up=None):
    v, f, front = _lattice_meshes(w, up)[t]
    return make(v, f, _intr(11.3, 3.37, 2.9), torch.eye(4), 7, w, up if run_up is None else run_up, front=front)


# ---- closed: a uv-sphere seen from outside ---------------------------------------------------------------------------


@functools.lru_cache(None)
def uv_sphere(stacks=10, slices=14, radius=0.5):
    v = [(0.0, radius, 0.0)]
    for i in range(1, stacks):
        th = math.pi * i / stacks
        for j in range(slices):
            ph = 2 * math.pi * j / slices
            v.append((radius * math.sin(th) * math.cos(ph), radius * math.cos(th), radius * math.sin(th) * math.sin(ph)))
    v.append((0.0, -radius, 0.0))
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    f = []
    for j in range(slices):
        f.append((0, ring(1, j + 1), ring(1, j)))
        f.append((len(v) - 1, ring(stacks - 1, j), ring(stacks - 1, j + 1)))
    for i in range(1, stacks - 1):
        for j in range(slices):
            f += [(ring(i, j), ring(i, j + 1), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i + 1, j))]
    f = np.asarray(f, np.int64)
    f[::4] = f[::4][:, [0, 2, 1]]
    return np.asarray(v, np.float64), f


def _closed():
    from surf_amd import synthetic
    v, f = uv_sphere()
    intrs, c2ws, _ = synthetic.ring_cameras(3, 24, 32)
    o = c2ws[1][:3, 3].double().numpy()
    centre = v[f].mean(axis=1)
    far = np.nonzero(((centre - o) * centre).sum(-1) > 0.02)[0]        # centroid normal points away from the camera, with margin
    return make(v, f, intrs[1], c2ws[1], 24, 32, 2, far=far)


# ---- edges of the rule, near, nonfinite: camera at the origin looking along +z ----------------------------------------

EK = ((20.0, 0.0, 4.3), (0.0, 20.0, 3.1), (0.0, 0.0, 1.0))
EH, EW, EUP = 8, 10, 3


class _Builder:
    def __init__(self, h=EH, w=EW, up=EUP, K=EK):
        self.h, self.w, self.up, self.K = h, w, up, K
        self.v, self.f, self.tags = [], [], {}

    def pts(self, xy, d):
        xy = np.asarray(xy, np.float64)
        p = _lift(xy[:, 0], xy[:, 1], d, self.h, self.w, self.h * self.up, self.w * self.up, self.K)
        n = len(self.v)
        self.v += [tuple(q) for q in p]
        return list(range(n, n + len(p)))

    def tri(self, xy, d, tag=None):
        i = self.pts(xy, np.asarray(d, np.float64) * np.ones(3))
        return self.face(i, tag)

    def face(self, i, tag=None):
        self.f.append(tuple(i))
        if tag:
            self.tags.setdefault(tag, []).append(len(self.f) - 1)
        return len(self.f) - 1

    def quad(self, x0, y0, x1, y1, d, tag=None):
        i = self.pts([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], d)
        return [self.face((i[0], i[1], i[2]), tag), self.face((i[0], i[2], i[3]), tag)]

    def case(self, **meta):
        return make(np.asarray(self.v), np.asarray(self.f), _intr(self.K[0][0], self.K[0][2], self.K[1][2]), torch.eye(4),
                    self.h, self.w, self.up, tags=self.tags, **meta)


def _plane_depth(P, x, y, b):
    """Depth at which the ray through sample (x, y) meets the plane of the three camera-space points P."""
    r = _lift([x], [y], 1.0, b.h, b.w, b.h * b.up, b.w * b.up, b.K)[0]
    n = np.cross(P[1] - P[0], P[2] - P[0])
    return float(n @ P[0] / (n @ r))


def _edges():
    b = _Builder()                                                     # 24 x 30 samples
    b.tri([(-100, -80), (200, -60), (30, 300)], 60.0, "huge")          # larger than the whole image, behind everything
    for k, (y, t) in enumerate([(3.5, 4e-4), (4.0, 5e-4), (5.25, 9e-4), (6.0, -7e-4)]):      # slivers thinner than 1e-3 sample
        b.tri([(2.3 + k, y), (19.7 + k, y + t / 2), (9.1, y + t)], 7.0 + k, "sliver")
    b.tri([(5.2, 7.3), (5.6, 7.4), (5.3, 7.8)], 6.0, "subsample")      # covers no sample
    b.tri([(6.9, 7.9), (7.2, 8.0), (7.0, 8.3)], 6.0, "subsample")      # covers sample (7, 8) alone
    b.tri([(9.0, 8.0), (9.6, 8.0), (9.0, 8.7)], 6.0, "subsample")      # a vertex on sample (9, 8)
    b.tri([(-9, 3), (-3, 5), (-5, 9)], 5.0, "off_left")
    b.tri([(33, 3), (39, 5), (35, 9)], 5.0, "off_right")
    b.tri([(3, -9), (5, -3), (9, -5)], 5.0, "off_top")
    b.tri([(3, 27), (5, 33), (9, 29)], 5.0, "off_bottom")
    i = b.pts([(12, 2), (17, 6)], 6.0)
    b.face((i[0], i[0], i[1]), "repeated")
    b.tri([(3, 10), (6, 13), (9, 16)], 6.0, "collinear")
    d = b.tri([(20.3, 1.2), (28.6, 2.1), (23.4, 8.8)], 3.0, "dup_first")
    for g, x in zip((1e-6, 1e-5, 1e-4, 1e-3), (1.5, 8.5, 15.5, 22.5)):                      # z-fighting layers
        b.quad(x, 17.4, x + 5.2, 22.7, 9.0, "zfight")
        b.quad(x, 17.4, x + 5.2, 22.7, 9.0 * (1 + g), "zfight")
    # a long slanted triangle from depth 1 to 50 and small triangles just in front of / behind it
    sl = b.pts([(1.0, 10.2), (28.4, 11.0), (14.0, 16.4)], [1.0, 50.0, 20.0])
    b.face(sl, "slanted")
    P = np.asarray([b.v[k] for k in sl])
    for n, (x, y) in enumerate([(6, 12), (10, 12), (14, 13), (18, 13), (12, 14), (16, 14)]):
        z = _plane_depth(P, x, y, b) * (0.97 if n % 2 == 0 else 1.03)
        b.tri([(x - 0.4, y - 0.3), (x + 0.5, y - 0.2), (x - 0.1, y + 0.6)], z, "before" if n % 2 == 0 else "behind")
    b.face(b.f[d], "dup_second")                                       # the exact duplicate, later in the list
    return b.case(banned=np.asarray(b.tags["dup_second"]), alias={b.tags["dup_second"][0]: b.tags["dup_first"][0]})


def _near():
    b = _Builder()
    b.quad(-2, -2, 14, 26, 4.0, "backdrop")                            # ordinary faces on the left part of the image
    for n, cz in enumerate([(0.0, 2.0, 2.0), (-1.0, 5e-7, 2.0), (5e-7, 0.0, -1.0), (5e-7, 2.0, 2.0), (2.0, -1.0, 2.0)]):
        y = 1.0 + 4.5 * n                                              # one, two, three vertices at cz <= 1e-6: not drawn
        b.face(b.pts([(1.5, y), (10.5, y + 0.5), (5.5, y + 4.0)], list(cz)), "behind")
    b.face(b.pts([(16.4, -1e7), (1e7, 9e6), (16.9, 1e7)], [1e-3, 2e-3, 1.5e-3]), "huge_near")      # projections ~1e7 samples
    b.face(b.pts([(20.2, -3e6), (8e6, 1e3), (21.3, 5e6)], [1.1e-3, 0.9e-3, 1e-3]), "huge_near")
    b.tri([(22.5, 3.5), (27.5, 4.5), (24.5, 9.5)], 2.0, "hidden")      # behind the near faces
    return b.case()


def _nonfinite(with_bad):
    b = _Builder()
    b.quad(1.5, 1.5, 20.5, 20.5, 5.0, "wall")
    b.tri([(3.2, 3.1), (12.7, 4.4), (6.1, 11.9)], 3.0, "front")
    if with_bad:
        n0 = len(b.v)
        b.v += [(float("nan"), 0.0, 1.0), (0.0, float("inf"), 2.0), (0.0, 0.0, float("-inf"))]         # referenced by no face
        bad = [(float("nan"), 0.1, 3.0), (float("inf"), 0.1, 3.0), (float("-inf"), 0.2, 3.0), (0.1, float("nan"), 3.0),
               (0.1, 0.1, float("inf")), (0.1, float("-inf"), 3.0), (0.1, 0.1, float("nan"))]
        for k, p in enumerate(bad):
            i = b.pts([(22.0 + k, 4.2), (28.3, 17.6 - k)], 2.0)             # beside the wall: nothing else is hit there
            b.v.append(p)
            b.face((i[0], len(b.v) - 1, i[1]) if k % 2 else (len(b.v) - 1, i[0], i[1]), "bad")
        assert len(b.v) - n0 == 3 + 3 * len(bad)
        return b.case(banned=np.asarray(b.tags["bad"]), base="nonfinite-base")
    return b.case()


# ---- the list ---------------------------------------------------------------------------------------------------------

BLOB = [f"blob-48x64x2-c{c}" for c in range(4)] + [f"blob-5x7x3-c{c}" for c in range(4)]
SIZES = ["blob-2x7x3-c0", "blob-5x2x2-c3", "blob-5x7x1-c1", "blob-5x7x5-c2"] + [f"blob-24x32x2-c3-n{n}" for n in (1, 255, 256, 257, 513)]
LATTICE = [f"lattice-t{t}" for t in range(6)] + [f"lattice9-t{t}" for t in range(6)]
GENERIC = BLOB + SIZES + ["closed"]
ADVERSARIAL = LATTICE + ["edges"]
OTHER = ["near", "nonfinite", "nonfinite-base"]
CLEANER = {"blob": [[f"blob-24x32x{up}-c{c}" for c in range(4)] for up in (1, 3)],
           "lattice": [[f"lattice-t{t}-up{up}"] for up in (1, 3) for t in (0, 4)]}
ALL = GENERIC + ADVERSARIAL + OTHER


@functools.lru_cache(None)
def case(name):
    p = name.split("-")
    if p[0] == "blob":
        h, w, up = (int(s) for s in p[1].split("x"))
        return _blob(h, w, up, int(p[2][1:]), int(p[3][1:]) if len(p) > 3 else None)
    if p[0] in ("lattice", "lattice9"):
        w, up = (8, 3) if p[0] == "lattice" else (9, 2)
        return _lattice(int(p[1][1:]), w, up, int(p[2][2:]) if len(p) > 2 else None)
    return {"closed": _closed, "edges": _edges, "near": _near, "nonfinite": lambda: _nonfinite(True),
            "nonfinite-base": lambda: _nonfinite(False)}[name]()
