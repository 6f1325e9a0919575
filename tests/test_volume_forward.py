"""The forward kernels of the volume build, each fed directly at ragged shapes (csrc/volume.hip, matching.hip and the
site-list kernels of spconv.hip).

Part A (no GPU): a float64 restatement of depth_filtering, back_proj_multiscale and the matching-field depth expectation,
pinned to the fp32 oracle on the golden scene, and the conditions every input set of parts C-E has to meet, evaluated from
that restatement alone.  Parts B-E (gpu): the kernels against NumPy / integer references (exact) and against the float64
restatement.

How a flag is compared (parts C, D).  The float64 reference decides every (voxel, view) term.  A term is UNCERTAIN when one of its
margins - |nx| - 1, |ny| - 1, qz, ||d - qz| - depth_range| - is closer to zero than EPS; a voxel is DECIDED when its certain terms
alone fix `cnt > 1`; flags are compared on decided voxels.  EPS is not chosen: it is 8 x the largest difference between the fp32
oracle's arithmetic and float64 seen on these very inputs (the 8 allows for the kernel's operation order and the device's
division), measured over the terms whose float64 margin is at most 1 - further out no rounding error reaches the threshold, and
near a camera's plane (qz -> 0) the absolute error of nx = x / qz grows without bound while |nx| itself is in the thousands.
A margin of exactly zero (part D's axis-aligned view with dyadic intrinsics: every operation on it is exact in fp32) is certain.

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest):
    part C  largest fp32-vs-float64 margin difference 4.2e-05  ->  EPS_FILTER  = 3.4e-04
    part D  largest fp32-vs-float64 margin difference 4.8e-06  ->  EPS_COSTVOL = 3.9e-05
    part E  largest fp32-vs-float64 clamp-argument difference 1.1e-06  ->  EPS_BAND = 8.8e-06
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import surf_oracle as O

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FINE_HW = (37, 53)
LEVELS_C2F = ((5, 7), (10, 14), (19, 27), (37, 53))          # not halves of one another


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# the float64 restatement (dt = float64) - the same statements at dt = float32 are the oracle's arithmetic
# ------------------------------------------------------------------------------------------------------------------


def _world(coords, D, dt):
    vs = torch.tensor(2.0 / (D - 1), dtype=F64).to(F32)        # float32(2 / (D - 1)), promoted
    return coords.to(dt) * vs.to(dt) + (-1.0)


def _ndc(world, intr, c2w, h, w, dt):
    w2c = torch.inverse(c2w.to(dt))
    hom = torch.cat([world, torch.ones_like(world[:, :1])], dim=1)
    q = (hom @ w2c.t()) @ intr.to(dt).t()
    x = q[:, 0] / q[:, 2]
    y = q[:, 1] / q[:, 2]
    return x / ((w - 1) / 2) - 1, y / ((h - 1) / 2) - 1, q[:, 2]


def _bilinear(img, x, y):
    """img (C,H,W), pixel positions (N,) -> (N,C); zero padding per tap."""
    C, H, W = img.shape
    x0, y0 = torch.floor(x), torch.floor(y)
    tx, ty = x - x0, y - y0
    x0, y0 = x0.long(), y0.long()
    flat = img.reshape(C, H * W)
    out = torch.zeros(x.shape[0], C, dtype=img.dtype)
    for dy, wy in ((0, 1.0 - ty), (1, ty)):
        for dx, wx in ((0, 1.0 - tx), (1, tx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            v = flat[:, yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)].t()
            out = out + torch.where(ok[:, None], v * (wx * wy)[:, None], torch.zeros_like(v))
    return out


def _unnorm_ac(g, size):
    return ((g + 1.0) / 2.0) * (size - 1)


def depth_filtering_ref(depths, coords, D, intrs, c2ws, dt=F64):
    """Per (view, voxel): nx, ny, qz and the bilinear depth d, each (nv, N)."""
    nv, h, w = depths.shape
    world = _world(coords, D, dt)
    rows = []
    for v in range(nv):
        nx, ny, qz = _ndc(world, intrs[v], c2ws[v], h, w, dt)
        d = _bilinear(depths[v][None].to(dt), _unnorm_ac(nx, w), _unnorm_ac(ny, h))[:, 0]
        rows.append(torch.stack([nx, ny, qz, d]))
    return torch.stack(rows, dim=1)                              # (4, nv, N)


def back_proj_ref(agg, feats_c2f, coords, D, intrs, c2ws, stage, dt=F64, ndc=None):
    """-> [mean | var] rows (N,8), the mask inputs (3, nv, N) = nx, ny, qz, and the agg_mlp pre-activations (nv, N, 8).
    ndc: a projection to use in place of _ndc (same signature)."""
    nv = feats_c2f[-1].shape[0]
    h, w = feats_c2f[-1].shape[-2:]
    w1, b1, w2, b2 = (t.to(dt) for t in agg)
    world = _world(coords, D, dt)
    warp, logits, terms, pres = [], [], [], []
    for v in range(nv):
        nx, ny, qz = (ndc or _ndc)(world, intrs[v], c2ws[v], h, w, dt)
        m = (nx.abs() <= 1) & (ny.abs() <= 1) & (qz > 0)
        f = torch.zeros(coords.shape[0], 4, dtype=dt)
        for lvl in feats_c2f[stage:]:
            hh, ww = lvl.shape[-2:]
            f = f + _bilinear(lvl[v].to(dt), _unnorm_ac(nx, ww), _unnorm_ac(ny, hh))
        pre = f @ w1.t() + b1
        a = torch.where(pre > 0, pre, torch.expm1(pre)) @ w2.t() + b2
        logits.append(torch.where(m[:, None], a, torch.full_like(a, -1e9)))
        warp.append(f)
        terms.append(torch.stack([nx, ny, qz]))
        pres.append(pre)
    wf = torch.stack(warp) * torch.softmax(torch.stack(logits), dim=0)   # no view sees the voxel: all -1e9 = uniform
    mean = wf.sum(0)
    return torch.cat([mean, (wf ** 2).sum(0) - mean ** 2], dim=1), torch.stack(terms, dim=1), torch.stack(pres)


def _trilinear(vol, g):
    D = vol.shape[0]
    g0 = torch.floor(g)
    t = g - g0
    g0 = g0.long()
    flat = vol.reshape(-1)
    out = torch.zeros(g.shape[0], dtype=vol.dtype)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = g0 + torch.tensor([dx, dy, dz])
                ok = ((c >= 0) & (c < D)).all(dim=1)
                c = c.clamp(0, D - 1)
                wgt = ((t[:, 0] if dx else 1.0 - t[:, 0]) * (t[:, 1] if dy else 1.0 - t[:, 1]) * (t[:, 2] if dz else 1.0 - t[:, 2]))
                out = out + torch.where(ok, flat[(c[:, 0] * D + c[:, 1]) * D + c[:, 2]] * wgt, torch.zeros_like(wgt))
    return out


def matching_ref(mvol, intrs, c2ws, near_fars, H, W, res_level, n, pre=None, ratio_cur=1.0, ratio_prev=1.0, dt=F64, jitter=None):
    """The matching field's expected depth: low-resolution maps (nv,h,w), full-resolution maps (nv,H,W) and, with `pre`, the four
    arguments the band construction compares with zero, (nv, h*w, 4) = b - far and a - near of the two bands.
    jitter (nv, h*w, 2): the train-mode shift per ray and band, z += jitter * (band's range) / n."""
    h, w = H // res_level, W // res_level
    py, px = torch.meshgrid(torch.linspace(0, H - 1, h), torch.linspace(0, W - 1, w), indexing="ij")   # fp32 positions: inputs
    px, py = px.reshape(-1), py.reshape(-1)
    lin = torch.linspace(0.0, 1.0, int(n), dtype=F32).to(dt)
    vol = mvol.to(dt)
    Dv = vol.shape[0]
    lrs, args = [], []
    for v in range(intrs.shape[0]):
        pix = torch.stack([px, py, torch.ones_like(px)], dim=-1).to(dt)
        camd = pix @ torch.inverse(intrs.to(dt))[v, :3, :3].t()
        R = c2ws[v, :3, :3].to(dt)
        rd = (camd / torch.linalg.norm(camd, dim=-1, keepdim=True)) @ R.t()
        ro = c2ws[v, :3, 3].to(dt)
        n0, f0 = near_fars[v, 0].to(dt), near_fars[v, 1].to(dt)
        cz = (rd @ torch.inverse(R).t())[:, 2]
        if pre is None:
            z = n0 + (f0 - n0) * lin[None, :].expand(px.shape[0], -1)
            if jitter is not None:
                z = z + jitter[v, :, 0:1].to(dt) * (f0 - n0) / n
        else:
            zc = (pre[v].to(dt)[py.long(), px.long()] / cz)[:, None]
            zs, arg = [], []
            for k, r in enumerate((ratio_cur, ratio_prev)):
                half = ((f0 - n0) * r) / 2
                a, b = zc - half, zc + half
                arg.append(b - f0)
                a = torch.where(b > f0, a - (b - f0), a)
                arg.append(a - n0)
                b = torch.where(a < n0, b + (n0 - a), b)
                a, b = torch.clamp(a, n0, f0), torch.clamp(b, n0, f0)
                zs.append(a + (b - a) * lin[None, :] + (0.0 if jitter is None else jitter[v, :, k:k + 1].to(dt) * (b - a) / n))
            z = torch.cat(zs, dim=-1)
            args.append(torch.cat(arg, dim=-1))
        pts = (ro[None, None, :] + rd[:, None, :] * z[..., None]).reshape(-1, 3)
        rho = _trilinear(vol, ((pts + 1.0) * Dv - 1.0) / 2.0).reshape(z.shape)
        lrs.append(((z * torch.softmax(rho, dim=-1)).sum(dim=1) * cz).reshape(h, w))
    lr = torch.stack(lrs)
    full = F.interpolate(lr[:, None], size=(H, W), mode="bilinear")[:, 0]
    return lr, full, (torch.stack(args) if args else None)


# ------------------------------------------------------------------------------------------------------------------
# margins, decisions, EPS
# ------------------------------------------------------------------------------------------------------------------


def margins(terms, depth_range=None):
    """(K, nv, N): negative = the term's condition holds.  K = 3 (frustum) or 4 (with the depth band)."""
    g = [terms[0].abs() - 1, terms[1].abs() - 1, -terms[2]]
    if depth_range is not None:
        g.append((terms[3] - terms[2]).abs() - depth_range)
    return torch.stack(g)


def holds(terms, depth_range=None):
    ok = (terms[0].abs() <= 1) & (terms[1].abs() <= 1) & (terms[2] > 0)
    if depth_range is not None:
        ok = ok & ((terms[3] - terms[2]).abs() < depth_range)
    return ok


def margin_difference(t32, t64, depth_range=None):
    """Largest fp32-vs-float64 difference of a margin, over the terms whose float64 margin is at most 1 (module docstring)."""
    g32, g64 = margins(t32.to(F64), depth_range), margins(t64, depth_range)
    near = g64.abs() <= 1
    return float((g32 - g64).abs()[near].max()) if bool(near.any()) else 0.0


def decide(terms, eps, depth_range=None, exact_zero_is_certain=False):
    """-> (flag, decided, has an uncertain term), each (N,) bool, from the float64 terms alone."""
    g = margins(terms, depth_range)
    unc = g.abs() < eps
    if exact_zero_is_certain:
        unc = unc & (g != 0)
    unc = unc.any(dim=0)
    ok = holds(terms, depth_range)
    lo = (ok & ~unc).sum(0)
    hi = lo + unc.sum(0)
    return lo > 1, (lo > 1) | (hi <= 1), unc.any(dim=0)


# ------------------------------------------------------------------------------------------------------------------
# inputs: cameras in float64, rounded to fp32 once
# ------------------------------------------------------------------------------------------------------------------


def _look_at(pos, target):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, pos
    return c2w


def _intr(f, H, W):
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    return K


INSIDE_POS = (0.15, -0.1, -0.83)                                 # inside the unit cube: the voxels with z < -0.83 lie behind it


def make_cameras(nv, H, W, exact_first=False, per_axis_focal=False):
    """Ring cameras around the origin with a focal length that leaves the cube's corners outside the image, one camera INSIDE the
    unit cube (second ring slot), and - exact_first - an axis-aligned first view whose matrices are dyadic: the voxels (+-1, y, 0)
    of an odd lattice project to |nx| = 1 exactly.  per_axis_focal: the vertical focal length scaled by (H - 1) / (W - 1), for images
    far from square (the same share of the cube in view along both axes).  -> intrs, c2ws (nv,4,4) fp32, near_fars (nv,2) fp32."""
    c2ws, intrs = [], []
    if exact_first:
        c = np.eye(4)
        c[2, 3] = -2.0
        c2ws.append(c)
        intrs.append(_intr(float(W - 1), H, W))
    k = 0
    while len(c2ws) < nv:
        if k == 1:
            c2ws.append(_look_at(INSIDE_POS, (0.05, 0.13, 1.0)))
            intrs.append(_intr(0.45 * (W - 1), H, W))
        else:
            ang = 0.3 + 2.0 * np.pi * k / 7.0
            c2ws.append(_look_at((2.2 * np.cos(ang), 0.5 * np.sin(1.7 * k + 0.4), 2.2 * np.sin(ang)), (0.03 * k, -0.02 * k, 0.0)))
            intrs.append(_intr(0.77 * (W - 1), H, W))
        k += 1
    if per_axis_focal:
        for K in intrs:
            K[1, 1] *= (H - 1) / (W - 1)
    c2ws = torch.from_numpy(np.stack(c2ws)).to(F32)
    dist = c2ws[:, :3, 3].norm(dim=1)
    near_fars = torch.stack([(dist - 1.0).clamp(min=0.2), dist + 1.0], dim=1)
    return torch.from_numpy(np.stack(intrs)).to(F32), c2ws, near_fars


def sphere_depths(intrs, c2ws, H, W, radius=0.6):
    """The analytic depth (camera z) of a sphere about the origin from each camera - the plane through the origin where the ray
    misses it - plus a smooth perturbation; float64, rounded to fp32 once."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    out = []
    for v in range(intrs.shape[0]):
        K, c = intrs[v].to(F64), c2ws[v].to(F64)
        dc = torch.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], torch.ones_like(xs)], dim=-1)
        dw = dc @ c[:3, :3].t()
        o = c[:3, 3]
        a, b, cc = (dw * dw).sum(-1), (dw * o).sum(-1), float(o @ o) - radius * radius
        disc = b * b - a * cc
        sq = torch.sqrt(disc.clamp(min=0))
        s = torch.where((-b - sq) > 0, (-b - sq) / a, (-b + sq) / a)
        plane = -(o @ c[:3, 2]) / (dw @ c[:3, 2])             # camera z of the plane through the origin, normal = the optical axis
        s = torch.where((disc > 0) & (s > 0), s, plane)
        out.append(s + 0.03 * torch.sin(0.31 * xs + v) * torch.cos(0.23 * ys - v))
    return torch.stack(out).to(F32)


def random_parents(n, Dp, seed):
    """n parents on the Dp^3 lattice (repeats where n exceeds it), the first ones on the lattice faces."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, Dp, (n, 3), generator=g)
    k = min(n // 3, 12)
    if k:
        face = torch.randint(0, 3, (k,), generator=g)
        p[torch.arange(k), face] = torch.where(torch.rand(k, generator=g) < 0.5, 0, Dp - 1)
    return p.to(torch.int32)


# ---- part C ------------------------------------------------------------------------------------------------------
#              nv  (H, W)    D   n_parents  depth_range
FILTER_CASES = ((1, (37, 53), 34, 1000, 0.45),
                (2, (37, 53), 34, 1000, 1.00),
                (3, (37, 53), 34, 33, 0.45),
                (8, (37, 53), 34, 1000, 0.25),
                (2, (2, 3), 6, 33, 0.90),
                (8, (2, 3), 4, 1, 0.60),
                (3, (37, 53), 6, 1, 0.45),
                (8, (2, 3), 34, 1000, 0.45),
                (2, (37, 53), 4, 33, 1.00))


@functools.lru_cache(maxsize=None)
def filter_case(i):
    nv, (H, W), D, n_par, rng = FILTER_CASES[i]
    intrs, c2ws, _ = make_cameras(nv, H, W)
    depths = sphere_depths(intrs, c2ws, H, W)
    parents = random_parents(n_par, D // 2, 40 + i)
    if n_par == 1:
        parents = torch.tensor([[D // 4, D // 4, D // 4 - (1 if D == 4 else 0)]], dtype=torch.int32).clamp(min=0)
    children = (parents.long() * 2)[:, None, :] + torch.tensor(O.CHILD_OFFSETS)[None]
    children = children.reshape(-1, 3)
    t64 = depth_filtering_ref(depths, children, D, intrs, c2ws, F64)
    t32 = depth_filtering_ref(depths, children, D, intrs, c2ws, F32)
    return dict(nv=nv, H=H, W=W, D=D, range=rng, intrs=intrs, c2ws=c2ws, depths=depths, parents=parents, children=children,
                t64=t64, t32=t32)


@functools.lru_cache(maxsize=None)
def eps_filter():
    return 8.0 * max(margin_difference(filter_case(i)["t32"], filter_case(i)["t64"], FILTER_CASES[i][4])
                     for i in range(len(FILTER_CASES)))


# ---- part D ------------------------------------------------------------------------------------------------------
#               D   n_parents (None: full lattice)  stage  nv
COSTVOL_CASES = ((2, None, 0, 1),
                 (3, None, 1, 2),
                 (5, None, 2, 5),
                 (9, None, 3, 8),
                 (9, None, 0, 2),
                 (4, 1, 3, 2),
                 (6, 33, 1, 5),
                 (34, 1000, 0, 8),
                 (34, 1000, 2, 1),
                 (34, 1000, 1, 2))


def make_agg(seed, dt=F32):
    """dt = float64: drawn in float64 and rounded to fp32 once (the same bits on every host)."""
    g = torch.Generator().manual_seed(seed)
    return tuple(t.to(F32) for t in (torch.randn(8, 4, generator=g, dtype=dt) * 0.7, torch.randn(8, generator=g, dtype=dt) * 0.5,
                                     torch.randn(1, 8, generator=g, dtype=dt) * 0.7, torch.randn(1, generator=g, dtype=dt) * 0.3))


def agg_state_dict(agg):
    return {"volume.agg_mlp.0.weight": agg[0], "volume.agg_mlp.0.bias": agg[1], "volume.agg_mlp.2.weight": agg[2],
            "volume.agg_mlp.2.bias": agg[3]}


def make_pyramid(nv, seed, levels=LEVELS_C2F, dt=F32):
    """Four levels (nv,4,h,w) coarse -> fine whose contents differ per level: a smooth field of its own plus its own offset.
    dt = float64: computed in float64 and rounded to fp32 once (the same bits on every host)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for l, (h, w) in enumerate(levels):
        ys, xs = torch.meshgrid(torch.linspace(0, 1, h, dtype=dt), torch.linspace(0, 1, w, dtype=dt), indexing="ij")
        ph = torch.rand(nv, 4, 1, 1, generator=g, dtype=dt) * 6.28
        smooth = torch.sin((3.0 + l) * xs[None, None] + ph) * torch.cos((2.0 + 1.5 * l) * ys[None, None] - ph)
        out.append((0.6 * smooth + 0.15 * torch.randn(nv, 4, h, w, generator=g, dtype=dt) + 0.25 * (l - 1.5)).to(F32).contiguous())
    return out


@functools.lru_cache(maxsize=None)
def costvol_case(i):
    D, n_par, stage, nv = COSTVOL_CASES[i]
    H, W = FINE_HW
    intrs, c2ws, _ = make_cameras(nv, H, W, exact_first=True)
    feats = make_pyramid(nv, 70 + i)
    agg = make_agg(90 + i)
    if n_par is None:
        parents = idx = None
        coords = O.init_coords(D).long()
    else:
        parents = random_parents(n_par, D // 2, 60 + i)
        g = torch.Generator().manual_seed(80 + i)
        idx = torch.nonzero(torch.rand(8 * n_par, generator=g) < 0.6).view(-1).to(torch.int32)
        if idx.numel() == 0:
            idx = torch.tensor([5], dtype=torch.int32)
        coords = 2 * parents.long()[idx.long() >> 3] + torch.tensor(O.CHILD_OFFSETS)[idx.long() & 7]
    feat64, t64, pre64 = back_proj_ref(agg, feats, coords, D, intrs, c2ws, stage, F64)
    _, t32, _ = back_proj_ref(agg, feats, coords, D, intrs, c2ws, stage, F32)
    feat32, keep32 = O.back_proj_multiscale(agg_state_dict(agg), feats, coords.float(), D, intrs, c2ws, stage)   # the fp32 oracle itself
    return dict(D=D, stage=stage, nv=nv, intrs=intrs, c2ws=c2ws, feats=feats, agg=agg, parents=parents, idx=idx, coords=coords,
                feat64=feat64, t64=t64, t32=t32, pre64=pre64, feat32=feat32, keep32=keep32)


@functools.lru_cache(maxsize=None)
def eps_costvol():
    return 8.0 * max(margin_difference(costvol_case(i)["t32"], costvol_case(i)["t64"]) for i in range(len(COSTVOL_CASES)))


# ---- part E ------------------------------------------------------------------------------------------------------
#                D  (H, W)   res_level nv  n    pre    (ratio_cur, ratio_prev)
MATCH_CASES = ((8, (37, 53), 1, 1, 16, False, (1.0, 1.0)),
               (12, (37, 53), 2, 2, 33, True, (0.4, 0.7)),
               (8, (37, 53), 4, 8, 128, True, (0.1, 0.4)),
               (12, (16, 24), 4, 2, 16, True, (0.1, 0.4)),
               (8, (16, 24), 1, 8, 33, False, (1.0, 1.0)),
               (12, (16, 24), 2, 1, 128, False, (1.0, 1.0)),
               (8, (16, 24), 1, 2, 128, True, (0.4, 0.7)))


def smooth_volume(D):
    r = torch.linspace(-1, 1, D, dtype=F64)
    x, y, z = torch.meshgrid(r, r, r, indexing="ij")
    rad = torch.sqrt(x * x + y * y + z * z)
    return (6.0 * torch.exp(-((rad - 0.55) / 0.3) ** 2) + 0.8 * torch.sin(2.5 * x + 0.4) * torch.cos(1.7 * y - z)).to(F32).contiguous()


@functools.lru_cache(maxsize=None)
def match_case(i):
    D, (H, W), L, nv, n, with_pre, (rc, rp) = MATCH_CASES[i]
    intrs, c2ws, near_fars = make_cameras(nv, H, W)
    mvol = smooth_volume(D)
    pre = None
    if with_pre:                                                   # depths that push the bands against near AND far in places
        ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
        mid = near_fars.to(F64).mean(dim=1)[:, None, None]
        pre = (mid + 1.05 * torch.sin(0.21 * xs[None] + torch.arange(nv)[:, None, None]) * torch.cos(0.17 * ys[None])).to(F32).contiguous()
    kw = dict(pre=pre, ratio_cur=rc, ratio_prev=rp)
    lr64, full64, arg64 = matching_ref(mvol, intrs, c2ws, near_fars, H, W, L, n, dt=F64, **kw)
    _, _, arg32 = matching_ref(mvol, intrs, c2ws, near_fars, H, W, L, n, dt=F32, **kw)
    # the fp32 oracle itself: full maps through matching_field, low-resolution ones through matching_field_pixels
    h, w = H // L, W // L
    py, px = torch.meshgrid(torch.linspace(0, H - 1, h), torch.linspace(0, W - 1, w), indexing="ij")
    stage, ratios, ns, ls = (1, [rp, rc], [0, n], [0, L]) if with_pre else (0, [rc], [n], [L])
    full32 = torch.stack(O.matching_field((H, W), intrs, c2ws, near_fars, mvol, stage, ratios, ns, ls, pre_depths=pre))
    lr32 = torch.stack([O.matching_field_pixels(px.reshape(-1), py.reshape(-1), v, intrs, c2ws, near_fars, mvol, stage, ratios, ns,
                                                None if pre is None else pre[v]).reshape(h, w) for v in range(nv)])
    return dict(D=D, H=H, W=W, L=L, nv=nv, n=n, pre=pre, rc=rc, rp=rp, intrs=intrs, c2ws=c2ws, near_fars=near_fars, mvol=mvol,
                lr64=lr64, full64=full64, arg64=arg64, arg32=arg32, lr32=lr32, full32=full32)


@functools.lru_cache(maxsize=None)
def eps_band():
    return 8.0 * max(float((match_case(i)["arg32"].to(F64) - match_case(i)["arg64"]).abs().max())
                     for i in range(len(MATCH_CASES)) if MATCH_CASES[i][5])


def band_included(c):
    """Pixels that stay in the comparison: (lr mask (nv,h,w), full mask (nv,H,W)).  A full-resolution pixel is left out when one
    of the low-resolution pixels it interpolates is."""
    h, w = c["H"] // c["L"], c["W"] // c["L"]
    if c["arg64"] is None:
        return torch.ones(c["nv"], h, w, dtype=torch.bool), torch.ones(c["nv"], c["H"], c["W"], dtype=torch.bool)
    out = (c["arg64"].abs() < eps_band()).any(dim=-1).reshape(c["nv"], h, w)
    spread = F.interpolate(out[:, None].to(F64), size=(c["H"], c["W"]), mode="bilinear")[:, 0]
    return ~out, spread == 0


# ------------------------------------------------------------------------------------------------------------------
# A. the references and the input sets, on the CPU
# ------------------------------------------------------------------------------------------------------------------


def test_reference_depth_filtering_matches_oracle(scene, golden_pipe):
    """Stage 1 of the golden scene: the fp32 statements ARE the oracle's (same keep, bit for bit), and the float64 ones decide
    every voxel the oracle's own rounding cannot move the same way."""
    D = 16
    parents = golden_pipe["s0_coords"].float()
    children, _ = O.up_sample(parents, torch.zeros(parents.shape[0], 1))
    depths = golden_pipe["s0_depths"]
    rng = float((scene["far"] - scene["near"]).squeeze()) * 0.4
    keep = O.depth_filtering(list(depths), children, D, scene["intrs"], scene["c2ws"], rng)
    t32 = depth_filtering_ref(depths, children.long(), D, scene["intrs"], scene["c2ws"], F32)
    t64 = depth_filtering_ref(depths, children.long(), D, scene["intrs"], scene["c2ws"], F64)
    assert torch.equal(holds(t32, rng).sum(0) > 1, keep)
    eps = 8.0 * margin_difference(t32, t64, rng)
    assert 0 < eps < 1e-3, eps
    flag, decided, _ = decide(t64, eps, rng)
    assert float(decided.double().mean()) > 0.99
    assert torch.equal(flag[decided], keep[decided])
    assert 0.05 < float(keep.double().mean()) < 0.95


def test_reference_back_proj_matches_oracle(scene, weights, golden_fpn, golden_pipe):
    """Stage 1 of the golden scene against O.back_proj_multiscale.  Its own fp32 error: ~100 roundings of values of order 1
    (1e-5) plus the bilinear position error, W/2 * 1e-6 pixels against a feature slope of order 1 per pixel (3e-5): 1e-4 of the
    tensor's scale bounds it with room, and a wrong level, normalisation or softmax is off by 1e-2 and more."""
    D, stage = 16, 1
    coords = golden_pipe["s1_filt_coords"].long()
    feats = [golden_fpn[f"out{i}"] for i in range(4)]
    agg = tuple(weights[f"volume.agg_mlp.{k}"] for k in ("0.weight", "0.bias", "2.weight", "2.bias"))
    ref32, keep32 = O.back_proj_multiscale(weights, feats, coords.float(), D, scene["intrs"], scene["c2ws"], stage)
    feat64, t64, _ = back_proj_ref(agg, feats, coords, D, scene["intrs"], scene["c2ws"], stage, F64)
    _, t32, _ = back_proj_ref(agg, feats, coords, D, scene["intrs"], scene["c2ws"], stage, F32)
    assert torch.equal(holds(t32).sum(0) > 1, keep32)
    eps = 8.0 * margin_difference(t32, t64)
    flag, decided, unc = decide(t64, eps)
    assert torch.equal(flag[decided], keep32[decided]) and float(decided.double().mean()) > 0.99
    sure = ~unc
    err = float((ref32.double() - feat64)[sure].abs().max())
    assert err <= 1e-4 * max(1.0, float(feat64.abs().max())), err
    assert float(feat64[:, 4:].abs().max()) > 1e-3                    # the variance half is not trivially zero


def test_reference_matching_depth_matches_oracle(scene, golden_pipe):
    """Stages 0 (one band) and 1 (two bands about the previous depths) of the golden scene against O.matching_field.  The
    expectation is a smooth function of every input (the band construction is continuous), depths are of order 1: 1e-4 absolute
    is far above the oracle's rounding and far below what a wrong band, sample count or volume lookup does."""
    from tests.golden_cfg import CFG
    H, W = scene["imgs"].shape[-2:]
    pre = None
    for s in (0, 1):
        mvol = golden_pipe[f"s{s}_mvol"]
        ref = torch.stack(O.matching_field((H, W), scene["intrs"], scene["c2ws"], scene["near_fars"], mvol, s, CFG["range_ratios"],
                                           CFG["n_samples_depths"], CFG["depth_res_levels"], pre_depths=pre))
        _, full, _ = matching_ref(mvol, scene["intrs"], scene["c2ws"], scene["near_fars"], H, W, CFG["depth_res_levels"][s],
                                  CFG["n_samples_depths"][s], pre, CFG["range_ratios"][s], CFG["range_ratios"][s - 1] if s else 1.0)
        assert float((ref.double() - full).abs().max()) < 1e-4
        assert float(full.std()) > 1e-2
        pre = golden_pipe[f"s{s}_depths"]


def test_filter_inputs_meet_their_conditions():
    eps = eps_filter()
    behind = outside = 0
    for i, (nv, hw, D, n_par, rng) in enumerate(FILTER_CASES):
        c = filter_case(i)
        assert bool(torch.isfinite(c["t64"]).all()) and bool(torch.isfinite(c["t32"]).all())
        flag, decided, _ = decide(c["t64"], eps, rng)
        assert float((~decided).double().mean()) <= 0.01, (i, float((~decided).double().mean()))
        p = c["parents"]
        if n_par >= 33:
            assert bool(((p == 0) | (p == D // 2 - 1)).any()), i       # parents on the lattice faces
        if nv == 1:
            assert not bool(flag.any()) and bool(decided.all())
        else:
            share = float(flag[decided].double().mean())
            assert 0.1 <= share <= 0.9, (i, share)
        nb = int((c["t64"][2] < -eps).any(0).sum())
        no = int(((c["t64"][0].abs() > 1 + eps) | (c["t64"][1].abs() > 1 + eps)).all(0).sum())
        if nv >= 2 and n_par >= 33:
            assert nb > 0, i                                           # the camera inside the cube is the second view
        if nv <= 2 and n_par == 1000:
            assert no > 0, i
        behind, outside = behind + nb, outside + no
    assert behind > 0 and outside > 0
    assert {c[0] for c in FILTER_CASES} == {1, 2, 3, 8} and {c[1] for c in FILTER_CASES} == {(37, 53), (2, 3)}
    assert {c[2] for c in FILTER_CASES} == {4, 6, 34} and {c[3] for c in FILTER_CASES} == {1, 33, 1000}


def test_costvol_inputs_meet_their_conditions():
    eps = eps_costvol()
    unseen = exact = 0
    for i, (D, n_par, stage, nv) in enumerate(COSTVOL_CASES):
        c = costvol_case(i)
        assert bool(torch.isfinite(c["t64"]).all()) and bool(torch.isfinite(c["feat64"]).all()) and bool(torch.isfinite(c["feat32"]).all())
        flag, decided, unc = decide(c["t64"], eps, exact_zero_is_certain=True)
        assert float((~decided).double().mean()) <= 0.01, i
        assert float(unc.double().mean()) <= 0.01, i                 # rows left out of the feature comparison
        if nv == 1:
            assert not bool(flag.any())
        pre = c["pre64"]
        assert float((pre > 0.05).double().mean()) > 0.1 and float((pre < -0.05).double().mean()) > 0.1, i   # both sides of the ELU knee
        unseen += int((~holds(c["t64"]).any(0) & ~unc).sum())
        g = margins(c["t64"])
        on_edge = ((g[0] == 0) | (g[1] == 0)) & holds(c["t64"])
        if nv >= 2:
            exact += int(on_edge.any(0).sum())
            # ... and fp32 agrees that they are ON the edge: the view's arithmetic is exact
            assert torch.equal(margins(c["t32"].to(F64))[:2][:, on_edge] == 0, g[:2][:, on_edge] == 0)
        # per-level contents differ: dropping a level or starting the loop elsewhere moves the features
        if stage > 0:
            other, _, _ = back_proj_ref(c["agg"], c["feats"], c["coords"], D, c["intrs"], c["c2ws"], stage - 1, F64)
            assert float((other - c["feat64"]).abs().max()) > 0.05, i
    assert unseen > 0 and exact > 0
    assert {c[0] for c in COSTVOL_CASES if c[1] is None} == {2, 3, 5, 9} and {c[0] for c in COSTVOL_CASES if c[1]} == {4, 6, 34}
    assert {c[2] for c in COSTVOL_CASES} == {0, 1, 2, 3} and {c[3] for c in COSTVOL_CASES} == {1, 2, 5, 8}


def test_matching_inputs_meet_their_conditions():
    clamped_far = clamped_near = 0
    for i, (D, (H, W), L, nv, n, with_pre, _) in enumerate(MATCH_CASES):
        c = match_case(i)
        assert bool(torch.isfinite(c["lr64"]).all()) and float(c["lr64"].std()) > 1e-2
        lr_ok, full_ok = band_included(c)
        assert float((~lr_ok).double().mean()) <= 0.01 and float((~full_ok).double().mean()) <= 0.01, i
        if with_pre:
            clamped_far += int((c["arg64"][..., 0] > eps_band()).sum())
            clamped_near += int((c["arg64"][..., 1] < -eps_band()).sum())
    assert clamped_far > 0 and clamped_near > 0                        # both shifts of the band construction are exercised
    assert any(H % L or W % L for _, (H, W), L, *_ in MATCH_CASES)
    assert {c[0] for c in MATCH_CASES} == {8, 12} and {c[2] for c in MATCH_CASES} == {1, 2, 4}
    assert {c[3] for c in MATCH_CASES} == {1, 2, 8} and {c[4] for c in MATCH_CASES} == {16, 33, 128}


def _recorded(label):
    import re
    m = re.search(label + r"\s*=\s*([0-9.e+-]+)", __doc__)
    return float(m.group(1))


def test_measured_margins_are_recorded():
    """The EPS values of the module docstring are the ones these inputs give (same arithmetic on any x86 host, 10 % of slack for
    another BLAS' summation order)."""
    for label, fn in (("EPS_FILTER", eps_filter), ("EPS_COSTVOL", eps_costvol), ("EPS_BAND", eps_band)):
        assert abs(fn() / _recorded(label) - 1.0) < 0.1, (label, fn())


# ------------------------------------------------------------------------------------------------------------------
# B. exact kernels
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097, 8191, 4_194_305])
def test_compact_offsets_values_densities(n):
    """Flag arrays that start 0, 1, 3, 15, 17 bytes into an allocation (all but the first take the byte-wise path everywhere), flag
    bytes from {0, 1, 2, 255}, densities 0, 1 and 0.3: the list is nonzero(), the device count of compact_counted its length."""
    from surf_amd import ops
    d = dev()
    rs = np.random.RandomState(n % 9973)
    vals = np.array([1, 2, 255], np.uint8)
    for p in (0.0, 1.0, 0.3):
        flags = np.where(rs.rand(n) < p, vals[rs.randint(0, 3, n)], 0).astype(np.uint8)
        ref = torch.from_numpy(np.flatnonzero(flags))
        for k in (0, 1, 3, 15, 17):
            buf = torch.zeros(k + n, dtype=torch.uint8)
            buf[k:] = torch.from_numpy(flags)
            view = buf.to(d)[k:]
            assert view.data_ptr() % 16 == k % 16 and view.is_contiguous()
            idx = ops.compact(view)
            assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), ref), (n, p, k)
            idx2, count = ops.compact_counted(view)
            assert int(count.item()) == ref.numel() and torch.equal(idx2[:ref.numel()].cpu().long(), ref), (n, p, k)


@gpu
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.int32])
def test_gather_rows_bit_exact_and_confined(src_dtype):
    from surf_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(11)
    sentinel = 0x5ca1ab1e
    for w in (1, 3, 8, 16):
        for shift in (0, 3):
            for n in (1, 255, 256, 257):
                rows = 37
                bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, w), generator=g, dtype=torch.int64).to(torch.int32)
                idx = torch.randint(0, rows << shift, (n,), generator=g, dtype=torch.int64).to(torch.int32)
                if n > 2:
                    idx[1] = idx[0]                                   # repeated indices
                    idx[n // 2] = idx[n - 1]
                src = bits.view(src_dtype).to(d).contiguous()
                # packed result
                out = ops.gather_rows(src, idx.to(d), shift=shift)
                assert out.dtype == src_dtype and torch.equal(out.cpu().view(torch.int32), bits[(idx >> shift).long()])
                # into columns off .. off + w of a wider, pre-filled destination
                for off, stride in ((3, w + 5), (1, w + 1)):
                    dst = torch.full((n, stride), sentinel, dtype=torch.int32).view(src_dtype).to(d)
                    ops.gather_rows(src, idx.to(d), shift=shift, dst=dst, dst_off=off)
                    got = dst.cpu().view(torch.int32)
                    assert torch.equal(got[:, off:off + w], bits[(idx >> shift).long()]), (w, shift, n, off)
                    rest = torch.cat([got[:, :off], got[:, off + w:]], dim=1)
                    assert bool((rest == sentinel).all()), (w, shift, n, off)


@gpu
def test_compose_index():
    from surf_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(12)
    for n in (1, 255, 256, 257, 100_003):
        a = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 7,), generator=g, dtype=torch.int64).to(torch.int32)
        b = torch.randint(0, n + 7, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        assert torch.equal(ops.compose_index(a.to(d), b.to(d)).cpu(), a[b.long()])


def _occupancies(D, g):
    full = O.init_coords(D).long()
    corners = full[((full == 0) | (full == D - 1)).all(dim=1)]
    yield "one", full[torch.randint(0, full.shape[0], (1,), generator=g)]
    yield "one-odd", torch.tensor([[1, 1, 1]])                         # a bounding box that holds no even site
    yield "corners", corners
    yield "sparse", full[torch.rand(full.shape[0], generator=g) < 0.2]
    yield "full", full


@gpu
@pytest.mark.parametrize("D", [2, 3, 4, 5, 9, 16, 33])
def test_site_lists_match_oracle(D):
    """table_from_coords against O.get_index and down_sites (compose of coords_bbox, mark_down_sites, compact, sites_from_keys)
    against O.down_coords for the three rules; 'pad0' as the U-Net calls it - coordinates stored + 1 on the (D + 1) lattice and
    q_max = the true output lattice size, which is 0 (nothing survives) below D = 3."""
    from surf_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(200 + D)
    empties = 0
    for name, occ in _occupancies(D, g):
        if occ.shape[0] == 0:
            continue
        coords = occ[torch.randperm(occ.shape[0], generator=g)].contiguous()       # rows in no particular order
        c_dev = coords.to(torch.int32).to(d).contiguous()
        assert torch.equal(ops.table_from_coords(c_dev, D).cpu().long(), O.get_index(coords, D)), name
        for rule in ("dilate", "floor", "pad0"):
            ref, D1 = O.down_coords(coords, D, rule)
            if rule == "pad0":
                q_max = max((D - 3) // 2 + 1, 0)
                assert q_max == (D1 if D >= 3 else 0)
                c2, t2, D2 = ops.down_sites((coords + 1).to(torch.int32).to(d).contiguous(), D + 1, rule, q_max=q_max)
                got = c2.cpu().long() - 1
            else:
                c2, t2, D2 = ops.down_sites(c_dev, D, rule)
                assert D2 == D1
                got = c2.cpu().long()
            assert c2.dtype == torch.int32 and tuple(c2.shape) == (ref.shape[0], 3), (name, rule)
            assert torch.equal(got, ref), (name, rule)
            stored = c2.cpu().long()
            key = (stored[:, 0] * D2 + stored[:, 1]) * D2 + stored[:, 2]
            assert bool((key[1:] > key[:-1]).all()), (name, rule)        # ascending key order
            t_ref = torch.full((D2 * D2 * D2,), -1, dtype=torch.int64)
            t_ref[key] = torch.arange(key.shape[0])
            assert tuple(t2.shape) == (D2, D2, D2) and torch.equal(t2.cpu().long().view(-1), t_ref), (name, rule)
            empties += ref.shape[0] == 0
    if D == 2:
        assert empties >= 2                  # 'dilate' on the lone odd voxel, 'pad0' on a lattice too small for a window


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, 100_003])
def test_row_linear8_within_fma_bound(n):
    """Eight fp32 FMAs per output: |err| <= 8 * 2^-24 * sum_c |x_c w_c|."""
    from surf_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(13 + n)
    x = torch.randn(n, 8, generator=g) * torch.exp(torch.randn(n, 1, generator=g))
    wgt = torch.randn(8, 8, generator=g)
    out = ops.row_linear8(x.to(d).contiguous(), wgt.to(d).contiguous()).cpu().double()
    ref = x.double() @ wgt.double().t()
    bound = 8.0 * 2.0 ** -24 * (x.double().abs() @ wgt.double().abs().t())
    assert bool(((out - ref).abs() <= bound).all()), float(((out - ref).abs() / bound).max())
    assert float(ref.abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------------------------
# C. upsample_filter
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("i", range(len(FILTER_CASES)))
def test_upsample_filter_flags(i):
    """Flags equal the float64 decision on every decided voxel (module docstring: largest fp32-vs-float64 margin difference
    4.2e-05, EPS_FILTER = 3.4e-04; at most 1 % of a case is undecided, test_filter_inputs_meet_their_conditions)."""
    from surf_amd import ops
    d = dev()
    c = filter_case(i)
    cams = ops.Cameras(c["intrs"], c["c2ws"])
    flags = ops.upsample_filter(c["parents"].to(d).contiguous(), c["D"], c["depths"].to(d).contiguous(), cams, c["range"])
    got = flags.cpu()
    assert got.dtype == torch.uint8 and got.numel() == 8 * c["parents"].shape[0] and bool((got <= 1).all())
    flag, decided, _ = decide(c["t64"], eps_filter(), c["range"])
    wrong = (got.bool() != flag) & decided
    print(f"case {i}: {int(decided.sum())}/{decided.numel()} decided, {int(flag[decided].sum())} set, {int(wrong.sum())} wrong")
    assert not bool(wrong.any()), (i, int(wrong.sum()))


# ------------------------------------------------------------------------------------------------------------------
# D. costvol
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("i", range(len(COSTVOL_CASES)))
def test_costvol_coords_keep_feat(i):
    """coords exact; keep exact on decided voxels (EPS_COSTVOL of the module docstring); feat against float64 on the rows without
    an uncertain frustum term, under BOTH the project's bar for this tensor (rel 1e-3 + abs 2e-5) and 4 x the fp32 CPU oracle's
    own largest error against float64 on the same rows (tensor-wide maxima: the variance channels cancel in both).
    The fp32 oracle's largest error per case is 4.9e-07 ... 6.6e-06 (CPU); the kernel's is printed per case beside it (run with -s)."""
    from surf_amd import ops
    d = dev()
    c = costvol_case(i)
    cams = ops.Cameras(c["intrs"], c["c2ws"])
    feats_t4 = [f.permute(0, 2, 3, 1).contiguous().to(d) for f in c["feats"]]          # texel4: (nv, h, w, 4)
    agg = np.concatenate([t.reshape(-1).numpy() for t in c["agg"]]).astype(np.float32)
    if c["idx"] is None:
        coords, feat, keep = ops.costvol(feats_t4, c["stage"], c["D"], cams, agg)
    else:
        coords, feat, keep = ops.costvol(feats_t4, c["stage"], c["D"], cams, agg, parents=c["parents"].to(d).contiguous(),
                                         idx=c["idx"].to(d).contiguous())
    assert torch.equal(coords.cpu().long(), c["coords"])            # x slowest / 2 parent + CHILD_OFFSETS[idx & 7]
    flag, decided, unc = decide(c["t64"], eps_costvol(), exact_zero_is_certain=True)
    got = keep.cpu()
    assert bool((got <= 1).all()) and torch.equal(got.bool()[decided], flag[decided])
    sure = ~unc
    f = feat.cpu().double()
    err = (f - c["feat64"]).abs()[sure]
    err_oracle = float((c["feat32"].double() - c["feat64"]).abs()[sure].max())
    print(f"case {i}: kernel max err {float(err.max()):.3e}, fp32 oracle max err {err_oracle:.3e}")
    assert bool((err <= 2e-5 + 1e-3 * c["feat64"].abs()[sure]).all()), float(err.max())
    assert float(err.max()) <= 4.0 * err_oracle, (float(err.max()), err_oracle)
    none = ~holds(c["t64"]).any(0) & sure                              # seen by no view: the uniform average over the views
    if bool(none.any()):
        assert float((f - c["feat64"]).abs()[none].max()) <= 4.0 * err_oracle


# ------------------------------------------------------------------------------------------------------------------
# E. matching_depth
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("i", range(len(MATCH_CASES)))
def test_matching_depth_both_resolutions(i):
    """Low- and full-resolution maps against float64 under the project's bar for this tensor (rel 1e-3 + abs 5e-5) and 4 x the
    fp32 CPU oracle's own largest error; pixels whose band arguments lie within EPS_BAND of a clamp are left out (<= 1 %).
    The fp32 oracle's largest error per case is 4.3e-07 ... 9.3e-07 (CPU); the kernel's is printed per case beside it (run with -s)."""
    from surf_amd import ops
    d = dev()
    c = match_case(i)
    cams = ops._cams_ext(ops.Cameras(c["intrs"], c["c2ws"]), c["intrs"], c["c2ws"])
    pre = None if c["pre"] is None else c["pre"].to(d).contiguous()
    full, lr = ops.matching_depth(c["mvol"].to(d).contiguous(), cams, c["near_fars"], c["H"], c["W"], c["L"], c["n"], pre,
                                  c["rc"], c["rp"], return_lr=True)
    assert tuple(lr.shape) == tuple(c["lr64"].shape) and tuple(full.shape) == tuple(c["full64"].shape)
    lr_ok, full_ok = band_included(c)
    for name, got, ref, ora, ok in (("lr", lr, c["lr64"], c["lr32"], lr_ok), ("full", full, c["full64"], c["full32"], full_ok)):
        err = (got.cpu().double() - ref).abs()[ok]
        err_oracle = float((ora.double() - ref).abs()[ok].max())
        print(f"case {i} {name}: kernel max err {float(err.max()):.3e}, fp32 oracle max err {err_oracle:.3e}")
        assert bool((err <= 5e-5 + 1e-3 * ref.abs()[ok]).all()), (name, float(err.max()))
        assert float(err.max()) <= 4.0 * err_oracle, (name, float(err.max()), err_oracle)
