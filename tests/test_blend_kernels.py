"""The blend kernels per element against a float64 restatement, at ragged map sizes, two to eight views and ragged sample counts:
surf_blend (blend.hip, fp32), surf_blend_split / _dn (blend_split.hip: f32lds, bf16x3, f16x2), surf_blend_backward (blend_bwd.hip)
and ops.blend_backward's assembled gradients.  Every kernel is held to float64 independently, never to another kernel.

What is compared.  The whole operation - multi-view feature fetch, compute_angle, BlendingNetwork.forward - is written once in
plain torch with a `dt` argument (front_end, restate): the two unit directions with their +1e-6, ray_diff with its clamp, the
projection, the per-level mask and its AND, align_corners=False zero-padded bilinear sampling of the image and the four levels,
ex, the min over all views, the pooling weights with +1e-8, weighted mean and variance, the eleven linear layers with ELU and
sigmoid, the -1e9 fill, the softmax over views.  It returns n_valid, the colour and per layer and (sample, view) the layer's
input vector and pre-activation.  Reverse mode (reverse) is torch autograd of sum_n gcolor_n . colour_n through it, the adjoint
of every pre-activation read with retain_grad, s a per-sample leaf.  An `operand` hook is applied to both factors of the ten
matrix-pipe layers: identity for fp32 / f32lds / bf16x3, hi + lo of two halves for f16x2.  Part A anchors it on the CPU: at
float32 it reproduces O.lookup_feature + O.blending on the golden points (mask bit-equal, the golden blend_rgb within 1e-3
relative), at float64 its assembled dW / db / ds equal float64 autograd through the oracle.

How.  A case is a scene, a weight set, an s and a fixed list of 301 points (601 for v8, 65,573 for `long`): random in the cube of
half-width 1.3 plus four points of every planted class (behind a camera; inside every finer level but outside a coarser one;
valid with u or v in [0, 0.5); exactly one valid view that is / is not the ex minimum; no valid view).  For every compared
quantity E = the largest |restatement(float32, the policy's operand hook) - restatement(float64)| over the case's points; the
kernel must lie within 8 E of float64, element by element.  The sample counts are launches over the first n points of the case.
Scenes: v5 37x45 floored / v8 16x21 floored down to 2x2 / v3 9x33 ceiled / v2 32x40 exact / v4 21x19 floored / v6 37x45 / v7
16x21 (the number is the view count; no camera repeated); weights golden, synth1, synth2; s in {0.2, -0.2, 10}, 0 (v2s0,
forward only), -80 on an evenly spaced ring (`saturated`: a valid view's ex is exactly zero in float32, E stated separately).
Part B: the forward kernels through the C entry points on NaN / sentinel-filled buffers (mask, idx, both, the device count,
scratch reuse, the wrapper).  Part C: surf_blend_backward's rows (E per layer and side), ds, colour; gfeats_t4 texel by texel
onto prefilled maps.  Part D: ops.blend_backward against float64 autograd.  Part E: refusals.  The sensitivity tests plant
the issue's twelve mistakes into the float32 restatement; the same comparators reject each (16-bit operands at 5 x the bound, every
other one above 10^4 x).

Left out, by rules the float64 reference decides (asserted <= 1 % per case): a point with a (view, level) margin - qz, u, W - u,
v, H - v in pixels - under EPS_VALID = 8 x the measured float32-vs-float64 margin difference, or a view within NEAR_PLANE of a
camera plane; its n_valid must lie within the float64 count +- its marginal views.  Backward only: the two smallest exponents
of a point closer than 100 x 8 x their measured difference.  Seen: 2 marginal points of 601 in v8, 1 tie of 301 in v7, none
elsewhere.

Statements of the issue that could not hold as worded, and what stands in their place:
  - the tie rule on ex itself: at s = 10 the two smallest ex of a point are both ~1e-7 and every gap lies under 100 x 8 x the
    largest |ex32 - ex64| of the case (265 and 298 of 301 points left out).  The rule is applied to the exponents |s| (dot - 1),
    which order the views as ex does and carry one float32 error scale.
  - the margin difference is measured where the projection can decide a mask (in front of the camera plane by NEAR_PLANE, within
    four map sizes of the image); nearer to a camera plane u and v lose digits without bound, such a view is marginal by rule.
  - E per case, not per launch: the colours of a one-point launch have an E of three numbers, which can be zero by luck.
  - "a level narrower than 2" was refused by surf_blend_split alone; surf_blend and surf_blend_backward now refuse it too.
    surf_blend_backward has no n_level argument.
  - the colour hardly depends on the MLP's operand precision (the 16-bit plant moves it by 5 x the bound, an f16x2 operand by
    nothing measurable: E_FWD_F16X2 = E_FWD_ID): per element the colour pins the front end, the pooling and the softmax; the
    layers are pinned per element by part C for blend_bwd.hip only.
  - the batch sums: 8 E + u sum|terms| for the assembled dW / db / ds (u = 2^-24; E is the error of ONE float32 summation
    order), and 8 E + sqrt(m) u (|prior| + sum|terms|) for a texel that m atomics reach in free order on top of its prior value,
    as tests/test_sdf_train_kernels.py derived; the ratios against 8 E alone are printed beside them.

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest): the largest E over the cases, per part
    forward colour, identity hook   E_FWD_ID = 4.14e-06        (case long; the 301-point cases 1.3e-06 .. 3.6e-06)
    forward colour, f16x2 hook      E_FWD_F16X2 = 4.14e-06
    forward colour, saturated       E_FWD_SATURATED = 1.83e-06
    rows, layer inputs              E_ROWS_IN = 4.19e-05
    rows, adjoints                  E_ROWS_ADJ = 9.48e-06
    ds per sample                   E_DS = 3.30e-06
    recomputed colour               E_BWD_COLOR = 3.56e-06
    feature-map gradients           E_GFEATS = 4.96e-06
    assembled dW, db                E_DW = 1.39e-05
    assembled ds                    E_DS_SUM = 3.17e-06
Seen on an MI355X, largest |kernel - float64| / bound per part and kernel:
    forward colour (8 E)      blend.hip 0.125 (v5, v6, v7)   f32lds 0.125 (v5, v6)   bf16x3 0.139 (v4)   f16x2 0.125 (v4, v5, v6);
                              `long` 0.100 and `saturated` 0.117 on all four; n_valid equal to float64 everywhere
    rows (8 E)                0.347 (ds, v4), 0.248 (ray_dir_fc.0 adjoints, v3), every other layer and case under 0.16
    feature-map gradients     0.386 (v8) with the atomics' term; against 8 E alone 0.930 (v8), 0.368 (v6), else under 0.26.  That
                              8 E alone does not hold for sound arithmetic is shown on the CPU: the float32 contributions of v8
                              added onto the prior in ten random orders reach 1.09 x 8 E.
    assembled gradients       0.443 (vis_fc2.2.bias, v7) with u sum|terms|; against 8 E alone 2.06 (vis_fc2.2.bias, v8 with
                              n = 601: 4207 rows through colgram's matrix-pipe plan), 0.80 (v7), else under 0.66
    (v2, one source view: the colour is that view's rgb whatever the network says; its gradients are exact zeros on both sides.)
What the new cases found in the kernels (both fixed in the commit that added this file): the forward kernels ANDed the view
mask of the two lane halves with `ok = ok && (__shfl_xor(ok, 32) != 0)`, a cross-lane exchange behind a short-circuit: a point
inside levels 0, 1 of a floored pyramid and outside level 2 or 3 was counted as valid by all four forward kernels (n_valid 7
instead of 5, colours off by up to 0.34; case v8, first point); and blend_split.hip carried a view's mask as `ex > 0`, which
drops a valid view whose ex underflows to zero (case `saturated`).
"""
import ctypes
import functools
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import surf_oracle as O

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FACTOR = 8.0
U = 2.0 ** -24
TAIL = 4                                             # spare rows behind every output buffer
NV_SENTINEL = 0xEE                                   # prefill of n_valid
PREFIX = "implicit_surface.color_network."
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYERS = [  # (state_dict prefix, in, out, IN column, ADJ column) of surf_blend_backward's rows: ops._BLEND_LAYERS
    ("ray_dir_fc.0", 4, 16, 0, 4), ("ray_dir_fc.2", 16, 19, 20, 36), ("base_fc.0", 57, 64, 55, 112), ("base_fc.2", 64, 32, 176, 240),
    ("vis_fc.0", 32, 32, 272, 304), ("vis_fc.2", 32, 33, 336, 368), ("vis_fc2.0", 32, 32, 401, 433), ("vis_fc2.2", 32, 1, 465, 497),
    ("rgb_fc.0", 37, 16, 498, 535), ("rgb_fc.2", 16, 8, 551, 567), ("rgb_fc.4", 8, 1, 575, 583)]
ROW = 584
FMA_LAYERS = ("vis_fc2.2", "rgb_fc.4")               # the two layers that do not run on the matrix pipe (NKS of blend_split.hip)
KERNELS = ("f32", "f32lds", "bf16x3", "f16x2")       # blend.hip | blend_split.hip's three policies
SPLIT = KERNELS[1:]
SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 301)
BSIZES = (1, 2, 3, 17, 64, 65, 301)
LONG_N = 256 * 8 * 32 + 37                           # the first size at which a wavefront of the persistent grid takes a second tile
N_PTS = 301
SUM_TERM = True                                      # assembled sums: 8 E + u sum|terms| (docstring)
HALF_WIDTH = 1.3
NEAR_PLANE = 0.15                                    # |qz| below which a view's projection is called ill conditioned


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# scenes, weights, points
# ------------------------------------------------------------------------------------------------------------------


def _look_at(eye):
    """c2w of a camera at `eye` looking at the origin (x right, y down, z forward)."""
    eye = torch.tensor(eye, dtype=F64)
    f = -eye / eye.norm()
    r = torch.linalg.cross(f, torch.tensor([0.0, 0.0, 1.0], dtype=F64))
    r = r / r.norm()
    d = torch.linalg.cross(f, r)
    m = torch.eye(4, dtype=F64)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, d, f, eye
    return m.to(F32)


def level_sizes(H, W, rounding):
    out = [(H, W)]
    for _ in range(3):
        H, W = ((H + 1) // 2, (W + 1) // 2) if rounding == "ceil" else (H // 2, W // 2)
        out.append((H, W))
    return out


SCENES = {  # name: (H, W, pyramid rounding, views, evenly spaced ring)
    "v5": (37, 45, "floor", 5, False), "v8": (16, 21, "floor", 8, False), "v3": (9, 33, "ceil", 3, False),
    "v2": (32, 40, "exact", 2, False), "v4": (21, 19, "floor", 4, False), "v6": (37, 45, "floor", 6, False),
    "v7": (16, 21, "floor", 7, False), "ring5": (37, 45, "floor", 5, True)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """A ring of distinct cameras at radius ~3 and different heights looking at the origin, focal length 1.1 W, random images
    in [0, 1] and random feature maps."""
    H, W, rounding, nv, even = SCENES[name]
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    eyes = []
    for k in range(nv):
        ang = 2.0 * math.pi * k / nv + (0.0 if even else 0.13 * math.sin(2.1 * k + 0.3))
        z = 0.15 * k if even else 0.9 * math.sin(1.3 * k + 0.4)
        rad = 3.0 + (0.0 if even else 0.1 * math.cos(1.7 * k))
        eyes.append((rad * math.cos(ang), rad * math.sin(ang), z))
    c2ws = torch.stack([_look_at(e) for e in eyes])
    K = torch.eye(4, dtype=F32)
    K[0, 0] = K[1, 1] = 1.1 * W
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    sizes = level_sizes(H, W, rounding)
    return types.SimpleNamespace(
        name=name, nv=nv, sizes=sizes, rounding=rounding, intrs=K[None].repeat(nv, 1, 1).contiguous(), c2ws=c2ws,
        imgs=torch.rand(nv, 3, H, W, generator=g), feats=[torch.randn(nv, 4, h, w, generator=g) * 0.5 for h, w in sizes])


@functools.lru_cache(maxsize=None)
def weight_set(kind):
    """'golden': the checkpoint's colour network; 'synth1' / 'synth2': N(0, (scale / sqrt(fan_in))^2), biases 0.1."""
    if kind == "golden":
        z = np.load(os.path.join(GOLDEN, "weights.npz"))
        return {k[len(PREFIX):]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith(PREFIX)}
    scale = {"synth1": 1.0, "synth2": 2.0}[kind]
    g = torch.Generator().manual_seed(int(scale) + 70)
    sd = {"s": torch.tensor(0.2)}
    for name, cin, cout, _, _ in LAYERS:
        sd[name + ".weight"] = torch.randn(cout, cin, generator=g) * (scale / math.sqrt(cin))
        sd[name + ".bias"] = torch.full((cout,), 0.1)
    return sd


CASES = {  # name: (scene, weights, s, points, backward too)
    "v5": ("v5", "golden", 0.2, N_PTS, True), "v8": ("v8", "synth1", -0.2, 601, True), "v3": ("v3", "synth2", 10.0, N_PTS, True),
    "v2": ("v2", "golden", 0.2, N_PTS, True), "v2s0": ("v2", "synth1", 0.0, N_PTS, False), "v4": ("v4", "synth2", -0.2, N_PTS, True),
    "v6": ("v6", "synth1", 10.0, N_PTS, True), "v7": ("v7", "golden", -0.2, N_PTS, True),
    "saturated": ("ring5", "golden", -80.0, N_PTS, False), "long": ("v3", "synth1", 0.2, LONG_N, False)}
SHORT = [k for k in CASES if k != "long"]
BACKWARD = [k for k, v in CASES.items() if v[4]]
PLANTED = ("behind", "coarse_out", "border", "one_valid_min", "one_valid_not_min", "none_valid")


def classify(sc, pts):
    """Which planted class a point is in, decided by the float64 restatement's front end alone."""
    c = types.SimpleNamespace(scene=sc, pts=pts, sd=weight_set("synth1"), s=0.2, n=pts.shape[0])
    fe = front_end(c, F64)
    nvd = fe.mask.sum(1)
    only = fe.mask.float().argmax(1)
    is_min = fe.rd[..., 3].argmin(1) == only                      # ex is increasing in dot: the smallest dot is the ex minimum
    finer_in = torch.cumprod(fe.level_in.long(), dim=2).bool()   # inside levels 0..l
    coarse_out = (finer_in[:, :, :3] & ~fe.level_in[:, :, 1:]).any(2).any(1)
    border = (fe.mask[:, :, None] & (((fe.u >= 0) & (fe.u < 0.5)) | ((fe.v >= 0) & (fe.v < 0.5)))).any(2).any(1)
    return {"behind": (fe.qz < 0).any(1), "coarse_out": coarse_out, "border": border, "one_valid_min": (nvd == 1) & is_min,
            "one_valid_not_min": (nvd == 1) & ~is_min, "none_valid": nvd == 0}


def wanted_classes(sc):
    out = [k for k in PLANTED if not (k == "coarse_out" and sc.rounding != "floor") and not (k == "one_valid_not_min" and sc.nv == 2)]
    return out


@functools.lru_cache(maxsize=None)
def points(scene_name, n):
    """n points: random in the cube of half-width 1.3, with four points of every planted class among the first 301 (found among
    random candidates of a wider cube by the float64 front end), in a fixed random order."""
    sc = scene(scene_name)
    g = torch.Generator().manual_seed(77 + sum(map(ord, scene_name)))
    if n > 1000:
        return ((torch.rand(n, 3, generator=g) * 2 - 1) * HALF_WIDTH).contiguous()
    cand = (torch.rand(40000, 3, generator=g) * 2 - 1) * 4.0
    cand[:20000] *= 0.4
    cls = classify(sc, cand)
    clear = front_end(types.SimpleNamespace(scene=sc, pts=cand), F64).qz.abs().min(1).values > 2 * NEAR_PLANE
    cls = {k: v & clear for k, v in cls.items()}
    planted = torch.cat([cand[cls[k]][:4] for k in wanted_classes(sc)])
    head = torch.cat([planted, (torch.rand(N_PTS - planted.shape[0], 3, generator=g) * 2 - 1) * HALF_WIDTH])
    head = head[torch.randperm(N_PTS, generator=g)]
    rest = (torch.rand(n - N_PTS, 3, generator=g) * 2 - 1) * HALF_WIDTH
    return torch.cat([head, rest]).contiguous()


@functools.lru_cache(maxsize=None)
def case(name):
    sname, wname, s, n, _ = CASES[name]
    sd = dict(weight_set(wname))
    sd["s"] = torch.tensor(float(s))
    g = torch.Generator().manual_seed(5 + sum(map(ord, name)))
    pts = points(sname, n)
    return types.SimpleNamespace(name=name, scene=scene(sname), sd=sd, s=float(s), pts=pts, n=n, gcolor=torch.randn(n, 3, generator=g))


# ------------------------------------------------------------------------------------------------------------------
# A. the restatement (dt = float64: the reference; dt = float32: the oracle's arithmetic)
# ------------------------------------------------------------------------------------------------------------------


def _r16(x):
    """fp32 values rounded to 16 significant bits."""
    bits = x.contiguous().view(torch.int32)
    return ((bits + 0x80) & ~0xFF).view(torch.float32)


def hook_f16x2(x):
    """The f16x2 policy's operand: hi + lo with hi = half(x), lo = half(x - hi) (include/surf_hip.h)."""
    hi = x.half().to(x.dtype)
    return hi + (x - hi).half().to(x.dtype)


HOOKS = {"f32": None, "f32lds": None, "bf16x3": None, "f16x2": hook_f16x2}   # a three-way bf16 split is exact: identity
EKEY = {"f32": "id", "f32lds": "id", "bf16x3": "id", "f16x2": "f16x2"}


def bilinear(img, gx, gy):
    """grid_sample(align_corners=False, zeros) at pixel coordinates: img (C, H, W) -> (n, C); the four taps' flat texel index
    (n, 4) (-1 outside the map) and weight (n, 4)."""
    C, H, W = img.shape
    x0, y0 = torch.floor(gx), torch.floor(gy)
    tx, ty = gx - x0, gy - y0
    x0, y0 = x0.detach().long(), y0.detach().long()
    flat = img.reshape(C, H * W)
    out, idx, wgt = 0.0, [], []
    for dy, wy in ((0, 1.0 - ty), (1, ty)):
        for dx, wx in ((0, 1.0 - tx), (1, tx)):
            xi, yi = x0 + dx, y0 + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            lin = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
            w = wx * wy * ok.to(img.dtype)
            out = out + flat[:, lin].t() * w[:, None]
            idx.append(torch.where(ok, lin, torch.full_like(lin, -1)))
            wgt.append(w)
    return out, torch.stack(idx, 1), torch.stack(wgt, 1)


def front_end(c, dt, plant=None, feats=None):
    """lookup_feature / compute_angle (projector.py:485-556) for every source view: the two unit directions with their +1e-6,
    ray_diff with its clamp, the projection, the per-level mask and its AND, the bilinear samples.  Expression by expression
    as O.lookup_feature, so that float32 gives the oracle's bits."""
    sc = c.scene
    P, C, Ks = c.pts.to(dt), sc.c2ws.to(dt), sc.intrs.to(dt)
    imgs = sc.imgs.to(dt)
    feats = [f.to(dt) for f in sc.feats] if feats is None else feats
    n, V = P.shape[0], sc.nv - 1
    o_ref = C[0, :3, 3]
    rd, rgbf, masks, lvl_in, us, vs, qzs, margins, taps = [], [], [], [], [], [], [], [], {}
    for j in range(1, V + 1):
        a = o_ref[None] - P
        a = a / (torch.linalg.norm(a, dim=-1, keepdim=True) + 1e-6)
        b = C[j, :3, 3][None] - P
        b = b / (torch.linalg.norm(b, dim=-1, keepdim=True) + 1e-6)
        d = a - b
        dn = torch.linalg.norm(d, dim=-1, keepdim=True)
        rd.append(torch.cat([d / dn.clamp(min=1e-6), (a * b).sum(-1, keepdim=True)], dim=-1))
        chans, mask, lin, uu, vv, mm = [], torch.ones(n, dtype=torch.bool), [], [], [], []
        for i, feat in enumerate(feats):
            H, W = feat.shape[-2:]
            K = Ks[j].clone()
            K[:2] = K[:2] * (0.5 ** i)
            w2c = torch.inverse(C[j])
            hom = torch.cat([P, torch.ones_like(P[:, :1])], dim=1)
            cam = (hom @ w2c.t())[:, :3]
            q = cam @ K[:3, :3].t()
            u = q[:, 0] / q[:, 2]
            v = q[:, 1] / q[:, 2]
            nx = u / ((W - 1) / 2) - 1
            ny = v / ((H - 1) / 2) - 1
            inside = (q[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            lin.append(inside)
            if not (plant == "drop_level" and i == 3):
                mask = mask & inside
            if plant == "align_corners":
                gx, gy = O.unnormalize(nx, W, True), O.unnormalize(ny, H, True)
            else:
                gx, gy = O.unnormalize(nx, W, False), O.unnormalize(ny, H, False)
            if i == 0:
                chans.append(bilinear(imgs[j], gx, gy)[0])
                qzs.append(q[:, 2])
            t, tidx, twgt = bilinear(feat[j], gx, gy)
            chans.append(t)
            taps[(j, i)] = (tidx, twgt)
            uu.append(u)
            vv.append(v)
            mm.append(torch.stack([q[:, 2], u, W - u, v, H - v], dim=-1))
        rgbf.append(torch.cat(chans, dim=-1))
        masks.append(mask)
        lvl_in.append(torch.stack(lin, 1))
        us.append(torch.stack(uu, 1))
        vs.append(torch.stack(vv, 1))
        margins.append(torch.stack(mm, 1))
    return types.SimpleNamespace(rgb_feat=torch.stack(rgbf, 1), rd=torch.stack(rd, 1), mask=torch.stack(masks, 1),
                                 level_in=torch.stack(lvl_in, 1), u=torch.stack(us, 1), v=torch.stack(vs, 1), qz=torch.stack(qzs, 1),
                                 margins=torch.stack(margins, 1).detach(), taps=taps)


class _EluD1(torch.autograd.Function):
    """The planted mistake `ELU derivative 1 everywhere`."""
    @staticmethod
    def forward(ctx, x):
        return torch.where(x > 0, x, torch.expm1(x.clamp(max=0)))

    @staticmethod
    def backward(ctx, g):
        return g


def restate(c, dt, hook=None, plant=None, leaves=None):
    """The whole operation.  Returns n_valid, the colour and, per layer and (sample, view), the layer's input vector (ins) and
    its pre-activation (pres).  hook: applied to both factors of the ten matrix-pipe layers.  leaves: the parameters, the
    per-sample s and the feature maps as autograd leaves (reverse)."""
    sd = {k: v.to(dt) for k, v in c.sd.items()} if leaves is None else leaves.sd
    fe = front_end(c, dt, plant, None if leaves is None else leaves.feats)
    n, V = fe.mask.shape
    s_n = sd["s"].reshape(1).expand(n) if leaves is None else leaves.s_n
    ident = lambda x: x
    hook = hook or ident
    if plant == "round16":
        hook = _r16
    ins, pres = {}, {}

    def elu(x):
        if plant == "elu_d1":
            return _EluD1.apply(x)
        return torch.where(x > 0, x, torch.expm1(x.clamp(max=0)))

    def lin(x, name):
        h = ident if name in FMA_LAYERS else hook
        pre = h(x) @ h(sd[name + ".weight"]).t() + sd[name + ".bias"]
        ins[name], pres[name] = x, pre
        return pre

    rgb_feat, ray_diff = fe.rgb_feat, fe.rd
    if leaves is not None:
        rgb_feat.retain_grad()
    m = fe.mask[:, :, None].to(dt)
    dfeat = elu(lin(elu(lin(ray_diff, "ray_dir_fc.0")), "ray_dir_fc.2"))
    rgb_in = rgb_feat[..., :3]
    if plant == "rgb_swap":
        rgb_in = rgb_in.roll(1, dims=1)
    f = rgb_feat + dfeat
    dot = ray_diff[..., 3:4]
    ex = torch.exp(torch.abs(s_n)[:, None, None] * (dot - 1))
    emin = ex.min(dim=1, keepdim=True).values
    if plant == "min_valid":
        emin = torch.where(fe.mask.any(1)[:, None, None], ex.masked_fill(~fe.mask[:, :, None], float("inf")).min(dim=1, keepdim=True).values, emin)
    w = (ex - emin) * m
    w = w / (w.sum(dim=1, keepdim=True) + (0.0 if plant == "no_eps" else 1e-8))
    mean = (f * w).sum(dim=1, keepdim=True)
    var = (w * (f if plant == "var_zero" else f - mean) ** 2).sum(dim=1, keepdim=True)
    x = torch.cat([mean.expand(-1, V, -1), var.expand(-1, V, -1), f], dim=-1)
    x = elu(lin(elu(lin(x, "base_fc.0")), "base_fc.2"))
    t = elu(lin(elu(lin(x * w, "vis_fc.0")), "vis_fc.2"))
    x = x + t[..., :-1]
    vis = torch.sigmoid(t[..., -1:]) * (1.0 if plant == "vis_unmasked" else m)
    vis = torch.sigmoid(lin(elu(lin(x * vis, "vis_fc2.0")), "vis_fc2.2")) * m
    r = lin(elu(lin(elu(lin(torch.cat([x, vis, ray_diff], dim=-1), "rgb_fc.0")), "rgb_fc.2")), "rgb_fc.4")
    if plant != "no_fill":
        r = torch.where(m == 0, torch.full_like(r, -1e9), r)
    beta = torch.softmax(r, dim=1)
    color = (rgb_in * beta).sum(dim=1)
    return types.SimpleNamespace(n_valid=fe.mask.sum(1), color=color, ins=ins, pres=pres, mask=fe.mask, ex=ex[..., 0], fe=fe,
                                 expo=(torch.abs(s_n)[:, None, None] * (dot - 1))[..., 0].detach(),
                                 rgb_feat=rgb_feat, n=n, V=V)


def reverse(c, dt, plant=None):
    """Reverse mode: torch autograd of sum_n gcolor_n . colour_n through the restatement at dt.  rows (n, V, ROW) in the layout
    of surf_blend_backward, ds (n) (s is a per-sample leaf), the parameter gradients, the feature maps' gradients (nv, 4, h, w)."""
    lv = types.SimpleNamespace(sd={k: v.to(dt).clone().requires_grad_(True) for k, v in c.sd.items() if k != "s"},
                               feats=[f.to(dt).clone().requires_grad_(True) for f in c.scene.feats],
                               s_n=torch.full((c.n,), c.s, dtype=dt).requires_grad_(True))
    lv.sd["s"] = None
    r = restate(c, dt, plant=plant, leaves=lv)
    for p in r.pres.values():
        p.retain_grad()
    (r.color * c.gcolor.to(dt)).sum().backward()
    rows = torch.zeros(r.n, r.V, ROW, dtype=dt)
    for name, cin, cout, c_in, c_ad in LAYERS:
        rows[..., c_in:c_in + cin] = r.ins[name].detach()
        rows[..., c_ad:c_ad + cout] = r.pres[name].grad
    ds = lv.s_n.grad.clone()
    if plant == "ds_sign" and c.s < 0:
        ds = -ds
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.sd.items() if v is not None}
    grads["s"] = ds.sum()
    return types.SimpleNamespace(rows=rows, ds=ds, color=r.color.detach(), grads=grads, gfeats=[f.grad for f in lv.feats],
                                 fbar=r.rgb_feat.grad, r=r)


def assemble(rows, absolute=False):
    """dW = adj^T in, db = sum adj over the (sample, view) rows, as ops.blend_backward assembles them."""
    flat = rows.reshape(-1, ROW)
    flat = flat.abs() if absolute else flat
    out = {}
    for name, cin, cout, c_in, c_ad in LAYERS:
        out[name + ".weight"] = flat[:, c_ad:c_ad + cout].t() @ flat[:, c_in:c_in + cin]
        out[name + ".bias"] = flat[:, c_ad:c_ad + cout].sum(0)
    return out


# ------------------------------------------------------------------------------------------------------------------
# references, E, the rules that leave a point out
# ------------------------------------------------------------------------------------------------------------------


def _maxabs(a, b):
    d = (a.double() - b.double()).abs()
    return float(d.max()) if d.numel() else 0.0


@functools.lru_cache(maxsize=None)
def reference(name):
    """Forward reference of a case: float64 colour and n_valid, E per operand hook, the marginal points."""
    c = case(name)
    with torch.no_grad():
        r64, r32 = restate(c, F64), restate(c, F32)
        r32h = restate(c, F32, hook=hook_f16x2)
    m64, m32 = r64.fe.margins, r32.fe.margins.double()
    # The margins' float32 error is measured where the projection is well conditioned and can decide a mask: 5 % of the ring's
    # radius in front of the camera plane, within four map sizes of the image.  Nearer to the camera plane u and v lose digits
    # without bound, so a view with |qz| < NEAR_PLANE is marginal by rule; farther out than four map sizes nothing can flip.
    near = (m64[..., :1].abs() < NEAR_PLANE)
    reach = 4.0 * max(c.scene.sizes[0])
    sane = torch.isfinite(m64) & torch.isfinite(m32) & ~near & (m64[..., :1] > 0) & (m64.abs() < reach)
    eps_valid = FACTOR * float((m64 - m32).abs()[sane].max())
    marg_view = ((m64.abs() < eps_valid) | near).flatten(2).any(2)             # (n, V)
    marginal = marg_view.any(1)
    keep = ~marginal
    E = {"id": _maxabs(r32.color[keep], r64.color[keep]), "f16x2": _maxabs(r32h.color[keep], r64.color[keep])}
    return types.SimpleNamespace(c=c, r64=r64, r32=r32, r32h=r32h, c64=r64.color, nv64=r64.n_valid, E=E, eps_valid=eps_valid,
                                 marginal=marginal, n_marg=marg_view.sum(1), expo_diff=_maxabs(r32.expo, r64.expo),
                                 span=float(r64.color.max() - r64.color.min()))


@functools.lru_cache(maxsize=None)
def reference_bwd(name):
    """Backward reference: rows / ds / colour per sample with E per layer and side, and the points the tie rule leaves out."""
    c, f = case(name), reference(name)
    b64, b32 = reverse(c, F64), reverse(c, F32)
    ex = f.r64.expo                      # the exponents |s| (dot - 1): ex's order, on a scale where one float32 error fits all
    if ex.shape[1] > 1:
        two = ex.topk(2, dim=1, largest=False).values
        tie = (two[:, 1] - two[:, 0]) < 100.0 * FACTOR * f.expo_diff
    else:
        tie = torch.zeros(c.n, dtype=torch.bool)
    keep = ~(tie | f.marginal)
    E = {}
    for lname, cin, cout, c_in, c_ad in LAYERS:
        E[lname + ".in"] = _maxabs(b32.rows[keep][..., c_in:c_in + cin], b64.rows[keep][..., c_in:c_in + cin])
        E[lname + ".adj"] = _maxabs(b32.rows[keep][..., c_ad:c_ad + cout], b64.rows[keep][..., c_ad:c_ad + cout])
    E["ds"] = _maxabs(b32.ds[keep], b64.ds[keep])
    E["color"] = _maxabs(b32.color[keep], b64.color[keep])
    return types.SimpleNamespace(c=c, b64=b64, b32=b32, E=E, keep=keep, tie=tie)


@functools.lru_cache(maxsize=None)
def reference_sums(name, n):
    """The batch sums over the kept points among the first n: parameter gradients and feature-map gradients in float64 and
    float32 (E of the summed quantity), the sums of the terms' magnitudes and the texels' contribution counts."""
    c, rb = case(name), reference_bwd(name)
    sel = torch.nonzero(rb.keep[:n])[:, 0]
    sub = types.SimpleNamespace(name=c.name, scene=c.scene, sd=c.sd, s=c.s, pts=c.pts[sel].contiguous(), n=int(sel.numel()),
                                gcolor=c.gcolor[sel].contiguous())
    b64, b32 = reverse(sub, F64), reverse(sub, F32)
    absW = assemble(b64.rows, absolute=True)
    absW["s"] = b64.ds.abs().sum()
    E = {k: _maxabs(b32.grads[k], v) for k, v in b64.grads.items()}
    sumabs, count = [], []
    for i, (h, w) in enumerate(c.scene.sizes):
        sa, ct = torch.zeros(c.scene.nv, 4, h * w, dtype=F64), torch.zeros(c.scene.nv, h * w, dtype=F64)
        for j in range(1, c.scene.nv):
            tidx, twgt = b64.r.fe.taps[(j, i)]
            live = (tidx >= 0) & (twgt != 0)
            fb = b64.fbar[:, j - 1, 3 + 4 * i:7 + 4 * i].abs()                # (n, 4)
            contrib = (fb[:, None, :] * twgt[:, :, None].abs())[live]           # (taps, 4)
            sa[j].index_add_(1, tidx[live], contrib.t())
            ct[j].index_add_(0, tidx[live], torch.ones(int(live.sum()), dtype=F64))
        sumabs.append(sa.reshape(c.scene.nv, 4, h, w))
        count.append(ct.reshape(c.scene.nv, 1, h, w))
    Eg = [_maxabs(a, b) for a, b in zip(b32.gfeats, b64.gfeats)]
    return types.SimpleNamespace(sel=sel, grads64=b64.grads, E=E, absW=absW, gfeats64=b64.gfeats, Eg=Eg, sumabs=sumabs, count=count,
                                 rows=int(sel.numel()) * (c.scene.nv - 1))


# ------------------------------------------------------------------------------------------------------------------
# comparators (the same for the planted float32 restatements and for the kernels)
# ------------------------------------------------------------------------------------------------------------------


def _ratio(err, bound):
    """max err / bound; NaN or an error above a zero bound counts as infinite."""
    err = err.double()
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    if err.numel() == 0:
        return 0.0
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max())


def nan_buffer(rows, width):
    return torch.full((rows + TAIL, width), float("nan"), dtype=F32)


def _bits(x):
    return x.contiguous().view(torch.int32) if x.dtype == F32 else x


def judge_forward(cbuf, nbuf, evaluated, ref, ekey, prefill=None):
    """cbuf (N + TAIL, 3), nbuf (N + TAIL) after a launch that had to evaluate the point rows `evaluated` (LongTensor) and nothing
    else.  Returns (largest |colour - float64| / (8 E) over the kept points, list of complaints)."""
    bad = []
    touched = torch.zeros(cbuf.shape[0], dtype=torch.bool)
    touched[evaluated] = True
    before_c = torch.full_like(cbuf, float("nan")) if prefill is None else prefill[0]
    before_n = torch.full_like(nbuf, NV_SENTINEL) if prefill is None else prefill[1]
    if not torch.equal(_bits(cbuf)[~touched], _bits(before_c)[~touched]):
        bad.append("a colour row that must keep its bits was written")
    if not torch.equal(nbuf[~touched], before_n[~touched]):
        bad.append("an n_valid entry that must keep its bits was written")
    col, nv = cbuf[evaluated].double(), nbuf[evaluated].long()
    keep = ~ref.marginal[evaluated]
    if not torch.equal(nv[keep], ref.nv64[evaluated][keep]):
        bad.append("n_valid differs from float64")
    if bool(((nv - ref.nv64[evaluated]).abs() > ref.n_marg[evaluated]).any()):
        bad.append("n_valid of a marginal point outside float64 +- marginal views")
    ratio = _ratio((col - ref.c64[evaluated])[keep], FACTOR * ref.E[ekey])
    return ratio, bad


def judge_backward(rows_buf, ds, color, samples, rb):
    """rows_buf (n + TAIL, V, ROW) NaN-prefilled, ds (n), color (n, 3) of a launch over the point rows `samples`.  Returns
    {quantity: largest |kernel - float64| / (8 E)} over the kept samples, and complaints."""
    n = samples.numel()
    bad = []
    if not bool(torch.isnan(rows_buf[n:]).all()):
        bad.append("a spare row behind `rows` was written")
    keep = rb.keep[samples]
    ref = rb.b64
    out = {}
    got = rows_buf[:n][keep].double()
    want = ref.rows[samples][keep]
    for lname, cin, cout, c_in, c_ad in LAYERS:
        out[lname + ".in"] = _ratio((got[..., c_in:c_in + cin] - want[..., c_in:c_in + cin]).abs(), FACTOR * rb.E[lname + ".in"])
        out[lname + ".adj"] = _ratio((got[..., c_ad:c_ad + cout] - want[..., c_ad:c_ad + cout]).abs(), FACTOR * rb.E[lname + ".adj"])
    out["ds"] = _ratio((ds[:n][keep].double() - ref.ds[samples][keep]).abs(), FACTOR * rb.E["ds"])
    if color is not None:
        out["color"] = _ratio((color[:n][keep].double() - ref.color[samples][keep]).abs(), FACTOR * rb.E["color"])
    return out, bad


def judge_sums(got, rs, sum_term=SUM_TERM):
    """{name: gradient} against the float64 autograd: 8 E (E of the summed quantity) [+ u sum|terms|]."""
    out = {}
    for k, ref in rs.grads64.items():
        bound = FACTOR * rs.E[k] + (U * rs.absW[k].reshape(ref.shape) if sum_term else 0.0)
        out[k] = _ratio((got[k].reshape(ref.shape).double() - ref).abs(), bound)
    return out


def judge_gfeats(got, prior, rs, atomic_term=True):
    """got, prior: per level (nv, 4, h, w).  Texel by texel: prior + float64 gradient within 8 E + sqrt(m) u sum|terms|
    (m contributions added by atomics in any order onto the prior; |prior| is one of the terms); texels no sample reaches keep
    their bits."""
    out, bad = {}, []
    for i, (g, p, ref, sa, ct) in enumerate(zip(got, prior, rs.gfeats64, rs.sumabs, rs.count)):
        reached = (ct > 0).expand_as(g)
        if not torch.equal(_bits(g)[~reached], _bits(p)[~reached]):
            bad.append(f"level {i}: a texel no sample reaches was written")
        bound = torch.full_like(ref, FACTOR * rs.Eg[i])
        if atomic_term:
            bound = bound + torch.sqrt(ct) * U * (sa + p.double().abs())
        out[f"gfeats[{i}]"] = _ratio((g.double() - (p.double() + ref)).abs()[reached], bound[reached])
    return out, bad


# ------------------------------------------------------------------------------------------------------------------
# CPU tests
# ------------------------------------------------------------------------------------------------------------------


def _golden():
    load = lambda f: {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, f)).items()}
    sc, fpn, rnd = load("scene.npz"), load("fpn.npz"), load("render.npz")
    feats = [fpn[f"out{i}"] for i in range(4)][::-1]
    s = types.SimpleNamespace(name="golden", nv=int(sc["intrs"].shape[0]), sizes=[tuple(f.shape[-2:]) for f in feats], rounding="exact",
                              intrs=sc["intrs"], c2ws=sc["c2ws"], imgs=sc["imgs"], feats=feats)
    sd = weight_set("golden")
    g = torch.Generator().manual_seed(3)
    n = rnd["pts"].shape[0]
    return types.SimpleNamespace(name="golden", scene=s, sd=sd, s=float(sd["s"]), pts=rnd["pts"], n=n,
                                 gcolor=torch.randn(n, 3, generator=g)), rnd


def test_restatement_float32_is_the_oracle():
    """At float32 the restatement reproduces O.lookup_feature + O.blending on the golden scene's points: mask bit-equal, features
    and colour to what two evaluation orders of the same float32 arithmetic allow (a few ulps of the operands: 2e-6 on values of
    order one); the golden blend_rgb within 1e-3 relative."""
    c, rnd = _golden()
    sc = c.scene
    with torch.no_grad():
        r = restate(c, F32)
        rf, rdiff, mval = O.lookup_feature(c.pts, sc.imgs, sc.intrs, sc.c2ws, sc.feats)
        col = O.blending({PREFIX + k: v for k, v in c.sd.items()}, rf, rdiff, mval)
    assert torch.equal(r.mask, mval) and torch.equal(r.mask, rnd["mask_valid"].bool())
    assert 0 < int(mval.sum()) < mval.numel()
    ulps = lambda ref: 4 * 2.0 ** -23 * max(1.0, float(ref.abs().max()))
    assert _maxabs(r.fe.rgb_feat, rf) <= ulps(rf) and _maxabs(r.fe.rd, rdiff) <= ulps(rdiff)
    assert _maxabs(r.color, col) <= 2e-6, _maxabs(r.color, col)
    gold = rnd["blend_rgb"]
    assert bool(((r.color - gold).abs() <= 1e-3 * gold.abs() + 2e-5).all())


def test_restatement_float64_gradients_are_autograd_through_the_oracle():
    """At float64 the dW, db assembled from the restated rows and the summed ds equal float64 autograd through O.lookup_feature +
    O.blending."""
    c, _ = _golden()
    sc = c.scene
    b = reverse(c, F64)
    sd = {PREFIX + k: v.double().clone().requires_grad_(True) for k, v in c.sd.items()}
    rf, rdiff, mval = O.lookup_feature(c.pts.double(), sc.imgs.double(), sc.intrs.double(), sc.c2ws.double(), [f.double() for f in sc.feats])
    (O.blending(sd, rf, rdiff, mval) * c.gcolor.double()).sum().backward()
    asm = assemble(b.rows)
    asm["s"] = b.ds.sum()
    for k, v in sd.items():
        name = k[len(PREFIX):]
        scale = float(v.grad.abs().max()) + 1e-3              # (rgb_fc.4.bias: the softmax gradients sum to 0)
        assert _maxabs(asm[name].reshape(v.grad.shape), v.grad) <= 1e-9 * scale, name
        assert _maxabs(b.grads[name].reshape(v.grad.shape), v.grad) <= 1e-9 * scale, name


@pytest.mark.parametrize("name", SHORT)
def test_input_conditions(name):
    """Every count of valid views from 0 to nv - 1 occurs among the first 301 points, every planted class is present, the points a
    rule leaves out are at most 1 % of the case, and 8 E of the colour stays below 1e-3 x the colour range (no looser than the
    golden comparison)."""
    c, f = case(name), reference(name)
    V = c.scene.nv - 1
    hist = torch.bincount(f.nv64[:N_PTS], minlength=V + 1)
    print(f"[conditions] {name} valid-view histogram {hist.tolist()} marginal {int(f.marginal.sum())} eps_valid {f.eps_valid:.2e} "
          f"E {f.E} span {f.span:.3f}")
    assert bool((hist > 0).all()), hist
    cls = classify(c.scene, c.pts[:N_PTS])
    for k in wanted_classes(c.scene):
        assert int(cls[k].sum()) >= 1, k
    assert int(f.marginal.sum()) <= 0.01 * c.n
    for e in f.E.values():
        assert FACTOR * e < 1e-3 * f.span, (e, f.span)
    if CASES[name][4]:
        rb = reference_bwd(name)
        print(f"[conditions] {name} ties {int(rb.tie.sum())}")
        assert int((~rb.keep).sum()) <= 0.01 * c.n
    views = {SCENES[v[0]][3] for v in CASES.values()}
    assert views >= set(range(2, 9))


def test_saturated_case_condition():
    """`saturated`: at least 32 points with a valid view whose |s| (1 - dot) > 110 (ex = 0 in float32 whatever the device does
    with subnormals) and another valid view beside it; the float32 restatement keeps such a view, as the oracle does."""
    f = reference("saturated")
    dot = f.r64.fe.rd[..., 3]
    gone = f.r64.mask & (abs(f.c.s) * (1 - dot) > 110.0)
    hit = gone.any(1) & (f.r64.mask.sum(1) >= 2)
    assert int(hit.sum()) >= 32, int(hit.sum())
    assert float(f.r32.ex[gone].max()) == 0.0
    assert torch.equal(f.r32.n_valid, f.nv64)


def test_long_case_condition():
    c, f = case("long"), reference("long")
    assert c.n == LONG_N and int(f.marginal.sum()) <= 0.01 * c.n and FACTOR * max(f.E.values()) < 1e-3 * f.span


FWD_PLANTS = ("round16", "drop_level", "align_corners", "min_valid", "no_eps", "var_zero", "no_fill", "rgb_swap")
BWD_PLANTS = ("vis_unmasked", "elu_d1", "ds_sign")


def _as_buffers(r, n):
    cbuf, nbuf = nan_buffer(n, 3), torch.full((n + TAIL,), NV_SENTINEL, dtype=torch.uint8)
    cbuf[:n], nbuf[:n] = r.color[:n], r.n_valid[:n].to(torch.uint8)
    return cbuf, nbuf


@pytest.mark.parametrize("plant", (None,) + FWD_PLANTS + ("stray_write",))
def test_sensitivity_forward(plant):
    """The forward comparator accepts the float32 restatement and rejects each planted mistake (case v4: floored levels, three
    source views, synthetic weights of scale 2)."""
    f = reference("v4")
    with torch.no_grad():
        r = f.r32 if plant in (None, "stray_write") else restate(f.c, F32, plant=plant)
    cbuf, nbuf = _as_buffers(r, f.c.n)
    evaluated = torch.arange(f.c.n)
    if plant == "stray_write":
        evaluated = evaluated[:-1]
    ratio, bad = judge_forward(cbuf, nbuf, evaluated, f, "id")
    print(f"[sensitivity] forward {plant}: {ratio:.3g} {bad}")
    assert (ratio <= 1.0 and not bad) == (plant is None)


@pytest.mark.parametrize("plant", (None,) + BWD_PLANTS + ("stray_write",))
def test_sensitivity_backward(plant):
    """The backward comparator accepts the float32 restatement's rows / ds / colour and rejects each planted mistake (case v7:
    negative s, six source views)."""
    rb = reference_bwd("v7")
    b = rb.b32 if plant in (None, "stray_write") else reverse(rb.c, F32, plant=plant)
    n = rb.c.n
    buf = torch.full((n + TAIL, b.rows.shape[1], ROW), float("nan"), dtype=F32)
    buf[:n] = b.rows
    if plant == "stray_write":
        buf[n, 0, 0] = 0.0
    out, bad = judge_backward(buf, b.ds.float(), b.color.float(), torch.arange(n), rb)
    worst = max(out.values())
    print(f"[sensitivity] backward {plant}: {worst:.3g} {bad}")
    assert (worst <= 1.0 and not bad) == (plant is None)


def test_sensitivity_sums():
    """The comparators of the batch sums accept the float32 autograd and reject rows rounded to 16 bits / a texel written that
    no sample reaches."""
    rs = reference_sums("v7", N_PTS)
    c = case("v7")
    sub = types.SimpleNamespace(name=c.name, scene=c.scene, sd=c.sd, s=c.s, pts=c.pts[rs.sel].contiguous(), n=int(rs.sel.numel()),
                                gcolor=c.gcolor[rs.sel].contiguous())
    b32 = reverse(sub, F32)
    assert max(judge_sums(b32.grads, rs).values()) <= 1.0
    asm = assemble(_r16(b32.rows))
    asm["s"] = b32.ds.sum()
    assert max(judge_sums(asm, rs).values()) > 1.0
    prior = [torch.randn(f.shape, generator=torch.Generator().manual_seed(9)) * 0.5 for f in c.scene.feats]
    got = [(p + g).float() for p, g in zip(prior, b32.gfeats)]
    out, bad = judge_gfeats(got, prior, rs)
    assert max(out.values()) <= 1.0 and not bad, (out, bad)
    got[0][0, 0, 0, 0] += 1.0                                     # the reference view's map: no sample reaches it
    assert judge_gfeats(got, prior, rs)[1]
    got = [(p + 1.001 * g).float() for p, g in zip(prior, b32.gfeats)]
    assert max(judge_gfeats(got, prior, rs)[0].values()) > 1.0


def test_shape_checks_refuse_before_any_launch():
    """ops.blend and ops.blend_backward raise ValueError for an image that has not the finest level's shape, a map whose leading
    dimension is not cams.nv, and a level count other than four.  CPU tensors: the checks come before anything else."""
    from surf_amd import ops
    sc = scene("v3")
    cams = types.SimpleNamespace(nv=sc.nv)
    t4 = lambda x: torch.zeros(x.shape[0], x.shape[2], x.shape[3], 4)
    feats, imgs = [t4(f) for f in sc.feats], t4(sc.imgs)
    pts = torch.zeros(4, 3)
    wrong = [(feats, imgs[:, :-1]), (feats, imgs[:, :, :-1]), (feats, imgs[:-1]), ([feats[0], feats[1][:-1]] + feats[2:], imgs),
             ([f[:-1] for f in feats], imgs[:-1]), (feats[:3], imgs), (feats + feats[-1:], imgs)]
    for fs, im in wrong:
        with pytest.raises(ValueError):
            ops.blend(pts, fs, im, cams, None)
        with pytest.raises(ValueError):
            ops.blend_backward(pts, None, pts, fs, im, cams, None)
    with pytest.raises(ValueError):
        ops.blend_backward(pts, None, pts, feats, imgs, cams, None, gfeats_t4=feats[:3])
    assert ops._BLEND_LAYERS == LAYERS


def measured():
    """The largest E per part over the cases."""
    fwd = [reference(k) for k in CASES]
    out = {"E_FWD_ID": max(f.E["id"] for f in fwd if f.c.name != "saturated"),
           "E_FWD_F16X2": max(f.E["f16x2"] for f in fwd if f.c.name != "saturated"),
           "E_FWD_SATURATED": max(reference("saturated").E.values())}
    rbs = [reference_bwd(k) for k in BACKWARD]
    out["E_ROWS_IN"] = max(v for rb in rbs for k, v in rb.E.items() if k.endswith(".in"))
    out["E_ROWS_ADJ"] = max(v for rb in rbs for k, v in rb.E.items() if k.endswith(".adj"))
    out["E_DS"] = max(rb.E["ds"] for rb in rbs)
    out["E_BWD_COLOR"] = max(rb.E["color"] for rb in rbs)
    sums = [reference_sums(k, N_PTS) for k in BACKWARD] + [reference_sums("v8", 601)]
    out["E_GFEATS"] = max(max(rs.Eg) for rs in sums)
    out["E_DW"] = max(v for rs in sums for k, v in rs.E.items() if k != "s")
    out["E_DS_SUM"] = max(rs.E["s"] for rs in sums)
    return out


def _recorded(label):
    return float(re.search(rf"{label} = ([0-9.e+-]+)", __doc__).group(1))


def test_measured_margins_are_recorded():
    """The E lines of the module docstring are the ones these inputs give (10 % of slack for another host's libm / BLAS)."""
    m = measured()
    for label, v in m.items():
        print(f"    {label} = {v:.2e}")
    for label, v in m.items():
        rec = _recorded(label)
        assert abs(v - rec) <= 0.1 * rec + 1e-30, (label, v, rec)


# ------------------------------------------------------------------------------------------------------------------
# GPU side
# ------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def dev_scene(name):
    from surf_amd import ops
    sc, d = scene(name), dev()
    feats_t4 = [ops.pack_texel4(f.to(d).contiguous()) for f in sc.feats]
    return types.SimpleNamespace(sc=sc, feats_t4=feats_t4, imgs_t4=ops.pack_texel4(sc.imgs.to(d).contiguous()),
                                 cams=ops.Cameras(sc.intrs, sc.c2ws), fp=ops._ptr_array(feats_t4),
                                 hw=(ctypes.c_int * 8)(*[int(v) for hw in sc.sizes for v in hw]))


def _prefixed(sd):
    return {PREFIX + k: v for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def dev_weights(name, kernel):
    """The case's weights packed for a forward kernel, or (kernel 'raw') the raw parameter vector of the backward kernel."""
    from surf_amd import ops
    if kernel == "raw":
        return torch.from_numpy(ops.blend_raw_weights(_prefixed(case(name).sd))).to(dev())
    return ops.blend_pack_weights(_prefixed(case(name).sd), dev(), precision=kernel)


def _scratch_for(n, nv, fill=0):
    from surf_amd import _lib
    need = max(int(_lib.lib().surf_blend_split_scratch_bytes(int(max(n, 1)), int(nv))), 4096)
    return torch.full((need,), fill, dtype=torch.uint8, device=dev())


def fwd_buffers(n):
    d = dev()
    return (torch.full((n + TAIL, 3), float("nan"), dtype=F32, device=d), torch.full((n + TAIL,), NV_SENTINEL, dtype=torch.uint8, device=d))


def fwd_call(kernel, ds, packed, pts, n, color, nvalid, mask=None, idx=None, d_n=None, scratch=None, over=None):
    """surf_blend / surf_blend_split / surf_blend_split_dn the way ops.blend calls them, on buffers the test owns; `over`
    replaces arguments by name (a dict)."""
    from surf_amd import _lib, ops
    L, cams = _lib.lib(), ds.cams
    a = dict(pts=ops._p(pts), mask=ops._p(mask), idx=ops._p(idx), n=n, fp=ds.fp, hw=ds.hw, n_level=4, imgs=ops._p(ds.imgs_t4),
             nv=cams.nv, intrs=ops._np_ptr(cams.intrs), w2c=ops._np_ptr(cams.w2c), c2w=ops._np_ptr(cams.c2w), w=ops._p(packed),
             color=ops._p(color), nvalid=ops._p(nvalid), d_n=ops._p(d_n))
    if kernel != "f32":
        scratch = _scratch_for(n, cams.nv) if scratch is None else scratch
        a["scratch"] = ops._p(scratch)
    a.update(over or {})
    try:
        if kernel == "f32":
            L.surf_blend(a["pts"], a["mask"], a["idx"], a["n"], a["fp"], a["hw"], a["n_level"], a["imgs"], a["nv"], a["intrs"],
                         a["w2c"], a["c2w"], a["w"], a["color"], a["nvalid"], ops._stream())
        elif d_n is not None:
            L.surf_blend_split_dn(a["pts"], a["idx"], a["n"], a["d_n"], a["fp"], a["hw"], a["n_level"], a["imgs"], a["nv"], a["intrs"],
                                  a["w2c"], a["c2w"], a["w"], ops._BLEND_ID[kernel], a["color"], a["nvalid"], a["scratch"], ops._stream())
        else:
            L.surf_blend_split(a["pts"], a["mask"], a["idx"], a["n"], a["fp"], a["hw"], a["n_level"], a["imgs"], a["nv"], a["intrs"],
                               a["w2c"], a["c2w"], a["w"], ops._BLEND_ID[kernel], a["color"], a["nvalid"], a["scratch"], ops._stream())
    finally:
        torch.cuda.synchronize()


def _fwd_judged(kernel, name, n, mask=None, idx=None, d_n=None, evaluated=None, scratch=None):
    c, f = case(name), reference(name)
    ds, packed = dev_scene(CASES[name][0]), dev_weights(name, kernel)
    pts = c.pts.to(dev())
    color, nvalid = fwd_buffers(c.n)
    fwd_call(kernel, ds, packed, pts, n, color, nvalid, mask=mask, idx=idx, d_n=d_n, scratch=scratch)
    evaluated = torch.arange(n) if evaluated is None else evaluated
    ratio, bad = judge_forward(color.cpu(), nvalid.cpu(), evaluated, f, EKEY[kernel])
    return ratio, bad, color, nvalid


@gpu
@pytest.mark.parametrize("name", SHORT)
@pytest.mark.parametrize("kernel", KERNELS)
def test_forward(kernel, name):
    """Part B: colours within 8 E of float64 and n_valid exact at every sample count (launches over the first n points of the
    case); the rows behind the first n keep their NaN / sentinel bits."""
    worst = (0.0, None)
    for n in SIZES:
        ratio, bad, _, _ = _fwd_judged(kernel, name, n)
        assert not bad, (n, bad)
        worst = (ratio, n) if ratio >= worst[0] else worst
    print(f"[margin] forward {kernel} {name} {worst[0]:.3f} (n = {worst[1]})")
    assert worst[0] <= 1.0, worst


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_forward_long_case(kernel):
    """n = 256 x 8 x 32 + 37: wavefronts of the persistent grid take a second tile from the counter; every row compared."""
    ratio, bad, _, _ = _fwd_judged(kernel, "long", LONG_N)
    print(f"[margin] forward {kernel} long {ratio:.3f}")
    assert not bad and ratio <= 1.0, (ratio, bad)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_forward_mask_and_idx(kernel):
    """`mask` without `idx`, `idx` alone (a permuted subset), and both (the mask is indexed like pts): exactly the selected rows
    are evaluated, every other row keeps its bits."""
    name, d = "v5", dev()
    c = case(name)
    g = torch.Generator().manual_seed(31)
    mask = (torch.rand(c.n, generator=g) > 0.4).to(torch.uint8)
    idx = torch.randperm(c.n, generator=g)[:150].to(torch.int32)
    for m, i, n, evaluated in ((mask, None, c.n, torch.nonzero(mask)[:, 0]), (None, idx, 150, idx.long()),
                               (mask, idx, 150, idx.long()[mask[idx.long()] != 0])):
        ratio, bad, _, _ = _fwd_judged(kernel, name, n, mask=None if m is None else m.to(d), idx=None if i is None else i.to(d),
                                       evaluated=evaluated)
        assert not bad and ratio <= 1.0, (ratio, bad)


@gpu
@pytest.mark.parametrize("kernel", SPLIT)
def test_forward_device_count(kernel):
    """surf_blend_split_dn: the count read from device memory lies below the capacity; a count of zero writes nothing."""
    name, d = "v7", dev()
    c = case(name)
    idx = torch.randperm(c.n, generator=torch.Generator().manual_seed(32))[:200].to(torch.int32)
    for count in (137, 0):
        d_n = torch.tensor([count], dtype=torch.int32, device=d)
        ratio, bad, _, _ = _fwd_judged(kernel, name, 200, idx=idx.to(d), d_n=d_n, evaluated=idx.long()[:count])
        assert not bad and ratio <= 1.0, (count, ratio, bad)


@gpu
@pytest.mark.parametrize("kernel", SPLIT)
def test_forward_scratch_reuse_is_deterministic(kernel):
    """Two launches of different sizes on one reused scratch give the bits of launches on fresh scratch."""
    name = "v8"
    nv = case(name).scene.nv
    shared = _scratch_for(N_PTS, nv, fill=0xA5)
    got = [_fwd_judged(kernel, name, n, scratch=shared)[2:] for n in (N_PTS, 65)]
    fresh = [_fwd_judged(kernel, name, n, scratch=_scratch_for(n, nv))[2:] for n in (N_PTS, 65)]
    for (c1, n1), (c2, n2) in zip(got, fresh):
        assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(n1, n2)


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_ops_blend_wrapper(kernel):
    """ops.blend on its zero-filled outputs: all rows, and with a mask (compacted inside) the masked-out rows stay zero."""
    from surf_amd import ops
    name, d = "v6", dev()
    c, f, ds = case(name), reference(name), dev_scene(CASES[name][0])
    pts = c.pts.to(d)
    mask = (torch.rand(c.n, generator=torch.Generator().manual_seed(33)) > 0.5).to(torch.uint8)
    zeros = (torch.zeros(c.n, 3), torch.zeros(c.n, dtype=torch.uint8))
    for m, evaluated in ((None, torch.arange(c.n)), (mask, torch.nonzero(mask)[:, 0])):
        color, nvalid = ops.blend(pts, ds.feats_t4, ds.imgs_t4, ds.cams, dev_weights(name, kernel), mask=None if m is None else m.to(d))
        torch.cuda.synchronize()
        ratio, bad = judge_forward(color.cpu(), nvalid.cpu(), evaluated, f, EKEY[kernel], prefill=zeros)
        assert not bad and ratio <= 1.0, (ratio, bad)


def bwd_call(ds, raw, pts, idx, n, gcolor, rows, dsb, color, gfeats=None, over=None):
    """surf_blend_backward the way ops.blend_backward calls it, on buffers the test owns."""
    from surf_amd import _lib, ops
    cams = ds.cams
    intr16 = np.ascontiguousarray(cams.intrs.reshape(cams.nv, -1))
    a = dict(pts=ops._p(pts), idx=ops._p(idx), n=n, gcolor=ops._p(gcolor), fp=ds.fp, hw=ds.hw, imgs=ops._p(ds.imgs_t4), nv=cams.nv,
             intrs=ops._np_ptr(intr16), w2c=ops._np_ptr(cams.w2c), c2w=ops._np_ptr(cams.c2w), w=ops._p(raw), rows=ops._p(rows),
             ds=ops._p(dsb), color=ops._p(color), gfeats=gfeats if gfeats is None or isinstance(gfeats, ctypes.Array) else ops._ptr_array(list(gfeats)))
    a.update(over or {})
    try:
        _lib.lib().surf_blend_backward(a["pts"], a["idx"], a["n"], a["gcolor"], a["fp"], a["hw"], a["imgs"], a["nv"], a["intrs"], a["w2c"],
                                       a["c2w"], a["w"], a["rows"], a["ds"], a["color"], a["gfeats"], ops._stream())
    finally:
        torch.cuda.synchronize()


def bwd_buffers(n, V):
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=F32, device=dev())
    return nan(n + TAIL, V, ROW), nan(n + TAIL), nan(n + TAIL, 3)


@gpu
@pytest.mark.parametrize("name", BACKWARD)
def test_backward_rows(name):
    """Part C: every [in | adj] column range of the 584-float rows, ds per sample and the recomputed colour within 8 E of the
    float64 restatement (E per layer and side), idx NULL at every sample count and idx given; the spare rows stay NaN."""
    c, rb, d = case(name), reference_bwd(name), dev()
    ds, raw = dev_scene(CASES[name][0]), dev_weights(name, "raw")
    pts, gcolor, V = c.pts.to(d), c.gcolor.to(d), c.scene.nv - 1
    idx = torch.randperm(c.n, generator=torch.Generator().manual_seed(34))[:100].to(torch.int32)
    worst = (0.0, None, None)
    for n, i in [(n, None) for n in BSIZES] + [(100, idx)]:
        rows, dsb, color = bwd_buffers(n, V)
        bwd_call(ds, raw, pts, None if i is None else i.to(d), n, gcolor, rows, dsb, color)
        samples = torch.arange(n) if i is None else i.long()
        out, bad = judge_backward(rows.cpu(), dsb.cpu(), color.cpu(), samples, rb)
        assert not bad and bool(torch.isnan(dsb[n:]).all()) and bool(torch.isnan(color[n:]).all()), (n, bad)
        k = max(out, key=out.get)
        worst = (out[k], k, n) if out[k] >= worst[0] else worst
    print(f"[margin] rows {name} {worst[0]:.3f} ({worst[1]}, n = {worst[2]})")
    assert worst[0] <= 1.0, worst


def _t4_to_nchw(x):
    return x.cpu().permute(0, 3, 1, 2).contiguous()


@gpu
@pytest.mark.parametrize("name", BACKWARD)
def test_backward_feature_map_gradients(name):
    """Part C: gfeats_t4 accumulated onto prefilled maps (every other texel starts at zero), texel by texel; texels no sample
    reaches keep their bits."""
    c, rs, d = case(name), reference_sums(name, N_PTS), dev()
    ds, raw = dev_scene(CASES[name][0]), dev_weights(name, "raw")
    g = torch.Generator().manual_seed(35)
    prior = []
    for f in ds.feats_t4:
        p = torch.randn(f.shape, generator=g) * 0.5
        p.reshape(-1, 4)[::2] = 0.0
        prior.append(p)
    gf = [p.to(d).contiguous() for p in prior]
    n = int(rs.sel.numel())
    rows, dsb, color = bwd_buffers(n, c.scene.nv - 1)
    bwd_call(ds, raw, c.pts.to(d), rs.sel.to(torch.int32).to(d), n, c.gcolor.to(d), rows, dsb, color, gfeats=gf)
    got, pri = [_t4_to_nchw(x) for x in gf], [_t4_to_nchw(x) for x in prior]
    out, bad = judge_gfeats(got, pri, rs)
    plain = judge_gfeats(got, pri, rs, atomic_term=False)[0]
    print(f"[margin] gfeats {name} {max(out.values()):.3f} (8 E alone: {max(plain.values()):.3f})")
    assert not bad and max(out.values()) <= 1.0, (out, bad)


@gpu
@pytest.mark.parametrize("name,n", [(k, N_PTS) for k in BACKWARD] + [("v8", 601)])
def test_assembled_gradients(name, n):
    """Part D: ops.blend_backward (colgram at fp32 precision) against float64 autograd for every parameter; v8 with n = 601 has
    more than 4096 (sample, view) rows: colgram's matrix-pipe plan."""
    from surf_amd import ops
    c, rs, d = case(name), reference_sums(name, n), dev()
    ds = dev_scene(CASES[name][0])
    assert ops.colgram_precision == 0 and (n == N_PTS or rs.rows >= 4096)
    res = ops.blend_backward(c.pts.to(d), rs.sel.to(torch.int32).to(d), c.gcolor.to(d), ds.feats_t4, ds.imgs_t4, ds.cams,
                             dev_weights(name, "raw"))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in res.items()}
    out, plain = judge_sums(got, rs), judge_sums(got, rs, sum_term=False)
    k, kp = max(out, key=out.get), max(plain, key=plain.get)
    print(f"[margin] assembled {name} n = {n} {out[k]:.3f} ({k}) (8 E alone: {plain[kp]:.3f}, {kp})")
    assert out[k] <= 1.0, out


@gpu
def test_refusals():
    """Part E: the entry points refuse by status code (raised by the binding) nv of 1 and 9, n_level != 4, a level narrower than
    two texels, null pointers and n <= 0, and leave the buffers untouched; ops.blend refuses active_count with fp32 weights."""
    from surf_amd import _lib, ops
    name, d = "v3", dev()
    c, ds = case(name), dev_scene(CASES[name][0])
    pts, gcolor = c.pts.to(d), c.gcolor.to(d)
    null = ctypes.c_void_p(0)
    narrow = (ctypes.c_int * 8)(*(list(ds.hw)[:5] + [1] + list(ds.hw)[6:]))
    flat = (ctypes.c_int * 8)(*(list(ds.hw)[:2] + [1] + list(ds.hw)[3:]))
    hole = (ctypes.c_void_p * 4)(*([ds.fp[0], None] + list(ds.fp)[2:]))
    common = {"nv=1": dict(nv=1), "nv=9": dict(nv=9), "n=0": dict(n=0), "n<0": dict(n=-2), "narrow": dict(hw=narrow), "flat": dict(hw=flat),
              "pts": dict(pts=null), "feats": dict(fp=None), "hw": dict(hw=None), "imgs": dict(imgs=null), "intrs": dict(intrs=null),
              "w2c": dict(w2c=null), "c2w": dict(c2w=null), "weights": dict(w=null), "feats[1]": dict(fp=hole)}
    for kernel in KERNELS:
        over = dict(common, **{"n_level=3": dict(n_level=3), "n_level=5": dict(n_level=5), "color": dict(color=null)})
        if kernel != "f32":
            over["scratch"] = dict(scratch=null)
        color, nvalid = fwd_buffers(c.n)
        scratch = _scratch_for(c.n, 8)
        for what, o in over.items():
            with pytest.raises(_lib.SurfHipError):
                fwd_call(kernel, ds, dev_weights(name, kernel), pts, c.n, color, nvalid, scratch=scratch, over=o)
        if kernel != "f32":
            idx = torch.arange(c.n, dtype=torch.int32, device=d)
            cnt = torch.tensor([5], dtype=torch.int32, device=d)
            for o in (dict(idx=null), dict(d_n=null)):
                with pytest.raises(_lib.SurfHipError):
                    fwd_call(kernel, ds, dev_weights(name, kernel), pts, c.n, color, nvalid, idx=idx, d_n=cnt, scratch=scratch, over=o)
        assert bool(torch.isnan(color).all()) and bool((nvalid == NV_SENTINEL).all())
    rows, dsb, color = bwd_buffers(c.n, c.scene.nv - 1)
    gf = [torch.zeros_like(f) for f in ds.feats_t4]
    over = dict(common, **{"gcolor": dict(gcolor=null), "rows": dict(rows=null), "ds": dict(ds=null),
                           "gfeats[1]": dict(gfeats=(ctypes.c_void_p * 4)(*([gf[0].data_ptr(), None] + [g.data_ptr() for g in gf[2:]])))})
    for what, o in over.items():
        with pytest.raises(_lib.SurfHipError):
            bwd_call(ds, dev_weights(name, "raw"), pts, None, c.n, gcolor, rows, dsb, color, gfeats=gf, over=o)
    assert all(bool(torch.isnan(b).all()) for b in (rows, dsb, color)) and all(float(g.abs().max()) == 0 for g in gf)
    with pytest.raises(ValueError):
        ops.blend(pts, ds.feats_t4, ds.imgs_t4, ds.cams, dev_weights(name, "f32"), active_idx=torch.arange(c.n, dtype=torch.int32, device=d),
                  active_count=torch.tensor([c.n], dtype=torch.int32, device=d))
