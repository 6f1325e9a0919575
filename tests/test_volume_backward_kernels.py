"""The backward kernels of the volume build, each fed directly at ragged shapes: surf_costvol_backward, surf_densify_backward,
surf_scatter_rows_add (csrc/volume.hip) and surf_matching_depth_backward (csrc/matching.hip).

Part A (no GPU): closed-form float64 restatements of the three backwards in scatter form (index_add_), pinned to float64 autograd
through back_proj_ref, matching_ref and O.sparse2dense of tests/test_volume_forward.py; their fp32 twins; the conditions every
input set of parts B-E has to meet; planted faults the comparator has to reject.  Parts B-E (gpu): the kernels against the
restatements.

How a gradient is compared.  Every element e of a gradient is a sum of terms (one per (voxel, view, level, tap) for a feature
texel, one per (voxel, view) for an agg_mlp number, one per (ray, sample, corner) for a matching-volume cell).  The restatement
run with the absolute value of every factor and every subtraction turned into an addition gives A_e, the un-cancelled sum of the
terms that land on e, and T_e, their number.  The bar of parts C and D is per element

    |gpu_e - g64_e|  <=  4 r32 A_e  (+ T_e 2^-41 gmax for the binned cost-volume form: its fixed-point unit is <= 2^-40 gmax)

with r32 = max_e |g32_e - g64_e| / A_e of the fp32 twin of the SAME restatement on the same inputs (the oracle's arithmetic): never
the tensor's maximum, never the element's own value (d agg_mlp.2.bias is analytically zero - softmax shift invariance), never
anything the kernel produced.  gmax = the largest |d feature| of the float64 restatement.

Taps outside the LDS image of costvol_tile_kernel (origin ox = max(floor(16 tx (W_l - 1) / (W_3 - 1)) - 1, 0), edge CVT_E[l] =
(16 >> (3 - l)) + 4): 0 of every regular pyramid used here (cases 0-5; test_costvol_inputs_meet_their_conditions counts them).
It is zero for EVERY regular pyramid: (W_l - 1) / (W_3 - 1) <= 2^-(3 - l), so a tile's records span at most 16 >> (3 - l) texels of
level l past floor(16 tx rx), the second tap one more, the margin one before: local x in [0, (16 >> (3 - l)) + 2].  The branch is
dead code for the shapes cv_binned_ok lets through.

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest); r32 per case and tensor kind:
    costvol_0_feat         r32 = 6.195e-06
    costvol_0_agg          r32 = 0.000e+00
    costvol_0_sum          r32 = 7.541e-10
    costvol_1_feat         r32 = 8.696e-06
    costvol_1_agg          r32 = 3.932e-09
    costvol_1_sum          r32 = 4.206e-09
    costvol_2_feat         r32 = 1.755e-04
    costvol_2_agg          r32 = 1.924e-08
    costvol_2_sum          r32 = 3.162e-09
    costvol_3_feat         r32 = 1.376e-06
    costvol_3_agg          r32 = 5.457e-09
    costvol_3_sum          r32 = 1.064e-09
    costvol_4_feat         r32 = 8.237e-05
    costvol_4_agg          r32 = 1.117e-08
    costvol_4_sum          r32 = 6.792e-09
    costvol_5_feat         r32 = 6.750e-05
    costvol_5_agg          r32 = 1.894e-08
    costvol_5_sum          r32 = 5.128e-09
    costvol_6a_feat        r32 = 2.238e-04
    costvol_6a_agg         r32 = 4.788e-09
    costvol_6a_sum         r32 = 7.423e-09
    costvol_6b_feat        r32 = 1.536e-04
    costvol_6b_agg         r32 = 9.063e-09
    costvol_6b_sum         r32 = 1.614e-08
    costvol_6c_feat        r32 = 1.546e-05
    costvol_6c_agg         r32 = 0.000e+00
    costvol_6c_sum         r32 = 1.562e-08
    costvol_7_feat         r32 = 2.761e-01
    costvol_7_agg          r32 = 3.791e-06
    costvol_7_sum          r32 = 8.354e-06
    matching_0             r32 = 2.169e-06
    matching_1             r32 = 1.760e-05
    matching_2             r32 = 6.074e-06
    matching_3             r32 = 5.942e-05
    matching_4             r32 = 2.276e-06
    matching_5             r32 = 1.951e-05
    matching_6             r32 = 4.238e-06
    matching_odd           r32 = 1.419e-05
    matching_overflow      r32 = 6.516e-03
    upsample_0             r32 = 2.733e-06
    upsample_1             r32 = 6.003e-07

What these numbers are.  The largest |g32 - g64| / A sits on an element that few taps of small weight feed: there an error of a
POSITION (a few fp32 ulp of a pixel or voxel coordinate) is a large share of A_e, whatever the summation does.  Most of it comes
from the inverse camera matrices, which twin and kernels take rounded to fp32 and the float64 reference does not round: the
kernels' own largest err / A, printed by the GPU tests (-s), equals r32 to two or three digits (err / bar 0.25).  r32 is a maximum over
elements and one outlier sets it.  costvol_7_feat (rows of 16,400 pixels: one fp32 ulp of a position is 1e-3 pixels) is 0.28: that
per-texel bar, 1.1 A_e, is wider than any value on a texel with terms and rejects nothing there - a zero or a doubled gradient
passes it.  What discriminates in case 7, and tightens every other case, are the `sum` lines: the gradient of a level summed over
its texels, per view and channel, does not depend on the last bits of a position (bilinear weights add up to 1; cv_bars), and a
lost, doubled or skipped share moves it by far more than its r32 of 8e-10 ... 8e-6.  test_sensitivity_costvol runs every planted
fault on cases 1, 2, 3, 5, 6a and 7.  matching_overflow carries 6.5e-3: its bar catches a lost or misplaced term (the MB_SLOTS
fault), not a rounding-level one.  The agg_mlp sums (thousands of terms each) have r32 of 4e-9 ... 4e-6.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import surf_oracle as O
from tests.test_volume_forward import (F32, F64, LEVELS_C2F, MATCH_CASES, _bilinear, _unnorm_ac, _world, back_proj_ref, band_included,
                                       decide, dev, eps_costvol, gpu, make_agg, make_cameras, make_pyramid, match_case, matching_ref,
                                       smooth_volume)
from tests.test_volume_forward import _ndc, _recorded as forward_recorded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
SENTINEL = 7.25e11
GUARD = 256


def _mb_slots():
    """MB_SLOTS of csrc/matching.hip, from the default of SURF_MB_SLOT_BITS (read the way _lib.py reads the ABI number)."""
    with open(os.path.join(ROOT, "surf_amd", "csrc", "matching.hip")) as f:
        return 1 << int(re.search(r"^#define\s+SURF_MB_SLOT_BITS\s+(\d+)", f.read(), re.M).group(1))


MB_SLOTS = _mb_slots()
MB_TX, MB_TY = 8, 4                                                 # the low-resolution patch of one workgroup


def worst(got, ref, bar):
    """Largest |got - ref| / bar over the elements (an element with bar 0 has to be met exactly)."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")                                          # a NaN or an infinity is outside every bar
    ratio = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def within(got, ref, bar):
    """THE comparator of parts B-D (and of the planted faults): every element inside its own bar."""
    return worst(got, ref, bar) <= 1.0


def rel_to_A(got, ref, A):
    """max_e |got - ref| / A_e over the elements with terms; where no term lands, got has to equal ref (= 0)."""
    err = (got.double() - ref).abs()
    assert not bool((err[A == 0] > 0).any()), "a non-zero value where the float64 restatement has no term"
    return float((err[A > 0] / A[A > 0]).max()) if bool((A > 0).any()) else 0.0


# ------------------------------------------------------------------------------------------------------------------
# A1. the restatements
# ------------------------------------------------------------------------------------------------------------------
# The same statements run at float64 (the reference) and at float32 (the twin, A2).  A gradient element that one tap of weight
# ~1e-5 feeds alone turns one ulp of its position into a large share of A_e, so r32 - a maximum over elements - follows the last
# bit of the position arithmetic: the twin is therefore written so that every host computes the same bits.  Products are added
# in index order (no BLAS), long sums are sequential fp32 additions (index_add_ onto one row), exp / expm1 / sqrt are evaluated in
# float64 and rounded once (the vectorised fp32 ones differ between CPUs), and a matrix inverse is a float64 inverse computed here in plain Python and rounded once - LAPACK's fp32
# inverse differs between CPUs by more than every other rounding here together.  The GPU tests hand the kernels these very
# inverses (gpu_cameras).  Random inputs are drawn in float64 and rounded once for the same reason.


def _inv(M, dt):
    """Inverse of (..., k, k) matrices by Gauss-Jordan elimination with partial pivoting on Python floats (IEEE double operations in
    a fixed order: no LAPACK), rounded to dt once."""
    if M.dim() > 2:
        return torch.stack([_inv(m, dt) for m in M])
    k = M.shape[0]
    a = [[float(x) for x in row] + [1.0 if i == j else 0.0 for j in range(k)] for i, row in enumerate(M.to(F64).tolist())]
    for col in range(k):
        piv = max(range(col, k), key=lambda r: abs(a[r][col]))
        a[col], a[piv] = a[piv], a[col]
        d = a[col][col]
        a[col] = [x / d for x in a[col]]
        for r in range(k):
            if r != col and a[r][col] != 0.0:
                f = a[r][col]
                a[r] = [x - f * y for x, y in zip(a[r], a[col])]
    return torch.tensor([row[k:] for row in a], dtype=F64).to(dt)


def _mv(x, M):
    """x (N,k) @ M (m,k)^T, the products of an output added in index order."""
    cols = []
    for j in range(M.shape[0]):
        acc = x[:, 0] * M[j, 0]
        for k in range(1, M.shape[1]):
            acc = acc + x[:, k] * M[j, k]
        cols.append(acc)
    return torch.stack(cols, dim=1)


def _via64(fn, x):
    return fn(x.to(F64)).to(x.dtype)


def _sum_last(x):
    """Sum over the last axis, added in index order."""
    acc = x[..., 0]
    for k in range(1, x.shape[-1]):
        acc = acc + x[..., k]
    return acc


def _sum_rows(x):
    """(N, k) -> (k,): the rows added one after the other."""
    return torch.zeros(1, x.shape[1], dtype=x.dtype).index_add_(0, torch.zeros(x.shape[0], dtype=torch.long), x)[0]


def _softmax_last(x):
    e = _via64(torch.exp, x - x.max(dim=-1, keepdim=True).values)
    return e / _sum_last(e)[..., None]


def ndc(world, intr, c2w, h, w, dt, w2c=None):
    """_ndc of the forward file, written out (module comment above).  w2c: an inverse of c2w to use as it is."""
    hom = torch.cat([world, torch.ones_like(world[:, :1])], dim=1)
    q = _mv(_mv(hom, _inv(c2w, dt) if w2c is None else w2c.to(dt)), intr.to(dt))
    x = q[:, 0] / q[:, 2]
    y = q[:, 1] / q[:, 2]
    return x / ((w - 1) / 2) - 1, y / ((h - 1) / 2) - 1, q[:, 2]



def costvol_bwd_ref(agg, feats, coords, D, intrs, c2ws, stage, G, dt=F64, absolute=False, fault=None, drop=None, w2c=None):
    """d loss / d (pyramid levels >= stage, 49 agg_mlp numbers w1 | b1 | w2 | b2) for upstream G (n,8) = [d mean | d var].
    absolute: every factor by its absolute value, every subtraction an addition -> A (and the term counts T).
    drop: (nv, n) bool, records whose feature gradient a planted fault loses.  w2c (nv,4,4): inverses of c2ws to use as they are.
    -> dict(gfeats [None | (nv,4,H,W)] * 4, g_agg (49,), T_feats, T_agg, df (nv,n,4), nx, ny (nv,n), inside (nv,n))."""
    nv, n = feats[-1].shape[0], coords.shape[0]
    h, w = feats[-1].shape[-2:]
    w1, b1, w2, b2 = (t.to(dt) for t in agg)
    world = _world(coords, D, dt)
    nxs, nys, ins, fs, pres = [], [], [], [], []
    for v in range(nv):
        nx, ny, qz = ndc(world, intrs[v], c2ws[v], h, w, dt, None if w2c is None else w2c[v])
        f = torch.zeros(n, 4, dtype=dt)
        for lvl in feats[stage:]:
            hh, ww = lvl.shape[-2:]
            f = f + _bilinear(lvl[v].to(dt), _unnorm_ac(nx, ww), _unnorm_ac(ny, hh))
        nxs.append(nx), nys.append(ny), ins.append((nx.abs() <= 1) & (ny.abs() <= 1) & (qz > 0)), fs.append(f)
        pres.append(_mv(f, w1) + b1)
    nx, ny, inside, f, pre = torch.stack(nxs), torch.stack(nys), torch.stack(ins), torch.stack(fs), torch.stack(pres)
    act = torch.where(pre > 0, pre, _via64(torch.expm1, pre))
    logit = _sum_last(act * w2[0]) + b2[0]
    p = _softmax_last(torch.where(inside, logit, torch.full_like(logit, -1e9)).t()).t()       # (nv, n)
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    sg = 1.0 if absolute else -1.0
    fa, gm, gv = ab(f), ab(G[:, :4].to(dt)), ab(G[:, 4:].to(dt))
    wf = fa * p[..., None]
    mean = _sum_last(wf.permute(1, 2, 0))
    dwf = gm[None] + 2.0 * gv[None] * (wf if fault == "var_no_mean" else wf + sg * mean[None])  # d loss / d (weighted feature)
    dw = _sum_last(dwf * fa)
    dot = _sum_last((p * dw).t())
    ds = p * (dw if fault == "softmax_no_dot" else dw + sg * dot[None])                          # d loss / d logit
    if fault != "ds_unmasked":
        ds = torch.where(inside, ds, torch.zeros_like(ds))
    dact = torch.ones_like(pre) if fault == "elu_one" else torch.where(pre > 0, torch.ones_like(pre), _via64(torch.exp, pre))
    dh = ds[..., None] * ab(w2[0])[None, None] * dact                                            # (nv, n, 8)
    df = dwf * p[..., None] + _mv(dh.reshape(-1, 8), ab(w1).t()).reshape(nv, n, 4)               # (nv, n, 4)
    if fault == "tail256":
        dead = torch.arange(n) >= n - n % 256
        df, dh, ds = df * ~dead[None, :, None], dh * ~dead[None, :, None], ds * ~dead[None]
    if drop is not None:
        df = df * ~drop[..., None]
    g_agg = torch.cat([_sum_rows((dh[..., None] * fa[:, :, None, :]).reshape(nv * n, 32)), _sum_rows(dh.reshape(nv * n, 8)),
                       _sum_rows((ds[..., None] * ab(act)).reshape(nv * n, 8)), _sum_rows(ds.reshape(nv * n, 1))])
    nz = lambda t: (t != 0).to(dt)
    T_agg = torch.cat([nz(dh[..., None] * fa[:, :, None, :]).sum((0, 1)).reshape(-1), nz(dh).sum((0, 1)), nz(ds[..., None] * act).sum((0, 1)),
                       nz(ds).sum().reshape(1)])
    gmax = float(df.abs().max())
    step = 2.0 ** (np.floor(np.log2(gmax)) + 1 - 20) if gmax > 0 else 1.0                        # fault "coarse": 2^-20 of the largest
    gfeats, T_feats = [None] * 4, [None] * 4
    for l in range(stage + 1 if fault == "skip_level" else stage, 4):
        H, W = feats[l].shape[-2:]
        out, cnt = torch.zeros(nv, 4, H * W, dtype=dt), torch.zeros(nv, 4, H * W, dtype=dt)
        for v in range(nv):
            x, y = _unnorm_ac(nx[v], W), _unnorm_ac(ny[v], H)
            x0, y0 = torch.floor(x), torch.floor(y)
            tx, ty = x - x0, y - y0
            x0, y0 = x0.long(), y0.long()
            for dy, wy in ((0, 1.0 - ty), (1, ty)):
                for dx, wx in ((0, 1.0 - tx), (1, tx)):
                    xi, yi = x0 + dx, y0 + dy
                    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                    term = torch.where(ok[:, None], df[v] * (wx * wy)[:, None], torch.zeros_like(df[v]))
                    if fault == "coarse":
                        term = torch.round(term / step) * step
                    idx = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
                    out[v].index_add_(1, idx, term.t().contiguous())
                    cnt[v].index_add_(1, idx, nz(term).t().contiguous())
        gfeats[l], T_feats[l] = out.reshape(nv, 4, H, W), cnt.reshape(nv, 4, H, W)
    if fault == "skip_level":
        gfeats[stage], T_feats[stage] = torch.zeros_like(feats[stage], dtype=dt), torch.zeros_like(feats[stage], dtype=dt)
    return dict(gfeats=gfeats, g_agg=g_agg, T_feats=T_feats, T_agg=T_agg, df=df, nx=nx, ny=ny, inside=inside, pre=pre, gmax=gmax)


def upsample_T(g_full, h, w, dt=F64):
    """Transpose of F.interpolate((nv,h,w) -> (H,W), bilinear, align_corners=False): (nv,H,W) -> (nv,h,w)."""
    nv, H, W = g_full.shape
    g = g_full.to(dt)

    def axis(size_out, size_in):
        src = ((torch.arange(size_out, dtype=dt) + 0.5) * torch.tensor(size_in / size_out if dt == F64 else np.float32(size_in) / np.float32(size_out), dtype=dt)
               - 0.5).clamp(min=0)
        i0 = src.floor().long()
        return i0, (i0 + 1).clamp(max=size_in - 1), src - i0.to(dt)
    y0, y1, ly = axis(H, h)
    x0, x1, lx = axis(W, w)
    out = torch.zeros(nv, h * w, dtype=dt)
    for yi, wy in ((y0, 1.0 - ly), (y1, ly)):
        for xi, wx in ((x0, 1.0 - lx), (x1, lx)):
            idx = (yi[:, None] * w + xi[None, :]).reshape(-1)
            out.index_add_(1, idx, (g * (wy[:, None] * wx[None, :])[None]).reshape(nv, -1))
    return out.reshape(nv, h, w)


def match_rays(c, v, dt, jitter=None):
    """The samples of view v's low-resolution rays: z (R,S), cos z (R,), the eight taps of every sample - flat offsets, weights,
    in-lattice flags, each (R,S,8).  The bands are constants (they come from detached depths)."""
    H, W, L, n, Dv = c["H"], c["W"], c["L"], c["n"], c["D"]
    h, w = H // L, W // L
    py, px = torch.meshgrid(torch.linspace(0, H - 1, h), torch.linspace(0, W - 1, w), indexing="ij")
    px, py = px.reshape(-1), py.reshape(-1)
    lin = torch.linspace(0.0, 1.0, int(n), dtype=F32).to(dt)
    pix = torch.stack([px, py, torch.ones_like(px)], dim=-1).to(dt)
    camd = _mv(pix, _inv(c["intrs"][v], dt)[:3, :3])
    R = c["c2ws"][v, :3, :3].to(dt)
    rd = _mv(camd / _via64(torch.sqrt, _sum_last(camd * camd))[:, None], R)
    ro = c["c2ws"][v, :3, 3].to(dt)
    n0, f0 = c["near_fars"][v, 0].to(dt), c["near_fars"][v, 1].to(dt)
    cz = _mv(rd, _inv(c["c2ws"][v, :3, :3], dt))[:, 2]
    jit = None if jitter is None else jitter[v].to(dt)
    if c["pre"] is None:
        z = n0 + (f0 - n0) * lin[None, :].expand(px.shape[0], -1)
        if jit is not None:
            z = z + jit[:, 0:1] * (f0 - n0) / n
    else:
        zc = (c["pre"][v].to(dt)[py.long(), px.long()] / cz)[:, None]
        zs = []
        for k, r in enumerate((c["rc"], c["rp"])):
            half = ((f0 - n0) * r) / 2
            a, b = zc - half, zc + half
            a = torch.where(b > f0, a - (b - f0), a)
            b = torch.where(a < n0, b + (n0 - a), b)
            a, b = torch.clamp(a, n0, f0), torch.clamp(b, n0, f0)
            zs.append(a + (b - a) * lin[None, :] + (0.0 if jit is None else jit[:, k:k + 1] * (b - a) / n))
        z = torch.cat(zs, dim=-1)
    g = ((ro[None, None, :] + rd[:, None, :] * z[..., None] + 1.0) * Dv - 1.0) / 2.0              # (R,S,3)
    g0 = torch.floor(g)
    t = g - g0
    g0 = g0.long()
    offs, wgts, oks = [], [], []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cc = g0 + torch.tensor([dx, dy, dz])
                oks.append(((cc >= 0) & (cc < Dv)).all(dim=-1))
                cc = cc.clamp(0, Dv - 1)
                offs.append((cc[..., 0] * Dv + cc[..., 1]) * Dv + cc[..., 2])
                wgts.append((t[..., 0] if dx else 1.0 - t[..., 0]) * (t[..., 1] if dy else 1.0 - t[..., 1]) * (t[..., 2] if dz else 1.0 - t[..., 2]))
    return z, cz, torch.stack(offs, -1), torch.stack(wgts, -1), torch.stack(oks, -1)


def selected_views(views, nv, fault=None):
    v0, v1 = views
    sel = [v0] + ([v1] if v1 >= 0 and v1 != v0 else [])
    if fault == "second_view_dropped":
        sel = sel[:1]
    if fault == "other_view_not_ignored":
        sel = sel + [next(v for v in range(nv) if v not in sel)]
    return sel


def patch_of_rays(h, w):
    """Patch number (8 x 4 low-resolution pixels, one workgroup) of every ray of a view, (h*w,)."""
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return ((ys // MB_TY) * ((w + MB_TX - 1) // MB_TX) + xs // MB_TX).reshape(-1)


def match_bwd_ref(c, g_full, views, jitter=None, dt=F64, absolute=False, fault=None):
    """d loss / d matching volume (D,D,D) for upstream g_full (nv,H,W): the maps of the selected views only, through the
    transposed bilinear upsample; depth = cos z sum_k z_k softmax(rho)_k with the z_k constants:
    d rho_k = g cos z p_k (z_k - E).  -> (dmvol, T)."""
    Dv, n = c["D"], c["n"]
    h, w = c["H"] // c["L"], c["W"] // c["L"]
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    g_lr = upsample_T(ab(g_full), h, w, dt).reshape(c["nv"], -1)
    vol = c["mvol"].to(dt).reshape(-1)
    dm, T = torch.zeros(Dv ** 3, dtype=dt), torch.zeros(Dv ** 3, dtype=dt)
    jit = jitter
    if fault == "jitter_first_band_only" and jitter is not None:
        jit = jitter.clone()
        jit[..., 1] = 0
    for v in selected_views(views, c["nv"], fault):
        z, cz, off, wgt, ok = match_rays(c, v, dt, jit)
        rho = _sum_last(torch.where(ok, vol[off] * wgt, torch.zeros_like(wgt)))
        p = _softmax_last(rho)
        E = _sum_last(p * z)[:, None]
        if fault == "E_band0":
            E = (_sum_last(p[:, :n] * z[:, :n]) / _sum_last(p[:, :n]))[:, None]
        coef = g_lr[v] * (1.0 if fault == "no_cosz" else ab(cz))
        drho = coef[:, None] * p * ((z.abs() + E.abs()) if absolute else (z - E))
        term = torch.where(ok, drho[..., None] * wgt, torch.zeros_like(wgt))                     # (R,S,8)
        if fault == "slots":        # per patch, only the first MB_SLOTS distinct z-pair keys (in ray, sample, corner order) are kept
            patch = patch_of_rays(h, w)
            for pid in patch.unique():
                rays = (patch == pid).nonzero().view(-1)
                keys = (off[rays] >> 1).reshape(-1).numpy()
                live = (ok[rays] & (term[rays] != 0)).reshape(-1).numpy()
                uniq, first = np.unique(keys[live], return_index=True)
                late = set(uniq[np.argsort(first)][MB_SLOTS:].tolist())
                lost = torch.from_numpy(np.isin(keys, list(late)) & live).reshape(term[rays].shape)
                term[rays] = torch.where(lost, torch.zeros_like(term[rays]), term[rays])
        dm.index_add_(0, off.reshape(-1), term.reshape(-1))
        T.index_add_(0, off.reshape(-1), (term != 0).to(dt).reshape(-1))
    return dm.reshape(Dv, Dv, Dv), T.reshape(Dv, Dv, Dv)


def keys_per_patch(c, views, jitter=None):
    """Distinct z-pair keys `off >> 1` a workgroup (8 x 4 patch, one view) sends to its LDS table, from float64."""
    h, w = c["H"] // c["L"], c["W"] // c["L"]
    patch = patch_of_rays(h, w)
    out = []
    for v in selected_views(views, c["nv"]):
        _, _, off, wgt, ok = match_rays(c, v, F64, jitter)
        for pid in patch.unique():
            rays = patch == pid
            out.append(int(torch.unique((off[rays] >> 1)[ok[rays] & (wgt[rays] != 0)]).numel()))
    return out


def up2_axis(D, fault=None):
    """Along one axis, fine voxel i of the x2 trilinear upsample (align_corners=False) reads coarse cells i0, i1 with 1 - l1, l1."""
    Dp = D // 2
    src = ((torch.arange(D, dtype=F64) + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = src.floor().long()
    i1 = (i0 + 1).clamp(max=Dp - 1)
    l1 = src - i0.to(F64)
    l0 = 1.0 - l1
    if fault == "ends_075":
        l0[0], l0[D - 1], l1[D - 1] = 0.75, 0.75, 0.0
    return i0, i1, l0, l1


def densify_bwd_ref(coords, g_dense, D, with_prev, dt=F64, absolute=False, fault=None):
    """-> (d rows (n,8): the dense gradient of the scattered sites in column 0, g_prev (D/2)^3 or None: the background voxels'
    gradient through the transposed x2 trilinear upsample, T of g_prev)."""
    c = coords.long()
    g = g_dense.to(dt).abs() if absolute else g_dense.to(dt)
    rows = torch.zeros(c.shape[0], 8, dtype=dt)
    rows[:, 0] = g[c[:, 0], c[:, 1], c[:, 2]]
    if fault == "all_columns":
        rows[:] = rows[:, 0:1]
    if not with_prev:
        return rows, None, None
    Dp = D // 2
    bg = torch.ones(D, D, D, dtype=torch.bool)
    if fault != "mask_ignored":
        bg[c[:, 0], c[:, 1], c[:, 2]] = False
    gb = torch.where(bg, g, torch.zeros_like(g))
    i0, i1, l0, l1 = up2_axis(D, fault)
    out, T = torch.zeros(Dp ** 3, dtype=dt), torch.zeros(Dp ** 3, dtype=dt)
    for xi, wx in ((i0, l0), (i1, l1)):
        for yi, wy in ((i0, l0), (i1, l1)):
            for zi, wz in ((i0, l0), (i1, l1)):
                idx = ((xi[:, None, None] * Dp + yi[None, :, None]) * Dp + zi[None, None, :]).reshape(-1)
                term = (gb * (wx[:, None, None] * wy[None, :, None] * wz[None, None, :]).to(dt)).reshape(-1)
                out.index_add_(0, idx, term)
                T.index_add_(0, idx, (term != 0).to(dt))
    return rows, out.reshape(Dp, Dp, Dp), T.reshape(Dp, Dp, Dp)


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------

# 1.5 x the forward file's EPS_COSTVOL as recorded there: eps_costvol() itself is measured from the host's fp32 LAPACK / BLAS
# arithmetic (4.0e-05 and 4.4e-05 on two hosts), and the list of voxels - hence every number below - has to be the same on every
# host; test_costvol_inputs_meet_their_conditions checks that the host's own value is covered
EPS_REMOVE = 1.5 * forward_recorded("EPS_COSTVOL")
REG_16_24 = ((2, 3), (4, 6), (8, 12), (16, 24))
REG_37_53 = ((4, 6), (9, 13), (18, 26), (37, 53))
REG_WIDE = ((4, 2050), (8, 4100), (16, 8200), (32, 16400))
CVT, CVT_E, CVT_MAX_BUCKETS = 16, (6, 8, 12, 20), 16384

#  name: D, voxels (None: the full lattice), pyramid, nv, stage, what the dispatch has to give: (binned, split) or the reason for direct
CV_CASES = {
    "0": (9, None, REG_16_24, 1, 0, (True, 1)),                    # nv = 1: g_agg exactly zero, d f = gm
    "1": (13, None, REG_16_24, 2, 0, (True, 2)),
    "2": (21, None, REG_16_24, 3, 1, (True, 4)),
    "3": (33, None, REG_16_24, 2, 2, (True, 8)),
    "4": (14, None, REG_16_24, 8, 3, (True, 2)),
    "5": (24, None, REG_37_53, 5, 0, (True, 2)),
    "6a": (10, 700, LEVELS_C2F, 2, 1, "irregular"),
    "6b": (10, 257, LEVELS_C2F, 2, 1, "irregular"),
    "6c": (10, 1, LEVELS_C2F, 2, 1, "irregular"),
    "7": (10, 500, REG_WIDE, 8, 3, "buckets"),
}


def cv_dispatch(n, nv, levels):
    """cv_binned_ok and the split rule of surf_costvol_backward, restated: (binned, split) or the reason for the direct scatter."""
    H3, W3 = levels[3]
    for l in range(4):
        if tuple(levels[l]) != (H3 >> (3 - l), W3 >> (3 - l)) or min(levels[l]) < 2:
            return "irregular"
    nb = nv * ((W3 + CVT - 1) // CVT) * ((H3 + CVT - 1) // CVT)
    if nb > CVT_MAX_BUCKETS or n * nv > 0x7fffffff:
        return "buckets"
    avg = n * nv // nb
    return True, (8 if avg > 16384 else 4 if avg > 4096 else 2 if avg > 1024 else 1)


def cv_buckets(r, levels):
    """The (view, tile) bucket of every record (nv, n), -1 for records the kernel does not list (d feature all zero)."""
    H3, W3 = levels[3]
    ntx, nty = (W3 + CVT - 1) // CVT, (H3 + CVT - 1) // CVT
    x0 = torch.floor(_unnorm_ac(r["nx"], W3)).clamp(0, W3 - 1).long()
    y0 = torch.floor(_unnorm_ac(r["ny"], H3)).clamp(0, H3 - 1).long()
    b = (torch.arange(r["nx"].shape[0])[:, None] * nty + y0 // CVT) * ntx + x0 // CVT
    return torch.where((r["df"] != 0).any(-1), b, torch.full_like(b, -1))


def cv_taps_outside_lds(r, levels, stage):
    """Valid taps of listed records that fall outside the tile kernel's LDS image (restated from its ox, oy, CVT_E)."""
    H3, W3 = levels[3]
    ntx = (W3 + CVT - 1) // CVT
    b = cv_buckets(r, levels)
    listed = b >= 0
    tile = b.clamp(min=0) % (ntx * ((H3 + CVT - 1) // CVT))
    ty, tx = (tile // ntx).numpy(), (tile % ntx).numpy()
    total = 0
    for l in range(stage, 4):
        H, W = levels[l]
        rx, ry = np.float32(W - 1) / np.float32(W3 - 1), np.float32(H - 1) / np.float32(H3 - 1)
        ox = np.maximum(np.floor((tx * CVT).astype(np.float32) * rx).astype(np.int64) - 1, 0)
        oy = np.maximum(np.floor((ty * CVT).astype(np.float32) * ry).astype(np.int64) - 1, 0)
        x0 = torch.floor(_unnorm_ac(r["nx"], W)).long().numpy()
        y0 = torch.floor(_unnorm_ac(r["ny"], H)).long().numpy()
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi = x0 + dx, y0 + dy
                valid = listed.numpy() & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                lx, ly = xi - ox, yi - oy
                total += int((valid & ((lx < 0) | (lx >= CVT_E[l]) | (ly < 0) | (ly >= CVT_E[l]))).sum())
    return total


@functools.lru_cache(maxsize=None)
def cv_case(name):
    D, n_list, levels, nv, stage, expect = CV_CASES[name]
    seed = 300 + sorted(CV_CASES).index(name)
    H, W = levels[3]
    intrs, c2ws, _ = make_cameras(nv, H, W, exact_first=False, per_axis_focal=levels is REG_WIDE)
    feats = make_pyramid(nv, seed, levels, F64)                    # every random input: float64, rounded to fp32 once
    agg = make_agg(seed + 50, F64)
    g = torch.Generator().manual_seed(seed + 100)
    coords = O.init_coords(D).long()
    if n_list is not None:                                          # a list in no particular order, drawn before the removal below
        coords = coords[torch.randperm(coords.shape[0], generator=g)[:n_list + 8]]
    # voxels with a frustum term within EPS_COSTVOL of its threshold leave the list (the backward takes any list)
    world = _world(coords, D, F64)
    t64 = torch.stack([torch.stack(ndc(world, intrs[v], c2ws[v], H, W, F64)) for v in range(nv)], dim=1)       # (3, nv, N)
    _, _, unc = decide(t64, EPS_REMOVE)
    n_unc = int(unc.sum())
    coords = coords[~unc]
    if n_list is not None:
        coords = coords[:n_list]
    coords = coords.contiguous()
    n = coords.shape[0]
    G = (torch.randn(n, 8, generator=g, dtype=F64) * 10.0 ** (-3.0 * torch.rand(n, 1, generator=g, dtype=F64))).to(F32)   # rows over three decades
    kw = dict(agg=agg, feats=feats, coords=coords, D=D, intrs=intrs, c2ws=c2ws, stage=stage, G=G)
    r64 = costvol_bwd_ref(**kw)
    rA = costvol_bwd_ref(**kw, absolute=True)
    r32 = costvol_bwd_ref(**kw, dt=F32)
    feat_r32 = max(rel_to_A(r32["gfeats"][l], r64["gfeats"][l], rA["gfeats"][l]) for l in range(stage, 4))
    agg_r32 = rel_to_A(r32["g_agg"], r64["g_agg"], rA["g_agg"])
    sum_r32 = max(rel_to_A(r32["gfeats"][l].sum((2, 3)), r64["gfeats"][l].sum((2, 3)), rA["gfeats"][l].sum((2, 3))) for l in range(stage, 4))
    return dict(name=name, D=D, nv=nv, stage=stage, levels=levels, expect=expect, n_unc=n_unc, n_full=n + n_unc, n=n, G=G, kw=kw,
                r64=r64, A=rA, r32=dict(feat=feat_r32, agg=agg_r32, sum=sum_r32), dispatch=cv_dispatch(n, nv, levels))


def cv_bars(c, binned):
    """Bars of case c: (feature levels [None | per texel] * 4, agg, sums [None | (nv,4)] * 4).
    The sums: bilinear weights add up to 1, so the sum of a level's gradient over its texels, per view and channel, is the sum of
    d feature over the records (less the taps outside the image) WHATEVER the last bits of the positions are.  It is one more
    element of the gradient - terms: all of the level's, A and T their sums - under the same rule, with its own r32: the check that
    a lost, doubled or misplaced share cannot pass where single ill-conditioned taps make the per-texel r32 large (case 7)."""
    extra = (2.0 ** -41 * c["r64"]["gmax"]) if binned else 0.0
    A, T = c["A"]["gfeats"], c["A"]["T_feats"]
    feats = [None if l < c["stage"] else 4.0 * c["r32"]["feat"] * A[l] + extra * T[l] for l in range(4)]
    sums = [None if l < c["stage"] else 4.0 * c["r32"]["sum"] * A[l].sum((2, 3)) + extra * T[l].sum((2, 3)) for l in range(4)]
    return feats, 4.0 * c["r32"]["agg"] * c["A"]["g_agg"], sums


#               D  (H, W)  res_level nv  n   what
NEW_MATCH = {"odd": (9, (16, 24), 1, 2, 16), "overflow": (48, (16, 24), 2, 2, 64)}
MATCH_NAMES = [str(i) for i in range(len(MATCH_CASES))] + sorted(NEW_MATCH)


@functools.lru_cache(maxsize=None)
def mb_case(name):
    """A matching case with its upstream maps (non-zero on EVERY view), jitter (both columns filled) and per-configuration
    references: ref[(two views?, jitter?)] = (g64, A, T, r32)."""
    if name in NEW_MATCH:
        D, (H, W), L, nv, n = NEW_MATCH[name]
        intrs, c2ws, near_fars = make_cameras(nv, H, W)
        c = dict(D=D, H=H, W=W, L=L, nv=nv, n=n, pre=None, rc=1.0, rp=1.0, intrs=intrs, c2ws=c2ws, near_fars=near_fars,
                 mvol=smooth_volume(D), arg64=None)
    else:
        c = dict(match_case(int(name)))
    nv, H, W, L = c["nv"], c["H"], c["W"], c["L"]
    h, w = H // L, W // L
    g = torch.Generator().manual_seed(500 + MATCH_NAMES.index(name))
    g_full = torch.randn(nv, H, W, generator=g, dtype=F64) * 10.0 ** (-2.0 * torch.rand(nv, H, W, generator=g, dtype=F64))
    _, full_ok = band_included(c)
    g_full = torch.where(full_ok, g_full, torch.zeros_like(g_full)).to(F32).contiguous()     # pixels next to a band clamp carry none
    jitter = (torch.rand(nv, h * w, 2, generator=g, dtype=F64) - 0.5).to(F32).contiguous()
    src = nv - 1
    c.update(name=name, g_full=g_full, jitter=jitter, src=src, excluded=float((~full_ok).double().mean()))
    ref = {}
    for two in ((False, True) if nv > 1 else (False,)):
        views = (0, src) if two else (0, 0)
        for jit in (False, True):
            j = jitter if jit else None
            g64, T = match_bwd_ref(c, g_full, views, j)
            A, _ = match_bwd_ref(c, g_full, views, j, absolute=True)
            g32, _ = match_bwd_ref(c, g_full, views, j, dt=F32)
            ref[(two, jit)] = (g64, A, T, rel_to_A(g32, g64, A))
    c["ref"] = ref
    c["r32"] = max(r[3] for r in ref.values())
    return c


UPSAMPLE_CASES = (((37, 53), (18, 26)), ((37, 53), (9, 13)))


@functools.lru_cache(maxsize=None)
def up_case(i):
    (H, W), (h, w) = UPSAMPLE_CASES[i]
    g = torch.Generator().manual_seed(700 + i)
    g_full = (torch.randn(3, H, W, generator=g, dtype=F64) * 10.0 ** (-2.0 * torch.rand(3, H, W, generator=g, dtype=F64))).to(F32)
    g64, A, g32 = upsample_T(g_full, h, w), upsample_T(g_full.abs(), h, w), upsample_T(g_full, h, w, F32)
    return dict(H=H, W=W, h=h, w=w, g_full=g_full, g64=g64, A=A, r32=rel_to_A(g32, g64, A))


DENSIFY_D = (2, 4, 6, 10, 34, 70)


@functools.lru_cache(maxsize=None)
def dn_case(D):
    g = torch.Generator().manual_seed(800 + D)
    occ = torch.rand(D, D, D, generator=g) < 0.3
    occ[0, 0, 0], occ[D - 1, D - 1, D - 1], occ[0, D - 1, 0] = True, False, True        # a scattered corner, a background corner
    if D > 2:
        occ[0, 1, 1], occ[D - 1, 1, D - 2] = True, False                                  # ... and faces of both kinds
    coords = occ.nonzero()
    coords = coords[torch.randperm(coords.shape[0], generator=g)].to(torch.int32).contiguous()
    g_dense = (torch.randn(D, D, D, generator=g, dtype=F64) * 10.0 ** (-2.0 * torch.rand(D, D, D, generator=g, dtype=F64))).to(F32).contiguous()
    rows64, prev64, T = densify_bwd_ref(coords, g_dense, D, True)
    _, A, _ = densify_bwd_ref(coords, g_dense, D, True, absolute=True)
    return dict(D=D, occ=occ, coords=coords, g_dense=g_dense, rows64=rows64, prev64=prev64, A=A, T=T)


def dn_bar(c, base=None):
    """Dyadic weights: a term rounds at most three times (g wx wy wz, fp32), at most 63 additions follow: 66 2^-24 A_e; adding into a
    non-zero g_prev rounds once more, at the size of |base| + A_e."""
    bar = 66.0 * U24 * c["A"]
    return bar if base is None else bar + U24 * (base.double().abs() + c["A"])


# ------------------------------------------------------------------------------------------------------------------
# A. references, conditions, planted faults (no GPU)
# ------------------------------------------------------------------------------------------------------------------


def _agg_grads(agg_leaf):
    return torch.cat([t.grad.reshape(-1) for t in agg_leaf])


@pytest.mark.parametrize("name", list(CV_CASES))
def test_costvol_restatement_matches_float64_autograd(name):
    c = cv_case(name)
    kw = c["kw"]
    feats = [f.to(F64).requires_grad_(l >= c["stage"]) for l, f in enumerate(kw["feats"])]
    agg = [t.to(F64).requires_grad_(True) for t in kw["agg"]]
    # the forward file's own projection, except on the 16,400-pixel rows of case 7: there two float64 routes to a position - LAPACK and
    # BLAS or the written-out sums - differ by 1e-12 pixels, 1e-8 of a tap weight of 1e-4, and the pin is about the backward
    # (test_projection_matches_the_forward_file pins the projection itself in every case)
    out, _, _ = back_proj_ref(agg, feats, kw["coords"], c["D"], kw["intrs"], kw["c2ws"], c["stage"], F64, ndc=ndc if name == "7" else None)
    (out * kw["G"].to(F64)).sum().backward()
    for l in range(c["stage"], 4):
        assert float(feats[l].grad.abs().max()) > 0 or c["n"] == 1
        assert within(c["r64"]["gfeats"][l], feats[l].grad, 1e-10 * c["A"]["gfeats"][l]), (name, l)
    assert within(c["r64"]["g_agg"], _agg_grads(agg), 1e-10 * c["A"]["g_agg"]), name
    # d agg_mlp.2.bias is analytically zero: its un-cancelled sum is what the bars are relative to
    assert abs(float(c["r64"]["g_agg"][48])) <= 1e-12 * float(c["A"]["g_agg"][48]) and float(c["A"]["g_agg"][48]) > 0 or c["nv"] == 1


@pytest.mark.parametrize("name", list(CV_CASES))
def test_projection_matches_the_forward_file(name):
    """ndc (plain-Python inverse, sums written out) against _ndc (LAPACK, BLAS) in float64: the homogeneous coordinates to 1e-10 of
    their un-cancelled sums, the normalised positions to 1e-10 (1 + |.|) wherever the voxel is not within 1e-3 of the camera plane."""
    c = cv_case(name)
    kw = c["kw"]
    H, W = c["levels"][3]
    world = _world(kw["coords"], c["D"], F64)
    for v in range(c["nv"]):
        a, b = ndc(world, kw["intrs"][v], kw["c2ws"][v], H, W, F64), _ndc(world, kw["intrs"][v], kw["c2ws"][v], H, W, F64)
        far = b[2].abs() > 1e-3
        assert bool(far.any())
        assert float((a[2] - b[2]).abs().max()) <= 1e-10 * 8.0                  # |q_z| <= |R| |x| + |t|: a few units
        for k in (0, 1):
            assert bool(((a[k] - b[k]).abs()[far] <= 1e-10 * (1.0 + b[k].abs()[far])).all()), (name, v, k)


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_matching_restatement_matches_float64_autograd(name):
    c = mb_case(name)
    for (two, jit), (g64, A, _, _) in c["ref"].items():
        mv = c["mvol"].to(F64).requires_grad_(True)
        j = c["jitter"] if jit else None
        _, full, _ = matching_ref(mv, c["intrs"], c["c2ws"], c["near_fars"], c["H"], c["W"], c["L"], c["n"], c["pre"], c["rc"], c["rp"],
                                  F64, jitter=j)
        sel = selected_views((0, c["src"]) if two else (0, 0), c["nv"])
        (full[sel] * c["g_full"][sel].to(F64)).sum().backward()             # the other views are rendered under no_grad
        assert float(mv.grad.abs().max()) > 0
        assert within(g64, mv.grad, 1e-10 * A), (name, two, jit)


@pytest.mark.parametrize("i", range(len(UPSAMPLE_CASES)))
def test_upsample_transpose_matches_float64_autograd(i):
    c = up_case(i)
    lr = torch.zeros(3, 1, c["h"], c["w"], dtype=F64, requires_grad=True)
    (F.interpolate(lr, size=(c["H"], c["W"]), mode="bilinear")[:, 0] * c["g_full"].to(F64)).sum().backward()
    assert within(c["g64"], lr.grad[:, 0], 1e-10 * c["A"])


@pytest.mark.parametrize("D", DENSIFY_D)
def test_densify_restatement_matches_float64_autograd(D):
    c = dn_case(D)
    n = c["coords"].shape[0]
    logit = torch.zeros(n, dtype=F64, requires_grad=True)
    prev = torch.zeros(D // 2, D // 2, D // 2, dtype=F64, requires_grad=True)
    dense, _ = O.sparse2dense(logit, c["coords"], D, prev)
    (dense * c["g_dense"].to(F64)).sum().backward()
    assert torch.equal(c["rows64"][:, 0], logit.grad) and float(c["rows64"][:, 1:].abs().max()) == 0
    assert within(c["prev64"], prev.grad, 1e-10 * c["A"])


def test_costvol_inputs_meet_their_conditions():
    splits, kinds, unseen, single, outside = set(), set(), 0, 0, 0
    for name in CV_CASES:
        c = cv_case(name)
        r = c["r64"]
        assert c["n_unc"] <= 0.01 * c["n_full"], (name, c["n_unc"])
        assert EPS_REMOVE >= eps_costvol()
        assert c["n"] == (CV_CASES[name][1] or c["n"])
        assert c["dispatch"] == c["expect"], (name, c["dispatch"])
        assert bool(torch.isfinite(r["g_agg"]).all()) and all(bool(torch.isfinite(t).all()) for t in r["gfeats"] if t is not None)
        seen = r["inside"].sum(0)
        unseen, single = unseen + int((seen == 0).sum()), single + int((seen == 1).sum())
        if c["n"] > 1:
            assert float((r["pre"] > 0.05).double().mean()) > 0.1 and float((r["pre"] < -0.05).double().mean()) > 0.1, name
            mag = c["G"].abs().max(dim=1).values
            assert float(mag.max() / mag.min()) > 300.0, name                          # upstream rows over three decades
            assert float(r["df"].abs().max()) > 0 and all(float(r["gfeats"][l].abs().max()) > 0 for l in range(c["stage"], 4)), name
        if c["dispatch"] in ("irregular", "buckets"):
            kinds.add(c["dispatch"])
        else:
            kinds.add("binned")
            splits.add(c["dispatch"][1])
            counts = torch.bincount(cv_buckets(r, c["levels"]).reshape(-1).clamp(min=-1) + 1)[1:]
            assert int(counts.max()) < 2 ** 20, name                                   # the fixed-point contract's condition
            outside += cv_taps_outside_lds(r, c["levels"], c["stage"])
    assert splits == {1, 2, 4, 8} and kinds == {"binned", "irregular", "buckets"}
    assert unseen > 0 and single > 0
    assert outside == 0                                                                # module docstring
    assert cv_case("6a")["n"] % 256 and cv_case("6b")["n"] == 257 and cv_case("1")["n"] % 256


def test_matching_inputs_meet_their_conditions():
    for name in MATCH_NAMES:
        c = mb_case(name)
        assert c["excluded"] <= 0.01, name
        assert all(bool((c["g_full"][v] != 0).any()) for v in range(c["nv"])), name       # every view's map carries gradient
        assert bool((c["jitter"][..., 1] != 0).all())
        for g64, A, T, r32 in c["ref"].values():
            assert bool(torch.isfinite(g64).all()) and float(g64.abs().max()) > 0
    assert any(c[0] % 2 for c in NEW_MATCH.values())                                       # odd D: z-pair keys straddle rows
    keys = keys_per_patch(mb_case("overflow"), (0, 1))
    assert len(keys) == 8 and max(keys) > MB_SLOTS > min(keys), keys
    assert MB_SLOTS == 2048                                                                # the case was sized for this table
    for name in ("0", "4", "odd"):                                                         # the others stay inside their table
        assert max(keys_per_patch(mb_case(name), (0, mb_case(name)["src"]))) < MB_SLOTS


def test_densify_inputs_meet_their_conditions():
    for D in DENSIFY_D:
        c = dn_case(D)
        occ = c["occ"]
        share = float(occ.double().mean())
        assert (0.25 < share < 0.35) if D >= 10 else (0.1 < share < 0.7), (D, share)
        assert bool(occ[0, 0, 0]) and not bool(occ[D - 1, D - 1, D - 1])
        cc = c["coords"].long()
        assert bool(((cc == 0) | (cc == D - 1)).any(dim=1).any()) and bool(((cc == 0) | (cc == D - 1)).all(dim=1).any())
        assert float(c["prev64"].abs().max()) > 0 and int(c["T"].max()) <= 64


CV_FAULTS = ("softmax_no_dot", "var_no_mean", "skip_level", "elu_one", "ds_unmasked", "tail256", "coarse")


@pytest.mark.parametrize("name", ["1", "2", "3", "5", "6a", "7"])
def test_sensitivity_costvol(name):
    """Each planted fault moves at least one element of the feature gradients - a texel or a per-(view, channel) sum - past the bar
    the GPU test uses (for the binned cases the binned form's bar, the wider of the two).  Case 7: its per-texel bar is wider than
    A_e (module docstring) and rejects nothing that stays on texels with terms; the sums reject every fault here.  The rounding to
    2^-20 of the largest term is a fault of the fixed-point (binned) form: not planted into the direct-scatter cases."""
    c = cv_case(name)
    binned = c["dispatch"] not in ("irregular", "buckets")
    bars, bar_agg, sum_bars = cv_bars(c, binned)
    good = c["r64"]

    def rejected(r, texels=True):
        lv = range(c["stage"], 4)
        return (texels and any(not within(r["gfeats"][l], good["gfeats"][l], bars[l]) for l in lv)) or \
            any(not within(r["gfeats"][l].sum((2, 3)), good["gfeats"][l].sum((2, 3)), sum_bars[l]) for l in lv) or \
            ("g_agg" in r and not within(r["g_agg"], good["g_agg"], bar_agg))     # (views outside the frustum put their taps outside too)
    assert not rejected(good)
    for fault in CV_FAULTS:
        if fault == "coarse" and not binned:
            continue
        if fault == "ds_unmasked" and bool(good["inside"].any(0).all()):
            assert name == "7"                                       # every voxel of its list is seen: the mask changes nothing
            continue
        r = costvol_bwd_ref(**c["kw"], fault=fault)
        assert rejected(r), (name, fault)
        if fault in ("softmax_no_dot", "var_no_mean", "elu_one", "ds_unmasked"):      # (a lattice's last voxels are seen by no view)
            assert not within(r["g_agg"], good["g_agg"], bar_agg), (name, fault)
    # one share of the records lost: one of the `split` shares of the fullest bucket (records in lattice order) of the binned form,
    # the last quarter of the fullest view's records of the direct one; and every term doubled
    if binned:
        split = c["dispatch"][1]
        b = cv_buckets(good, c["levels"]).reshape(-1)
        members = (b == int(torch.bincount(b + 1)[1:].argmax())).nonzero().view(-1)
        share = (members.numel() + split - 1) // split
        lost = members[share * (split - 1):]
        assert split > 1
    else:
        live = (good["df"] != 0).any(-1) & (good["nx"].abs() <= 1) & (good["ny"].abs() <= 1)
        v = int(live.sum(1).argmax())
        members = (live[v].nonzero().view(-1) + v * c["n"])
        lost = members[-max(1, members.numel() // 4):]
    drop = torch.zeros(c["nv"] * c["n"], dtype=torch.bool)
    drop[lost] = True
    assert bool(drop.any())
    assert rejected(costvol_bwd_ref(**c["kw"], drop=drop.reshape(c["nv"], c["n"]))), (name, "lost share")
    doubled = dict(gfeats=[None if g is None else 2.0 * g for g in good["gfeats"]])
    assert rejected(doubled, texels=False), (name, "doubled")


MB_FAULTS = ("no_cosz", "E_band0", "jitter_first_band_only", "second_view_dropped", "other_view_not_ignored")


@pytest.mark.parametrize("name", ["1", "6", "overflow"])
def test_sensitivity_matching(name):
    c = mb_case(name)
    for fault in MB_FAULTS + (("slots",) if name == "overflow" else ()):
        if c["pre"] is None and fault in ("E_band0", "jitter_first_band_only"):
            continue                                                   # one band only
        two = fault != "other_view_not_ignored"                        # (0, 0): view 1's map is the one to ignore
        g64, A, _, _ = c["ref"][(two, True)]
        bar = 4.0 * c["r32"] * A
        assert within(g64, g64, bar)
        bad, _ = match_bwd_ref(c, c["g_full"], (0, c["src"]) if two else (0, 0), c["jitter"], fault=fault)
        assert not within(bad, g64, bar), (name, fault)


@pytest.mark.parametrize("D", [4, 10, 34])
def test_sensitivity_densify(D):
    c = dn_case(D)
    for fault in ("mask_ignored", "ends_075", "all_columns"):
        rows, prev, _ = densify_bwd_ref(c["coords"], c["g_dense"], D, True, fault=fault)
        if fault == "all_columns":
            assert not torch.equal(rows, c["rows64"])
        else:
            assert not within(prev, c["prev64"], dn_bar(c)), (D, fault)


def _recorded():
    return {m.group(1): float(m.group(2)) for m in re.finditer(r"^\s+(\S+)\s+r32 = ([0-9.e+-]+)$", __doc__, re.M)}


def measured_r32():
    out = {}
    for name in CV_CASES:
        for kind in ("feat", "agg", "sum"):
            out[f"costvol_{name}_{kind}"] = cv_case(name)["r32"][kind]
    for name in MATCH_NAMES:
        out[f"matching_{name}"] = mb_case(name)["r32"]
    for i in range(len(UPSAMPLE_CASES)):
        out[f"upsample_{i}"] = up_case(i)["r32"]
    return out


def test_measured_margins_are_recorded():
    """The r32 values of the module docstring are the ones these inputs give (same arithmetic on any x86 host, 10 % of slack for
    another BLAS' summation order)."""
    rec, got = _recorded(), measured_r32()
    assert set(rec) == set(got), set(rec) ^ set(got)
    for key, v in got.items():
        assert (v == 0.0 and rec[key] == 0.0) or abs(v / max(rec[key], 1e-300) - 1.0) < 0.1, (key, v, rec[key])


# ------------------------------------------------------------------------------------------------------------------
# GPU helpers
# ------------------------------------------------------------------------------------------------------------------


def _guarded(n, fill=SENTINEL):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=F32, device=dev())
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n, what, fill=SENTINEL):
    h = buf.cpu()
    assert bool((h[:GUARD] == fill).all()) and bool((h[GUARD + n:] == fill).all()), f"{what} wrote outside its buffer"


def _env(name, fn):
    """Run fn with the switch `name` set (the library reads it per call)."""
    assert name not in os.environ
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def gpu_cameras(intrs, c2ws):
    """ops.Cameras with the inverses of the restatements (the float64 inverse rounded once) in place of the host's fp32 LAPACK ones:
    kernel and twin start from the same matrices."""
    from surf_amd import ops
    cams = ops._cams_ext(ops.Cameras(intrs, c2ws), intrs, c2ws)
    cams.w2c = np.ascontiguousarray(_inv(c2ws, F32).numpy())
    cams.kinv = np.ascontiguousarray(_inv(intrs, F32)[:, :3, :3].contiguous().numpy())
    cams.rinv = np.ascontiguousarray(_inv(c2ws[:, :3, :3], F32).contiguous().numpy())
    return cams


def _void_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def costvol_backward_direct(c, gfeats, g_agg, stage=None, null_level=None):
    """surf_costvol_backward through the C entry point, its workspace exactly surf_costvol_backward_workspace_floats_for(...)
    floats inside a guarded buffer.  -> the number of workspace floats."""
    from surf_amd import _lib, ops
    L, d, kw = _lib.lib(), dev(), c["kw"]
    cams = gpu_cameras(kw["intrs"], kw["c2ws"])
    feats_t4 = [f.permute(0, 2, 3, 1).contiguous().to(d) for f in kw["feats"]]
    hw = (ctypes.c_int * 8)(*[int(v) for f in feats_t4 for v in f.shape[1:3]])
    agg = np.ascontiguousarray(np.concatenate([t.reshape(-1).numpy() for t in kw["agg"]]), dtype=np.float32)
    nws = int(L.surf_costvol_backward_workspace_floats_for(c["n"], c["nv"], hw))
    wbuf, ws = _guarded(nws)
    coords, G = kw["coords"].to(torch.int32).to(d).contiguous(), kw["G"].to(d).contiguous()
    gptr = _void_array([None if l == null_level else t for l, t in enumerate(gfeats)])
    try:
        L.surf_costvol_backward(ops._p(coords), ops._p(G), c["n"], c["D"], ops._ptr_array(feats_t4), gptr, hw,
                                c["stage"] if stage is None else stage, c["nv"], ops._np_ptr(cams.intrs), ops._np_ptr(cams.w2c),
                                ops._np_ptr(agg), ops._p(ws), ops._p(g_agg), ops._stream())
    finally:
        torch.cuda.synchronize()
        _intact(wbuf, nws, ("costvol_backward workspace", c["name"]))
    return nws


def new_gfeats(c, base=None):
    """Gradient maps (texel4) for case c: a sentinel below the stage (the kernel must not touch them), zeros or `base` above."""
    d = dev()
    out = []
    for l, f in enumerate(c["kw"]["feats"]):
        nv, _, H, W = f.shape
        if l < c["stage"]:
            out.append(torch.full((nv, H, W, 4), SENTINEL, dtype=F32, device=d))
        else:
            out.append(torch.zeros(nv, H, W, 4, dtype=F32, device=d) if base is None else base[l].permute(0, 2, 3, 1).contiguous().to(d))
    return out


def check_costvol(c, gfeats, g_agg, binned, label, base=None, base_agg=None):
    """Every element of the feature gradients and of g_agg inside its bar; prints the kernel's largest err / A beside r32."""
    bars, bar_agg, sum_bars = cv_bars(c, binned)
    r64, A = c["r64"], c["A"]
    split = c["dispatch"][1] if binned else 1
    bad, rel, wf, ws, rel_s = [], 0.0, 0.0, 0.0, 0.0
    for l in range(4):
        got = gfeats[l].cpu().permute(0, 3, 1, 2)
        if l < c["stage"]:
            assert bool((got == SENTINEL).all()), (label, l, "a level below the stage was written")
            continue
        ref, bar = r64["gfeats"][l], bars[l]
        if base is not None:       # a texel lies in the LDS images of at most 4 tiles, each flushed by `split` workgroups: 4 split more
            ref = ref + base[l].double()                                   # roundings at the size of |base| + A
            bar = bar + 4.0 * split * U24 * (base[l].double().abs() + A["gfeats"][l])
        err = (got.double() - ref).abs()
        has = A["gfeats"][l] > 0
        rel = max(rel, float((err[has] / A["gfeats"][l][has]).max()) if bool(has.any()) else 0.0)
        w = worst(got, ref, bar)
        wf = max(wf, w)
        if not w <= 1.0:
            bad.append((l, w))
        # the per-(view, channel) sums over the level's texels (cv_bars)
        got_s, ref_s, bar_s = got.double().sum((2, 3)), r64["gfeats"][l].sum((2, 3)), sum_bars[l]
        if base is not None:
            got_s = (got.double() - base[l].double()).sum((2, 3))
            bar_s = bar_s + (4.0 * split * U24 * (base[l].double().abs() + A["gfeats"][l])).sum((2, 3))
        ws = max(ws, worst(got_s, ref_s, bar_s))
        rel_s = max(rel_s, float(((got_s - ref_s).abs() / A["gfeats"][l].sum((2, 3))).max()))
        if not worst(got_s, ref_s, bar_s) <= 1.0:
            bad.append((l, "sums", worst(got_s, ref_s, bar_s)))
    got, ref, bar = g_agg.cpu(), r64["g_agg"], bar_agg
    if base_agg is not None:
        ref, bar = ref + base_agg.double(), bar + U24 * (base_agg.double().abs() + A["g_agg"])
    err = (got.double() - ref).abs()
    has = A["g_agg"] > 0
    rel_agg = float((err[has] / A["g_agg"][has]).max()) if bool(has.any()) else 0.0
    w_agg = worst(got, ref, bar)
    print(f"costvol {label}: feat kernel err/A {rel:.3e} (r32 {c['r32']['feat']:.3e}), agg kernel err/A {rel_agg:.3e} "
          f"(r32 {c['r32']['agg']:.3e}), sums kernel err/A {rel_s:.3e} (r32 {c['r32']['sum']:.3e}), worst err/bar feat {wf:.3g} "
          f"agg {w_agg:.3g} sums {ws:.3g}")
    assert not bad, (label, "feature levels past their bar (level, err / bar)", bad)
    assert w_agg <= 1.0, (label, "g_agg err / bar", w_agg)


def _match_dev(c):
    from surf_amd import ops
    d = dev()
    if "_dev" not in c:
        c["_dev"] = dict(cams=gpu_cameras(c["intrs"], c["c2ws"]), mvol=c["mvol"].to(d).contiguous(),
                         pre=None if c["pre"] is None else c["pre"].to(d).contiguous())
    return c["_dev"]


def matching_backward_direct(c, g_full, views, g_lr, dmvol, nv=None):
    """surf_matching_depth_backward through the C entry point, with the caller's g_lr."""
    from surf_amd import _lib, ops
    d, m = dev(), _match_dev(c)
    H, W, L, n = c["H"], c["W"], c["L"], c["n"]
    h, w = H // L, W // L
    nf = ops._near_fars_host(c["near_fars"])
    _lib.lib().surf_matching_depth_backward(ops._p(m["mvol"]), int(c["D"]), c["nv"] if nv is None else nv, ops._np_ptr(m["cams"].kinv),
                                            ops._np_ptr(m["cams"].c2w), ops._np_ptr(m["cams"].rinv), ops._np_ptr(nf), H, W, h, w,
                                            ops._p(ops._linspace_dev(0, W - 1, w, d)), ops._p(ops._linspace_dev(0, H - 1, h, d)),
                                            ops._p(ops._linspace_dev(0.0, 1.0, n, d)), int(n), ops._p(m["pre"]), float(c["rc"]),
                                            float(c["rp"]), ops._p(None), ops._p(g_full), int(views[0]), int(views[1]), ops._p(g_lr),
                                            ops._p(dmvol), ops._p(None), ops._stream())


# ------------------------------------------------------------------------------------------------------------------
# B. exact or derivable
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("n", [1, 255, 257, 1500])
def test_scatter_rows_add_exact_and_bounded(n):
    """A permutation (no duplicates) is bit-exact; ~40 rows per target are within (T_e - 1) 2^-24 A_e (the first add to a zero is
    exact, each later one rounds a partial sum that |.| <= A_e); rows no index names keep their sentinel."""
    from surf_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(20 + n)
    for w in (1, 7, 8):
        for shift in (0, 3):
            for off in (0, 8):
                g_dst = (torch.randn(n, off + w + 3, generator=g) * 10.0 ** (-2.0 * torch.rand(n, 1, generator=g))).contiguous()
                for kind in ("permutation", "duplicates"):
                    rows = (n if kind == "permutation" else max(1, n // 40)) + 5
                    target = torch.randperm(rows, generator=g)[:n] if kind == "permutation" else torch.randint(0, rows - 5, (n,), generator=g)
                    idx = ((target << shift) + torch.randint(0, 1 << shift, (n,), generator=g)).to(torch.int32)
                    named = torch.zeros(rows, dtype=torch.bool)
                    named[target] = True
                    start = torch.full((rows, w), SENTINEL)
                    start[named] = 0.0
                    out = ops.scatter_rows_add(g_dst.to(d), idx.to(d), start.to(d), shift=shift, dst_off=off).cpu()
                    src = g_dst[:, off:off + w].double()
                    ref = torch.zeros(rows, w, dtype=F64).index_add_(0, target, src)
                    A = torch.zeros(rows, w, dtype=F64).index_add_(0, target, src.abs())
                    T = torch.bincount(target, minlength=rows).double()[:, None]
                    assert bool((out[~named] == SENTINEL).all()), (w, shift, off, kind)
                    if kind == "permutation":
                        assert torch.equal(out[named], ref[named].float()), (w, shift, off)
                    else:
                        assert within(out[named], ref[named], ((T - 1).clamp(min=0) * U24 * A)[named]), (w, shift, off)
                        assert n < 40 or float(T.max()) >= 20


@gpu
@pytest.mark.parametrize("D", DENSIFY_D)
def test_densify_backward_exact_rows_bounded_prev(D):
    """g_rows[:, 0] exact (one fp32 add per site), columns 1 .. 7 untouched, g_prev within dn_bar; a mostly-zero dense gradient
    (the gather form's early exit) accumulated into a non-zero g_prev; g_prev = None.  D = 2 runs the scatter form."""
    from surf_amd import ops
    d = dev()
    c = dn_case(D)
    n, Dp = c["coords"].shape[0], D // 2
    g = torch.Generator().manual_seed(900 + D)
    coords = c["coords"].to(d)
    table = O.get_index(c["coords"], D).to(torch.int32).to(d).contiguous()
    base_rows = torch.randn(n, 8, generator=g)
    want_rows = base_rows.clone()
    cc = c["coords"].long()
    want_rows[:, 0] = base_rows[:, 0] + c["g_dense"][cc[:, 0], cc[:, 1], cc[:, 2]]
    g_rows, g_prev = base_rows.to(d), torch.zeros(Dp, Dp, Dp, device=d)
    ops.densify_backward(coords, table, c["g_dense"].to(d), g_rows, g_prev)
    assert torch.equal(g_rows.cpu(), want_rows)
    print(f"densify D {D}: g_prev worst err / bar {worst(g_prev.cpu(), c['prev64'], dn_bar(c)):.3g}")
    assert within(g_prev.cpu(), c["prev64"], dn_bar(c))
    g_rows2 = base_rows.to(d)
    ops.densify_backward(coords, table, c["g_dense"].to(d), g_rows2, None)
    assert torch.equal(g_rows2.cpu(), want_rows)
    # mostly zero, into a non-zero g_prev
    Gs = torch.zeros(D, D, D)
    Gs[D // 2:, :2, 1] = c["g_dense"][D // 2:, :2, 1]
    Gs[0, 0, 0], Gs[D - 1, D - 1, D - 1], Gs[D - 1, 0, D - 1] = 1.5, -2.5, 0.75
    _, prev_s, _ = densify_bwd_ref(c["coords"], Gs, D, True)
    _, A_s, _ = densify_bwd_ref(c["coords"], Gs, D, True, absolute=True)
    assert float(prev_s.abs().max()) > 0
    base = torch.randn(Dp, Dp, Dp, generator=g)
    g_prev3 = base.to(d).clone()
    ops.densify_backward(coords, table, Gs.to(d), torch.zeros(n, 8, device=d), g_prev3)
    assert within(g_prev3.cpu(), base.double() + prev_s, dn_bar(dict(A=A_s), base))
    assert torch.equal(g_prev3.cpu()[A_s == 0], base[A_s == 0])                      # cells without a term keep their value


# ------------------------------------------------------------------------------------------------------------------
# C. costvol_backward
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name", list(CV_CASES))
def test_costvol_backward_by_dispatch(name):
    """Binned with split 1 / 2 / 4 / 8, direct by an irregular pyramid (and 700 / 257 / 1 voxels: replicated tail lanes), direct by
    more than 16,384 buckets; levels below the stage keep a sentinel; the workspace is exactly what the library asks for and the
    guard around it stays intact.  r32 per case: module docstring; the kernel's err / A is printed beside it (-s)."""
    c = cv_case(name)
    gfeats, g_agg = new_gfeats(c), torch.zeros(49, device=dev())
    nws = costvol_backward_direct(c, gfeats, g_agg)
    binned = c["dispatch"] not in ("irregular", "buckets")
    if not binned:
        assert nws == 4096, nws                                                        # the agg_mlp replicas only
    else:
        assert nws > 4096 + 9 * c["n"] * c["nv"]
    if c["nv"] == 1:
        assert torch.equal(g_agg.cpu(), torch.zeros(49))                               # one view: softmax = 1, nothing reaches agg_mlp
    check_costvol(c, gfeats, g_agg, binned, name)


@gpu
@pytest.mark.parametrize("name", ["1", "5"])
def test_costvol_backward_direct_switch(name):
    """SURF_CVB_DIRECT: the direct scatter on shapes the binned form would take, through the Python wrapper."""
    from surf_amd import ops
    c = cv_case(name)
    kw, d = c["kw"], dev()
    gfeats, g_agg = new_gfeats(c), torch.zeros(49, device=d)
    feats_t4 = [f.permute(0, 2, 3, 1).contiguous().to(d) for f in kw["feats"]]
    agg = np.concatenate([t.reshape(-1).numpy() for t in kw["agg"]]).astype(np.float32)
    _env("SURF_CVB_DIRECT", lambda: ops.costvol_backward(feats_t4, gfeats, c["stage"], c["D"], gpu_cameras(kw["intrs"], kw["c2ws"]), agg,
                                                         kw["coords"].to(torch.int32).to(d).contiguous(), kw["G"].to(d).contiguous(), g_agg))
    check_costvol(c, gfeats, g_agg, False, name + " direct")


@gpu
def test_costvol_backward_with_the_librarys_own_inverses():
    """Case 1 through ops.costvol_backward with ops.Cameras as it is: the host's fp32 inverse of c2ws, not gpu_cameras' matrices.  The
    float64 reference and A stay; r32 comes from the twin run with these very inverses (a host-dependent number: computed here, not
    recorded)."""
    from surf_amd import ops
    c = dict(cv_case("1"))
    kw, d = c["kw"], dev()
    cams = ops.Cameras(kw["intrs"], kw["c2ws"])
    t32 = costvol_bwd_ref(**kw, dt=F32, w2c=torch.from_numpy(cams.w2c.copy()))
    lv = range(c["stage"], 4)
    c["r32"] = dict(feat=max(rel_to_A(t32["gfeats"][l], c["r64"]["gfeats"][l], c["A"]["gfeats"][l]) for l in lv),
                    agg=rel_to_A(t32["g_agg"], c["r64"]["g_agg"], c["A"]["g_agg"]),
                    sum=max(rel_to_A(t32["gfeats"][l].sum((2, 3)), c["r64"]["gfeats"][l].sum((2, 3)), c["A"]["gfeats"][l].sum((2, 3))) for l in lv))
    gfeats, g_agg = new_gfeats(c), torch.zeros(49, device=d)
    feats_t4 = [f.permute(0, 2, 3, 1).contiguous().to(d) for f in kw["feats"]]
    agg = np.concatenate([t.reshape(-1).numpy() for t in kw["agg"]]).astype(np.float32)
    ops.costvol_backward(feats_t4, gfeats, c["stage"], c["D"], cams, agg, kw["coords"].to(torch.int32).to(d).contiguous(),
                         kw["G"].to(d).contiguous(), g_agg)
    check_costvol(c, gfeats, g_agg, True, "1 library inverses")


@gpu
@pytest.mark.parametrize("name", ["1", "6b"])
def test_costvol_backward_accumulates(name):
    """Into non-zero gfeats and g_agg: the same bars plus the roundings of the adds into the base (check_costvol)."""
    c = cv_case(name)
    g = torch.Generator().manual_seed(40)
    base = [None if l < c["stage"] else torch.randn(f.shape, generator=g) for l, f in enumerate(c["kw"]["feats"])]
    base_agg = torch.randn(49, generator=g)
    gfeats, g_agg = new_gfeats(c, base), base_agg.to(dev())
    costvol_backward_direct(c, gfeats, g_agg)
    check_costvol(c, gfeats, g_agg, c["dispatch"] not in ("irregular", "buckets"), name + " accumulate", base, base_agg)


# ------------------------------------------------------------------------------------------------------------------
# D. matching_depth_backward
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name", MATCH_NAMES)
def test_matching_depth_backward_views_jitter_stats(name):
    """views (0, 0), (0, src), (0, -1) with g_full non-zero on EVERY view, with and without jitter, from the forward's saved
    statistics and recomputed; 'odd': z-pair keys straddle rows; 'overflow': patches above and below the LDS table's size."""
    from surf_amd import ops
    d = dev()
    c = mb_case(name)
    m = _match_dev(c)
    g_full, jit_d = c["g_full"].to(d), c["jitter"].to(d)
    args = (m["mvol"], m["cams"], c["near_fars"], c["H"], c["W"], c["L"], c["n"])
    worst_rel, bad = 0.0, []
    for views in ((0, 0), (0, c["src"]), (0, -1)):
        two = views[1] > 0
        if views == (0, c["src"]) and not two:
            continue                                                                   # nv = 1
        for jit in (False, True):
            g64, A, _, _ = c["ref"][(two, jit)]
            bar = 4.0 * c["r32"] * A
            saved = {}
            ops.matching_depth(*args, m["pre"], c["rc"], c["rp"], jitter=jit_d if jit else None, saved=saved)
            for stats in (None, saved["stats"]):
                dm = ops.matching_depth_backward(*args, g_full, m["pre"], c["rc"], c["rp"], jitter=jit_d if jit else None, views=views,
                                                 stats=stats).cpu()
                err = (dm.double() - g64).abs()
                worst_rel = max(worst_rel, float((err[A > 0] / A[A > 0]).max()))
                wb = worst(dm, g64, bar)
                if not wb <= 1.0:
                    bad.append((views, jit, stats is not None, wb))
    print(f"matching {name}: kernel err/A {worst_rel:.3e} (r32 {c['r32']:.3e})")
    assert not bad, (name, "(views, jitter, stats, err / bar)", bad)


@gpu
def test_matching_depth_backward_accumulates():
    """Into a non-zero dmvol: a cell takes at most T_e adds (table flushes and direct atomics), each rounding at |base| + A_e."""
    from surf_amd import ops
    d = dev()
    c = mb_case("1")
    m = _match_dev(c)
    g64, A, T, _ = c["ref"][(True, True)]
    base = torch.randn(c["D"], c["D"], c["D"], generator=torch.Generator().manual_seed(41))
    dm = base.to(d).clone()
    ops.matching_depth_backward(m["mvol"], m["cams"], c["near_fars"], c["H"], c["W"], c["L"], c["n"], c["g_full"].to(d), m["pre"], c["rc"],
                                c["rp"], jitter=c["jitter"].to(d), dmvol=dm, views=(0, c["src"]))
    assert within(dm.cpu(), base.double() + g64, 4.0 * c["r32"] * A + T * U24 * (base.double().abs() + A))
    assert torch.equal(dm.cpu()[A == 0], base[A == 0])


@gpu
@pytest.mark.parametrize("i", range(len(UPSAMPLE_CASES)))
def test_upsample_transpose_g_lr(i):
    """g_lr of a direct call (all views' maps go through the transposed upsample) against float64, 4 r32 A_e."""
    u = up_case(i)
    d = dev()
    intrs, c2ws, near_fars = make_cameras(3, u["H"], u["W"])
    c = dict(D=8, H=u["H"], W=u["W"], L=u["H"] // u["h"], nv=3, n=4, pre=None, rc=1.0, rp=1.0, intrs=intrs, c2ws=c2ws,
             near_fars=near_fars, mvol=smooth_volume(8))
    assert (c["H"] // c["L"], c["W"] // c["L"]) == (u["h"], u["w"])
    gbuf, g_lr = _guarded(3 * u["h"] * u["w"])
    dmvol = torch.zeros(8, 8, 8, device=d)
    matching_backward_direct(c, u["g_full"].to(d).contiguous(), (0, 2), g_lr, dmvol)
    torch.cuda.synchronize()
    _intact(gbuf, 3 * u["h"] * u["w"], "g_lr")
    got = g_lr.cpu().reshape(3, u["h"], u["w"])
    print(f"upsample {i}: kernel err/A {rel_to_A(got, u['g64'], u['A']):.3e} (r32 {u['r32']:.3e})")
    assert within(got, u["g64"], 4.0 * u["r32"] * u["A"])
    assert float(dmvol.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------
# E. argument checks
# ------------------------------------------------------------------------------------------------------------------


@gpu
def test_argument_checks_raise_and_launch_nothing():
    from surf_amd import _lib, ops
    d = dev()
    # matching backward: bad view indices and too many views are refused before anything is written
    c = mb_case("1")
    h, w = c["H"] // c["L"], c["W"] // c["L"]
    c9 = dict(c)
    c9["intrs"], c9["c2ws"], c9["near_fars"] = make_cameras(9, c["H"], c["W"])
    c9.pop("_dev", None)
    c9["pre"] = None
    for cc, nv, views in ((c, c["nv"], (-1, 0)), (c, c["nv"], (c["nv"], 0)), (c, c["nv"], (0, c["nv"])), (c9, 9, (0, 1))):
        g_lr = torch.full((nv, h, w), SENTINEL, device=d)
        dmvol = torch.full((c["D"],) * 3, SENTINEL, device=d)
        g_full = torch.ones(nv, c["H"], c["W"], device=d)
        with pytest.raises(_lib.SurfHipError):
            matching_backward_direct(cc, g_full, views, g_lr, dmvol, nv=nv)
        torch.cuda.synchronize()
        assert bool((g_lr == SENTINEL).all()) and bool((dmvol == SENTINEL).all()), (nv, views)
    # densify backward: an odd lattice has no half-resolution parent
    D = 5
    coords = torch.tensor([[0, 0, 0], [4, 4, 4], [1, 2, 3]], dtype=torch.int32, device=d)
    table = O.get_index(coords.cpu(), D).to(torch.int32).to(d).contiguous()
    g_rows, g_prev = torch.full((3, 8), SENTINEL, device=d), torch.full((2, 2, 2), SENTINEL, device=d)
    with pytest.raises(_lib.SurfHipError):
        ops.densify_backward(coords, table, torch.ones(D, D, D, device=d), g_rows, g_prev)
    torch.cuda.synchronize()
    assert bool((g_rows == SENTINEL).all()) and bool((g_prev == SENTINEL).all())
    # costvol backward: stage 4; a null gradient map at a level the stage reads
    cv = cv_case("6b")
    for kw in (dict(stage=4), dict(null_level=3), dict(null_level=cv["stage"])):
        gfeats = [torch.full((cv["nv"], f.shape[2], f.shape[3], 4), SENTINEL, device=d) for f in cv["kw"]["feats"]]
        g_agg = torch.full((49,), SENTINEL, device=d)
        with pytest.raises(_lib.SurfHipError):
            costvol_backward_direct(cv, gfeats, g_agg, **kw)
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in gfeats) and bool((g_agg == SENTINEL).all()), kw
