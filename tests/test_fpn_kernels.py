"""The kernels of the feature pyramid (csrc/fpn.hip, fpn_mfma.hip) and its InstanceNorm backward (csrc/batchnorm.hip), each fed
directly at ragged map sizes and compared with float64 per element.

Part A (no GPU): a float64 restatement of the 3x3 convolution (stride 1 / 2), the stride-2 transposed convolution, the weight
gradient, InstanceNorm + ReLU (+ skip) and its backward, written as index arithmetic on NHWC arrays from the definitions of
include/surf_hip.h; pinned at float64 to torch.nn.functional and torch autograd, and - through FeatureNetwork.forward / backward
themselves, run on the CPU with the `ops` entry points replaced by the restatement - to oracle.surf_oracle.fpn_forward and its
autograd on the golden weights (so _pack_conv, _pack_deconv, flipT, deconv_dgrad, conv_s2_dgrad and the `finish` permutations
are all on the path); the conditions every input set of parts B-E has to meet; float64 emulations of subtly wrong kernels, each
of which has to break the very assertion parts B-E make.  Parts B-E (gpu): every instantiated kernel against the restatement.

How an element is compared.  u = 2^-24, B = the same expression over |x| and |W| (the magnitude sum), T = the real terms of the
element (valid taps x C_in; border pixels have 4 or 6 taps, transposed outputs 1, 2, 2 or 4 by parity class).
  * VALU convolutions (one fmaf per term into one accumulator): |got - ref| <= (T + 2) u B.
  * VALU weight gradient, T = P = the contributing pixels of the tap: the same form.  A term passes through at most P - 1 adds
    whose two operands are both non-zero (fmaf(0, d, acc) and acc + 0 are exact: padding, the G group sums of the thin pairs and
    the empty slots of a partial staging round round nothing), whatever the split into 2,048-pixel chunks; the chunk partials
    are added in float64 (<= P 2^-53) and cast once (u): (P - 1 + 1 + 1) u <= (P + 2) u.
  * exact bf16x3 on the matrix cores: x = x0 + x1 + x2 + r, x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1) (the
    residuals are exact in float32, surf_split3_bf16): |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x|, |r| <= 2^-27 |x|.  The six products
    kept are (0,0) (0,1) (1,0) (1,1) (0,2) (2,0); dropped are x1 w2 + x2 w1 (2 x 2^-27), x2 w2 (2^-36) and r w + x r' (2 x
    2^-27): 2^-25 (1 + 2^-11) |x| |w| per term, rounded up to 2^-24.  Every bf16 x bf16 product is exact in float32, and the
    accumulator is rounded per MFMA instruction (6 per 16 terms), not per term: (T + 2) u covers the accumulation of all six
    streams with room.  gamma = (T + 2) u + 2^-24.  (The sparse file's 2^-21 does not follow from the split and is not used.)
  * precision 1: both operands rounded to bf16 on the CPU (torch's round-to-nearest-even cast = (__bf16)x of surf_pack2_bf16);
    against the exact result of the rounded operands, (T + 2) u.
  * InstanceNorm statistics.  The sums are float64, of x - x[pixel 0] (see below): the mean carries the sums' slack
    (HW + 4) 2^-53 mean|x - p| and one float32 rounding, 0.5 ulp; var = E[(x-p)^2] - E[x-p]^2 carries 2 (HW + 4) 2^-53
    mean (x-p)^2, which reaches rstd as rstd / 2 x that / (var + eps) (asserted <= 0.2 ulp in part A for every input), and
    rstd = (float)(1 / sqrt(var + 1e-5)) is one float32 rounding of float64 arithmetic: 0.5 ulp + that slack.
  * InstanceNorm output, with bm, br the two bounds above: |(x - mean) rstd| moves by bm rstd + |x - mean| br, the kernel's
    subtraction and product add 2 u |xhat|; the ReLU is 1-Lipschitz; + u |out| for the skip add.  The output must ALSO be the
    float32 expression fmaxf((x - mean) * rstd, 0) (+ skip) of the statistics the kernel itself wrote, bit for bit (the build
    contracts nothing: -ffp-contract=off).
  * InstanceNorm backward, statistics given (the float32 cast of the restatement's): xh is two float32 operations (2 u |xh|), so
    the float64 sum of zbar xh carries (2 u + (n + 4) 2^-53) mean|zbar xh|; each sum is cast (u) and divided by n (counted at
    2.5 u as the sparse file counts a division): a = mean(zbar) within 3.5 u |a| + (n + 4) 2^-53 mean|zbar|, g = mean(zbar xh)
    within 3.5 u |g| + (2 u + (n + 4) 2^-53) mean|zbar xh|; xh g: |xh| dg + 3 u |xh g|; two subtractions u |zbar - a| + u |v|;
    the product with rstd u |dx|.  The gate: fl(x - mean) has the sign of x - mean and rstd > 0, so the float32 xh is > 0 exactly
    when the float64 one is - the propagated error of the gate is zero and no element needs a nudge (asserted in part A).

Statements of the issue this file was written for that cannot hold as worded, restated:
  * a transposed convolution writes 4 N H W outputs, never 128 k + 1: its dead-wave shape has 128 + 4 outputs ((1, 3, 11));
    the strided ones get shapes of their own with 129 outputs ((1, 3, 43) and (1, 6, 86)): "one shape" is one per mode.
  * no |xhat| can lie "within the propagated error of zero" (above); instead elements with x = mean EXACTLY (xhat = 0 in float32
    and float64 alike, dy != 0) are planted: they are what tells a gate of `>` from `>=`.
  * the float32 yardstick of the rms criterion adds one term at a time in the order of the definition (taps, then channels;
    pixels in order), so that it does not depend on a BLAS' blocking.

Which test reaches which path:
  dead waves in the last workgroup (129 / 132 outputs)      test_conv_*_per_element, shapes (1, 3, 43), (1, 6, 86), (1, 3, 11)
  32-pixel tiles holding two images, lanes i >= total       the same tests, shapes (3, 5, 7), (3, 6, 10) (S2: 45 outputs)
  a tap no lane of a wave has a source for (any == false)   test_conv_mfma_per_element, shapes (2, 1, 38), (3, 6, 1), (1, 1, 1)
  1 and 2 pixels per side                                   (1, 1, 1), (1, 2, 2)
  more than 64 statistics blocks (finalise: second stride)  test_inorm_forward[8] (258 x 255), large66048
  the InstanceNorm backward's second trip                   test_inorm_backward[64], hw = 4,097
  wgrad_kernel's 256- and 64-pixel rounds, partial last     test_wgrad_valu_per_element (totals 1 .. 2,049)
  wgrad_finalize_kernel's paired loop and its tail          test_wgrad_valu_many_chunks (9 chunks); 1 and 2 chunks above
  the thin pairs on the matrix cores                        test_wgrad_mfma_per_element under SURF_FPN_WGRAD_THIN_MFMA

Found by part C: inorm_partial_kernel summed x and x^2 themselves, and var = E[x^2] - mean^2 lost a channel whose mean is
large against its spread even in float64.  Worst rstd error of the kernel on an MI355X, in float32 ulp: 36 on `offset` (C = 64,
3 pixels, mean 19,200, spread 1), 62 on large66048, 171 on large48, 411 on large1025 (the float64 emulation of part A: 505 to
23,700 on the three large-mean inputs).  It now sums x - x[pixel 0], as bn_partial_kernel does: at most 0.5 ulp on every input
of part C (`normal` was at 0.5 before and after).  Nothing else failed: the worst |error| / bound of the other kernels is 0.25
(VALU convolutions), 0.08 (matrix-core convolutions), 0.33 / 0.76 (VALU / matrix-core weight gradients), 0.86 (InstanceNorm
backward); the InstanceNorm mean sits at its bound of half an ulp (0.999).

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest; smallest .. largest over the channel pairs):
rms over all elements of (float32 evaluation - float64) / B
    conv fp32 (2, 22, 38)       2.8e-08 .. 3.0e-08
    conv bf16 (2, 22, 38)       9.8e-09 .. 1.1e-08
    conv fp32 (3, 6, 10)        2.7e-08 .. 3.1e-08
    conv bf16 (3, 6, 10)        9.9e-09 .. 1.1e-08
    wgrad fp32 2047             2.7e-08 .. 3.1e-08
    wgrad fp32 2049             2.6e-08 .. 3.4e-08
    wgrad fp32 16641            2.8e-08 .. 2.8e-08
    wgrad fp32 mfma shapes      2.6e-08 .. 3.1e-08
    wgrad bf16 mfma shapes      9.3e-09 .. 1.2e-08
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import surf_oracle as O
from tests.test_sparse_unet_kernels import SENTINEL, _bf16_pieces, _gen, _holds, rel_rms, ulp32

gpu = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U = 2.0 ** -24
SPLIT = 2.0 ** -24                 # the dropped products of the exact bf16x3 form (module docstring)
UP = "up"                          # modes: 1 = stride 1, 2 = stride 2, UP = stride-2 transposed
EPS = 1e-5

CONV_CASES = [(4, 8, 1), (8, 8, 1), (8, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 64, 2), (64, 64, 1), (8, 4, 1),
              (16, 4, 1), (32, 4, 1), (64, 4, 1), (4, 16, 1), (4, 32, 1), (4, 64, 1)]                   # CONV_CASE, fpn.hip
DECONV_CASES = [(64, 32), (32, 16), (16, 8)]                                                              # DECONV_CASE
MFMA_CASES = [(32, 32, 1), (64, 64, 1), (16, 32, 2), (32, 64, 2), (64, 32, UP), (32, 16, UP)]             # FM_CONV, fpn_mfma.hip
WGRAD_CASES = [(4, 8, 1), (8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (8, 4, 1), (16, 4, 1), (32, 4, 1), (64, 4, 1),
               (8, 16, 2), (16, 32, 2), (32, 64, 2)]                                                      # WGRAD_CASE
WGRAD_MFMA = [(16, 16, 1), (32, 32, 1), (64, 64, 1), (64, 4, 1), (16, 32, 2), (32, 64, 2)]                # FM_WGRAD, dispatched
WGRAD_THIN = [(8, 16, 2), (8, 8, 1), (8, 4, 1), (4, 8, 1), (16, 4, 1), (32, 4, 1)]                        # ... under the switch

SHAPES = [(1, 1, 1), (1, 2, 2), (2, 1, 38), (3, 6, 1), (3, 5, 7), (3, 6, 10), (2, 22, 38)]                # (N, H, W) of the input
DEAD = {1: (1, 3, 43), 2: (1, 6, 86), UP: (1, 3, 11)}             # 129, 129 and 132 outputs: three dead waves of four
RMS_SHAPES = [(2, 22, 38), (3, 6, 10)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def shapes_for(mode):
    return [s for s in SHAPES if mode != 2 or (s[1] % 2 == 0 and s[2] % 2 == 0)] + [DEAD[mode]]


def out_size(mode, H, W):
    return (2 * H, 2 * W) if mode == UP else (H // mode, W // mode)


# ------------------------------------------------------------------------------------------------------------------
# the float64 restatement: convolutions
# ------------------------------------------------------------------------------------------------------------------


def _axis(n_out, n_in, mode, k, mut=""):
    """Along one axis: the input index output o reads through tap k, and whether there is one.  Convolution: o S + k - 1;
    transposed: (o + 1 - k) / 2 where the numerator is even and non-negative.  mut (part A.4): "no_parity" halves odd
    numerators too, "clamp" reads the nearest border pixel where there is none."""
    o = torch.arange(n_out)
    if mode == UP:
        t = o + 1 - k
        ok = (t >= 0) if mut == "no_parity" else (t >= 0) & (t % 2 == 0)
        i = torch.div(t, 2, rounding_mode="floor")
    else:
        i, ok = o * mode + k - 1, torch.ones(n_out, dtype=torch.bool)
    if mut == "clamp":
        return i.clamp(0, n_in - 1), ok
    return i.clamp(0, n_in - 1), ok & (i >= 0) & (i < n_in)


def gather(x, mode, ky, kx, mut=""):
    """(N, Ho, Wo, C): the input pixel every output pixel reads through tap (ky, kx), zero where it has none.  mut "wrap": the
    rows of the N images are one run of N H rows and only its two ends are padded (row -1 of image n + 1 = row H - 1 of image n)."""
    N, H, W, C = x.shape
    Ho, Wo = out_size(mode, H, W)
    yi, oky = _axis(Ho, H, mode, ky, mut)
    xi, okx = _axis(Wo, W, mode, kx, mut)
    if mut == "wrap":
        rows = torch.arange(N)[:, None] * H + (torch.arange(Ho) * mode + ky - 1)[None, :]
        okr = (rows >= 0) & (rows < N * H)
        g = x.reshape(N * H, W, C)[rows.clamp(0, N * H - 1)] * okr[:, :, None, None].to(x.dtype)
        return g[:, :, xi] * okx[None, None, :, None].to(x.dtype)
    return x[:, yi][:, :, xi] * (oky[:, None] & okx[None, :])[None, :, :, None].to(x.dtype)


def conv_ref(x, w, mode, dt=F64, mut=""):
    """out[n, yo, xo, co] = sum over (ky, kx, ci) of x[n, source] W[ky, kx, ci, co]; w is [ky][kx][ci][co].  At float32 the terms
    are added one at a time in the order of the definition (the yardstick of the rms criterion); mut "swap": [ky][kx][co][ci]."""
    x, w = x.to(dt), w.to(dt)
    Ho, Wo = out_size(mode, x.shape[1], x.shape[2])
    out = torch.zeros(x.shape[0], Ho, Wo, w.shape[3], dtype=dt)
    for ky in range(3):
        for kx in range(3):
            g = gather(x, mode, ky, kx, mut)
            wk = w[ky, kx].t() if mut == "swap" else w[ky, kx]
            if dt == F32:
                for ci in range(wk.shape[0]):
                    out = out + g[..., ci, None] * wk[ci]
            else:
                out = out + g @ wk
    return out


@functools.lru_cache(maxsize=None)
def tap_count(mode, shape):
    """(Ho, Wo) int64: the taps of an output pixel that have a source."""
    _, H, W = shape
    Ho, Wo = out_size(mode, H, W)
    cnt = torch.zeros(Ho, Wo, dtype=torch.int64)
    for ky in range(3):
        for kx in range(3):
            cnt += (_axis(Ho, H, mode, ky)[1][:, None] & _axis(Wo, W, mode, kx)[1][None, :]).long()
    return cnt


def wgrad_ref(big, small, S, dt=F64):
    """out[ky, kx, cb, cs] = sum over (n, ys, xs) of big[n, ys S + ky - 1, xs S + kx - 1, cb] small[n, ys, xs, cs].  At float32:
    one pixel at a time, in order (numpy keeps float32)."""
    big, small = big.to(dt), small.to(dt)
    cb, cs = big.shape[3], small.shape[3]
    out = torch.zeros(3, 3, cb, cs, dtype=dt)
    for ky in range(3):
        for kx in range(3):
            g = gather(big, S, ky, kx).reshape(-1, cb)
            s = small.reshape(-1, cs)
            if dt == F32:
                acc, gn, sn = np.zeros((cb, cs), np.float32), g.numpy(), s.numpy()
                for p in np.nonzero(np.abs(gn).sum(1))[0]:                 # (a padded pixel adds exact zeros)
                    acc += gn[p][:, None] * sn[p][None, :]
                out[ky, kx] = torch.from_numpy(acc)
            else:
                out[ky, kx] = g.t() @ s
    return out


def wgrad_pixels(N, Hs, Ws, S):
    """(3, 3, 1, 1) float64: the pixels that contribute to a tap."""
    P = torch.zeros(3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            P[ky, kx] = N * int(_axis(Hs, Hs * S, S, ky)[1].sum()) * int(_axis(Ws, Ws * S, S, kx)[1].sum())
    return P[:, :, None, None]


# ------------------------------------------------------------------------------------------------------------------
# the float64 restatement: InstanceNorm + ReLU (+ skip) and its backward
# ------------------------------------------------------------------------------------------------------------------


def inorm_ref(x, mut=""):
    """x (N, HW, C) float32 -> float64 mean, biased var, rstd = 1 / sqrt(var + 1e-5) per (n, c), (N, 1, C) each, and the slack
    the float64 sums of x - x[pixel 0] may carry.  mut (part A.4): "unbiased", "eps6", "raw" = var = E[x^2] - mean^2 of x itself
    with sequential float64 sums."""
    x64 = x.to(F64)
    HW = x.shape[1]
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    eps = EPS
    if mut == "unbiased":
        var = var * HW / (HW - 1)
    if mut == "eps6":
        eps = 1e-6
    if mut == "raw":
        mean = torch.cumsum(x64, 1)[:, -1:] / HW
        var = (torch.cumsum(x64 * x64, 1)[:, -1:] / HW - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    d = x64 - x64[:, :1]
    k = (HW + 4) * 2.0 ** -53
    slack_mean = k * d.abs().mean(1, keepdim=True) + 2.0 ** -52 * mean.abs()
    slack_rstd = 0.5 * rstd * 2 * k * (d * d).mean(1, keepdim=True) / (var + eps) + 2.0 ** -51 * rstd
    return dict(mean=mean, var=var, rstd=rstd, slack_mean=slack_mean, slack_rstd=slack_rstd)


def inorm_out(x, r, skip, before_relu=False):
    xh = (x.to(F64) - r["mean"]) * r["rstd"]
    if skip is None:
        return torch.relu(xh)
    return torch.relu(xh + skip.to(F64)) if before_relu else torch.relu(xh) + skip.to(F64)


def stat_bounds(r):
    return 0.5 * ulp32(r["mean"]) + r["slack_mean"], 0.5 * ulp32(r["rstd"]) + r["slack_rstd"]


def check_inorm(what, x, skip, r, mean, rstd, out):
    """The assertions of part C for one call: mean, rstd (N, 1, C) and out (N, HW, C) as the kernel wrote them (float32), against
    inorm_ref(x) = r.  -> (worst |error| / bound, worst rstd error in float32 ulp)."""
    bm, br = stat_bounds(r)
    worst = max(_holds(mean, r["mean"], bm, what + ("mean",)), _holds(rstd, r["rstd"], br, what + ("rstd",)))
    ref = inorm_out(x, r, skip)
    xc = x.to(F64) - r["mean"]
    bound = (bm * r["rstd"] + xc.abs() * br + 2 * U * (xc * r["rstd"]).abs()) * (1 + 1e-6)
    if skip is not None:
        bound = bound + U * ref.abs()
    worst = max(worst, _holds(out, ref, bound, what + ("out",)))
    own = torch.clamp_min((x - mean) * rstd, 0.0)
    assert torch.equal(out, own + skip if skip is not None else own), what + ("out is not the float32 expression of its own statistics",)
    return worst, float(((rstd.to(F64) - r["rstd"]).abs() / ulp32(r["rstd"])).max())


def inorm_bwd_ref(x, dy, mean32, rstd32, gate_ge=False):
    """dx = rstd (zbar - mean(zbar) - xhat mean(zbar xhat)), zbar = dy where xhat > 0, in float64 of the float32 inputs
    (x, dy (N, hw, C); mean32, rstd32 (N, 1, C)), and the bound of the module docstring."""
    mu, rs = mean32.to(F64), rstd32.to(F64)
    xh = (x.to(F64) - mu) * rs
    zb = torch.where((xh >= 0) if gate_ge else (xh > 0), dy.to(F64), torch.zeros((), dtype=F64))
    n = x.shape[1]
    a, g = zb.mean(1, keepdim=True), (zb * xh).mean(1, keepdim=True)
    k = (n + 4) * 2.0 ** -53
    t1 = zb - a
    v = t1 - xh * g
    dx = rs * v
    err_a = 3.5 * U * a.abs() + k * zb.abs().mean(1, keepdim=True)
    err_g = 3.5 * U * g.abs() + (2 * U + k) * (zb * xh).abs().mean(1, keepdim=True)
    bound = rs * (err_a + U * t1.abs() + xh.abs() * err_g + 3 * U * (xh * g).abs() + U * v.abs()) * (1 + 1e-6) + U * dx.abs()
    return dict(dx=dx, bound=bound, xh=xh)


# ------------------------------------------------------------------------------------------------------------------
# inputs and the references that go with them
# ------------------------------------------------------------------------------------------------------------------


def _rounded(t, variant):
    return t if variant == "fp32" else t.to(BF16).to(F32)


@functools.lru_cache(maxsize=None)
def conv_case(cin, cout, mode, shape):
    g = _gen("fpn conv", cin, cout, mode, shape)
    N, H, W = shape
    return dict(x=torch.randn(N, H, W, cin, generator=g), w=torch.randn(3, 3, cin, cout, generator=g) / (3.0 * cin ** 0.5))


@functools.lru_cache(maxsize=None)
def conv_reference(cin, cout, mode, shape, variant):
    c = conv_case(cin, cout, mode, shape)
    x, w = _rounded(c["x"], variant), _rounded(c["w"], variant)
    return dict(y=conv_ref(x, w, mode), B=conv_ref(x.abs(), w.abs(), mode), T=(tap_count(mode, shape) * cin).to(F64)[None, :, :, None])


@functools.lru_cache(maxsize=None)
def conv_rms32(cin, cout, mode, shape, variant):
    c, r = conv_case(cin, cout, mode, shape), conv_reference(cin, cout, mode, shape, variant)
    return rel_rms(conv_ref(_rounded(c["x"], variant), _rounded(c["w"], variant), mode, F32), r["y"], r["B"])


def check_conv(cin, cout, mode, shape, got, path, rms=False):
    """The assertions of part B for one output of the path "valu" | "mfma" (exact bf16x3) | "bf16" (precision 1).  -> the worst
    |error| / bound."""
    variant = "bf16" if path == "bf16" else "fp32"
    r = conv_reference(cin, cout, mode, shape, variant)
    what = ("conv", cin, cout, mode, shape, path)
    worst = _holds(got, r["y"], ((r["T"] + 2) * U + (SPLIT if path == "mfma" else 0.0)) * r["B"], what)
    if rms:
        mine, base = rel_rms(got, r["y"], r["B"]), conv_rms32(cin, cout, mode, shape, variant)
        assert mine <= 4 * base, f"{what}: rms of (got - float64) / B = {mine:.3g}, float32 on the CPU {base:.3g}: {mine / base:.3g} x"
    return worst


# weight gradients: (N, Hs, Ws) of the small map
WGRAD_TOTALS = [(1, 1, 1), (1, 7, 9), (1, 5, 13), (3, 5, 17), (1, 1, 257), (1, 23, 89), (3, 1, 683)]     # 1, 63, 65, 255, 257, 2,047, 2,049
WGRAD_BIG = (1, 129, 129)                                                                              # 16,641 pixels: 9 chunks
WGRAD_BIG_CASES = [(64, 64, 1), (32, 64, 2), (8, 4, 1)]              # 512 register blocks, exactly 256, a thin pair
WGRAD_MFMA_SHAPES = [(N, Hs, Ws) for N in (1, 2) for Hs in (1, 4, 5) for Ws in (1, 15, 16, 17, 33)]
WGRAD_RMS = [(1, 23, 89), (3, 1, 683), WGRAD_BIG, (2, 4, 33), (2, 5, 33)]


@functools.lru_cache(maxsize=None)
def wgrad_case(cb, cs, S, shape):
    g = _gen("fpn wgrad", cb, cs, S, shape)
    N, Hs, Ws = shape
    return dict(big=torch.randn(N, Hs * S, Ws * S, cb, generator=g), small=torch.randn(N, Hs, Ws, cs, generator=g))


@functools.lru_cache(maxsize=None)
def wgrad_reference(cb, cs, S, shape, variant):
    c = wgrad_case(cb, cs, S, shape)
    b, s = _rounded(c["big"], variant), _rounded(c["small"], variant)
    return dict(dW=wgrad_ref(b, s, S), A=wgrad_ref(b.abs(), s.abs(), S), P=wgrad_pixels(*shape, S))


@functools.lru_cache(maxsize=None)
def wgrad_rms32(cb, cs, S, shape, variant):
    c, r = wgrad_case(cb, cs, S, shape), wgrad_reference(cb, cs, S, shape, variant)
    return rel_rms(wgrad_ref(_rounded(c["big"], variant), _rounded(c["small"], variant), S, F32), r["dW"], r["A"])


def check_wgrad(cb, cs, S, shape, got, path, rms=False):
    variant = "bf16" if path == "bf16" else "fp32"
    r = wgrad_reference(cb, cs, S, shape, variant)
    what = ("wgrad", cb, cs, S, shape, path)
    worst = _holds(got, r["dW"], ((r["P"] + 2) * U + (SPLIT if path == "mfma" else 0.0)) * r["A"], what)
    if rms:
        mine, base = rel_rms(got, r["dW"], r["A"]), wgrad_rms32(cb, cs, S, shape, variant)
        assert mine <= 4 * base, f"{what}: rms of (got - float64) / A = {mine:.3g}, float32 on the CPU {base:.3g}: {mine / base:.3g} x"
    return worst


# InstanceNorm
INORM_CHANNELS = (4, 8, 16, 32, 64)
INORM_BWD_CHANNELS = (8, 16, 32, 64)
LARGE = {"large48": (15600.0, 0.055, 48, 64, 3), "large66048": (4000.0, 0.02, 66048, 8, 1), "large1025": (15600.0, 0.055, 1025, 64, 3)}
BIG_MAP = (258 * 255, 8, 1)                                          # 65,790 pixels = 65 statistics blocks


def inorm_sizes(C):
    G = 256 // C
    return [1, G - 1, 1023, 1024, 1025, 4 * G + 3, 2049]


def inorm_cases(C):
    """(kind, HW, N) of part C's forward for this channel count."""
    out = [(kind, HW, N) for kind in ("normal", "offset") for HW in inorm_sizes(C) for N in (1, 3)]
    if C == BIG_MAP[1]:
        out += [("normal", BIG_MAP[0], 1), ("offset", BIG_MAP[0], 1)]
    return out + [(k, v[2], v[4]) for k, v in LARGE.items() if v[3] == C]


@functools.lru_cache(maxsize=8)
def inorm_case(kind, C, HW, N):
    g = _gen("fpn inorm", kind, C, HW, N)
    x = torch.randn(N, HW, C, generator=g)
    if kind == "offset":
        x = x + 300.0 * (torch.arange(C, dtype=F32) + 1)
    if kind in LARGE:
        mean, spread = LARGE[kind][:2]
        x = mean * (0.75 + 0.25 * (torch.arange(C, dtype=F32) + 1) / C) + spread * x
    return dict(x=x.contiguous(), skip=torch.randn(N, HW, C, generator=g))


def inorm_bwd_sizes(C):
    return [1, 5, 1025] + ([4097] if C == 64 else [])


@functools.lru_cache(maxsize=8)
def inorm_bwd_case(C, hw, N):
    """x, dy and the float32 statistics of the restatement; from 5 pixels on, pixel 2 of channels 0 and 1 holds the float32 mean
    of its (n, c) exactly: xhat = 0 there, in any precision."""
    g = _gen("fpn inorm bwd", C, hw, N)
    x = (torch.randn(N, hw, C, generator=g) * 1.5 + 0.3).contiguous()
    if hw >= 5:
        for c in (0, 1):
            others = torch.cat([x[:, :2, c], x[:, 3:, c]], dim=1).to(F64)
            x[:, 2, c] = others.mean(1).to(F32)
    r = inorm_ref(x)
    return dict(x=x, dy=torch.randn(N, hw, C, generator=g), mean=r["mean"].to(F32), rstd=r["rstd"].to(F32))


def check_inorm_bwd(C, hw, N, dx):
    c = inorm_bwd_case(C, hw, N)
    r = inorm_bwd_ref(c["x"], c["dy"], c["mean"], c["rstd"])
    return _holds(dx, r["dx"], r["bound"], ("inorm backward", C, hw, N))


# ------------------------------------------------------------------------------------------------------------------
# A. the restatement against torch and the oracle
# ------------------------------------------------------------------------------------------------------------------


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(b.abs().max()) > 0.05 and float((a - b).abs().max()) <= tol * (1 + float(b.abs().max())), float((a - b).abs().max())


def test_restatement_is_torch_at_float64():
    import torch.nn.functional as F
    g = _gen("pin")
    for N, H, W in ((2, 6, 10), (1, 1, 1), (2, 2, 2), (3, 5, 7)):
        x = torch.randn(N, H, W, 8, generator=g, dtype=F64)
        wc = torch.randn(16, 8, 3, 3, generator=g, dtype=F64)                      # Conv2d (Cout, Cin, 3, 3)
        wd = torch.randn(8, 16, 3, 3, generator=g, dtype=F64)                      # ConvTranspose2d (Cin, Cout, 3, 3)
        for S in (1, 2):
            if S == 2 and (H % 2 or W % 2):
                continue
            xr, wr = _nchw(x).clone().requires_grad_(True), wc.clone().requires_grad_(True)
            y = F.conv2d(xr, wr, None, stride=S, padding=1)
            _close(conv_ref(x, wc.permute(2, 3, 1, 0), S), _nhwc(y.detach()))
            dy = torch.randn(y.shape, generator=g, dtype=F64)
            (y * dy).sum().backward()
            _close(wgrad_ref(x, _nhwc(dy), S).permute(3, 2, 0, 1), wr.grad)        # [ky][kx][ci][co] -> (Cout, Cin, 3, 3)
        xr, wr = _nchw(x).clone().requires_grad_(True), wd.clone().requires_grad_(True)
        y = F.conv_transpose2d(xr, wr, None, stride=2, padding=1, output_padding=1)
        _close(conv_ref(x, wd.permute(2, 3, 0, 1), UP), _nhwc(y.detach()))
        dy = torch.randn(y.shape, generator=g, dtype=F64)
        (y * dy).sum().backward()
        _close(wgrad_ref(_nhwc(dy), x, 2).permute(3, 2, 0, 1), wr.grad)            # [ky][kx][co][ci] -> (Cin, Cout, 3, 3)
    # InstanceNorm + ReLU + skip, forward and backward
    for N, HW, C in ((2, 35, 8), (1, 1025, 16), (3, 7, 4)):
        x = torch.randn(N, HW, C, generator=g) * 2 + 1
        skip, dy = torch.randn(N, HW, C, generator=g), torch.randn(N, HW, C, generator=g)
        xr = x.to(F64).permute(0, 2, 1)[..., None].clone().requires_grad_(True)    # (N, C, HW, 1)
        y = torch.relu(F.instance_norm(xr, eps=EPS)) + skip.to(F64).permute(0, 2, 1)[..., None]
        r = inorm_ref(x)
        _close(inorm_out(x, r, skip), y.detach()[..., 0].permute(0, 2, 1))
        (y * dy.to(F64).permute(0, 2, 1)[..., None]).sum().backward()
        b = inorm_bwd_ref(x, dy, r["mean"], r["rstd"])                              # (float64 statistics here)
        _close(b["dx"], xr.grad[..., 0].permute(0, 2, 1), 1e-10)


class _RestatementOps:
    """The entry points FeatureNetwork calls, computed by the restatement in float64 on the CPU."""

    @staticmethod
    def pack_texel4(x):
        n, C, H, W = x.shape
        out = torch.zeros(n, H, W, 4, dtype=F64)
        out[..., :C] = _nhwc(x.to(F64))
        return out

    @staticmethod
    def conv3x3(x, w_packed, cout, stride=1, precision=0):
        assert w_packed.shape == (3, 3, x.shape[3], cout) and w_packed.is_contiguous()
        return conv_ref(x, w_packed, stride)

    @staticmethod
    def deconv3x3_s2(x, w_packed, cout, precision=0):
        assert w_packed.shape == (3, 3, x.shape[3], cout) and w_packed.is_contiguous()
        return conv_ref(x, w_packed, UP)

    @staticmethod
    def conv3x3_wgrad(big, small, stride=1, precision=0):
        return wgrad_ref(big, small, stride)

    @staticmethod
    def inorm_relu_(x, skip=None, want_stats=False, in_place=True):
        N, H, W, C = x.shape
        r = inorm_ref(x.reshape(N, H * W, C))
        out = inorm_out(x.reshape(N, H * W, C), r, None if skip is None else skip.reshape(N, H * W, C)).reshape(x.shape)
        stats = torch.stack([r["mean"][:, 0], r["rstd"][:, 0]], dim=2)
        return (out, stats) if want_stats else out

    @staticmethod
    def inorm_relu_backward(raw, dy, stats):
        N, H, W, C = raw.shape
        return inorm_bwd_ref(raw.reshape(N, H * W, C), dy.reshape(N, H * W, C), stats[:, None, :, 0], stats[:, None, :, 1])["dx"].reshape(raw.shape)


def test_host_layouts_reproduce_the_oracle(scene, weights, monkeypatch):
    """FeatureNetwork.forward and .backward on the CPU, their kernels replaced by the restatement: the outputs are the oracle's
    fpn_forward and every weight gradient is its autograd's - so the weight layouts the host builds (_pack_conv, _pack_deconv,
    flipT, deconv_dgrad, conv_s2_dgrad, the `finish` permutations) are the ones the restatement's index order means."""
    from surf_amd import conf, ops
    from surf_amd.feature_network import FeatureNetwork
    for name in ("pack_texel4", "conv3x3", "deconv3x3_s2", "conv3x3_wgrad", "inorm_relu_", "inorm_relu_backward"):
        monkeypatch.setattr(ops, name, getattr(_RestatementOps, name))
    net = FeatureNetwork(conf.from_dict({"d_in": 3, "d_base": 8, "d_out": [4, 4, 4, 4]}))
    prefix = "feature_network."
    net.load_state_dict({k[len(prefix):]: v for k, v in weights.items() if k.startswith(prefix)}, strict=True)
    tape = []
    outs = net(scene["imgs"], tape)
    sd = {k: v.to(F64).clone().requires_grad_(True) for k, v in weights.items() if k.startswith(prefix)}
    refs = O.fpn_forward(sd, scene["imgs"].to(F64))
    g = _gen("fpn backward")
    g_outs = [torch.randn(o.shape, generator=g, dtype=F64) for o in outs]
    for o, ref in zip(outs, refs):
        _close(_nchw(o), ref.detach(), 1e-10)
    sum((_nchw(go) * ref).sum() for go, ref in zip(g_outs, refs)).backward()
    net.backward(tape, g_outs)
    for k, p in net.named_parameters():
        ref = sd[prefix + k].grad
        assert p.grad is not None and float((p.grad.to(F64) - ref).abs().max()) <= 1e-6 * (1 + float(ref.abs().max())), k


# ------------------------------------------------------------------------------------------------------------------
# A. the conditions the input sets meet
# ------------------------------------------------------------------------------------------------------------------


def _tiles(mode, shape):
    """-> (outputs, number of 32-pixel tiles that hold pixels of two images)"""
    N, H, W = shape
    Ho, Wo = out_size(mode, H, W)
    total = N * Ho * Wo
    img = torch.arange(total) // (Ho * Wo)
    return total, sum(int(img[t] != img[min(t + 31, total - 1)]) for t in range(0, total, 32))


def test_conv_input_sets_meet_their_conditions():
    for mode in (1, 2, UP):
        counts, straddle, partial = set(), 0, 0
        for shape in shapes_for(mode):
            assert mode != 2 or (shape[1] % 2 == 0 and shape[2] % 2 == 0)
            cnt = tap_count(mode, shape)
            assert int(cnt.min()) >= 1
            counts |= set(cnt.reshape(-1).tolist())
            total, two = _tiles(mode, shape)
            straddle += two
            partial += int(total % 32 != 0)
        # corner, edge and interior outputs; the transposed outputs' four parity classes 1, 2, 2, 4
        assert ({1, 2, 4} if mode == UP else {4, 6, 9}) <= counts, (mode, counts)
        assert straddle > 0 and partial > 0, mode                       # a tile of two images; a lane with i >= total
        total = _tiles(mode, DEAD[mode])[0]
        assert 1 <= total % 128 <= 32                                   # the last workgroup's waves 1 - 3 are dead
    cnt = tap_count(UP, (3, 5, 7))
    par = {(y % 2, x % 2): int(cnt[y, x]) for y in (2, 3) for x in (2, 3)}
    assert par == {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}
    # H = 1 (W = 1): no output of the whole map has a source for ky != 1 (kx != 1): any == false for six taps of every wave
    for mode in (1, UP):
        for shape, axis in (((2, 1, 38), 0), ((3, 6, 1), 1), ((1, 1, 1), 0)):
            n_in = shape[1 + axis]
            n_out = out_size(mode, shape[1], shape[2])[axis]
            if mode == 1:
                assert not bool(_axis(n_out, n_in, 1, 0)[1].any()) and not bool(_axis(n_out, n_in, 1, 2)[1].any())
            else:
                assert not bool(_axis(n_out, n_in, UP, 0)[1].any())     # (transposed: tap 0 would read row 1)


def test_inorm_input_sets_meet_their_conditions():
    for C in INORM_CHANNELS:
        G = 256 // C
        assert inorm_sizes(C) == [1, G - 1, 1023, 1024, 1025, 4 * G + 3, 2049]
        worst = 0.0
        for kind, HW, N in inorm_cases(C):
            c = inorm_case(kind, C, HW, N)
            r = inorm_ref(c["x"])
            ratio = float((r["slack_rstd"] / ulp32(r["rstd"])).max())
            worst = max(worst, ratio)
            assert ratio <= 0.2, (kind, C, HW, N, ratio)                 # the pivoted float64 sums can meet the rstd bound
            if kind in LARGE:
                mean, spread = LARGE[kind][:2]
                assert float(c["x"].max()) <= mean + 6 * spread and float(r["var"].max()) < (1.5 * spread) ** 2
        print(f"InstanceNorm C={C}: float64 slack of rstd / ulp = {worst:.3g}")
    assert (BIG_MAP[0] + 1023) // 1024 > 64 and (LARGE["large66048"][2] + 1023) // 1024 > 64      # statistics blocks
    for C in INORM_BWD_CHANNELS:
        for hw in inorm_bwd_sizes(C):
            for N in (1, 3):
                c = inorm_bwd_case(C, hw, N)
                r = inorm_bwd_ref(c["x"], c["dy"], c["mean"], c["rstd"])
                xh32 = (c["x"] - c["mean"]) * c["rstd"]                 # the kernel's own float32 expression
                assert torch.equal(xh32 > 0, r["xh"] > 0) and torch.equal(xh32 == 0, r["xh"] == 0), (C, hw, N)
                planted = int((r["xh"] == 0).sum())
                assert planted >= (2 * N if hw >= 5 else 0), (C, hw, N, planted)
                if hw >= 5:
                    assert float(c["dy"][:, 2, :2].abs().min()) > 0
        assert min(-(-4097 * 64 // 256), 1024) * (256 // 64) < 4097      # 1,024 workgroups x G rows < 4,097: a second trip


def test_wgrad_input_sets_meet_their_conditions():
    totals = [N * Hs * Ws for N, Hs, Ws in WGRAD_TOTALS]
    assert totals == [1, 63, 65, 255, 257, 2047, 2049]
    big = WGRAD_BIG[0] * WGRAD_BIG[1] * WGRAD_BIG[2]
    nchunk = -(-big // 2048)
    assert big > 8 * 2048 and nchunk == 9                                # finalise: pairs (b, b + 4) and a tail (b = 8)
    assert [(-(-t // 2048)) for t in totals[-2:]] == [1, 2]              # odd and even chunk counts
    assert any(t % 256 and t % 64 for t in totals)                       # a partial staging round of either size
    N, Hs, Ws = WGRAD_TOTALS[-1]
    assert N > 1 and Hs * Ws < 2048 < N * Hs * Ws                        # a chunk spans two images
    N, Hs, Ws = WGRAD_TOTALS[-2]
    assert Ws < 2048 and Hs > 1                                          # a chunk spans two rows
    assert any(Hs % 4 for _, Hs, _ in WGRAD_MFMA_SHAPES) and any(Ws % 16 for _, _, Ws in WGRAD_MFMA_SHAPES)
    assert {(Hs, Ws) for _, Hs, Ws in WGRAD_MFMA_SHAPES} == {(h, w) for h in (1, 4, 5) for w in (1, 15, 16, 17, 33)}
    for cb, cs, S in WGRAD_BIG_CASES:
        assert (cb, cs, S) in WGRAD_CASES
    assert [(cb // 4) * (cs // 2) for cb, cs, _ in WGRAD_BIG_CASES] == [512, 256, 4]
    assert sorted(WGRAD_MFMA + WGRAD_THIN) == sorted(WGRAD_CASES)
    P = wgrad_pixels(1, 1, 1, 1)
    assert float(P[1, 1]) == 1 and float(P.sum()) == 1                   # one pixel: eight taps are all padding


# ------------------------------------------------------------------------------------------------------------------
# A. emulated wrong kernels against the assertions of parts B-E
# ------------------------------------------------------------------------------------------------------------------


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_sensitivity_wrong_sources_and_layouts():
    """No parity test in the transposed convolution, a border tap clamped, the images' rows run together, [co][ci] weights."""
    for mut, cin, cout, mode, shapes in (("no_parity", 16, 8, UP, shapes_for(UP)), ("clamp", 8, 8, 1, shapes_for(1)),
                                         ("clamp", 8, 16, 2, shapes_for(2)), ("wrap", 8, 8, 1, [(3, 5, 7), (3, 6, 10), (2, 22, 38)]),
                                         ("wrap", 8, 16, 2, [(3, 6, 10), (2, 22, 38)]), ("swap", 8, 8, 1, shapes_for(1)),
                                         ("swap", 32, 32, 1, shapes_for(1))):
        for shape in shapes:
            c = conv_case(cin, cout, mode, shape)
            assert check_conv(cin, cout, mode, shape, conv_ref(c["x"], c["w"], mode, F32), "valu") <= 1.0
            bad = conv_ref(c["x"], c["w"], mode, mut=mut).to(F32)
            assert _rejected(lambda: check_conv(cin, cout, mode, shape, bad, "valu")), (mut, cin, cout, mode, shape)


def test_sensitivity_weight_gradient_drops():
    """The last partial 16-pixel k-step of a row dropped; the rows of the last partial group of four dropped."""
    for cb, cs, S in ((16, 16, 1), (8, 16, 2)):
        for shape in WGRAD_MFMA_SHAPES:
            _, Hs, Ws = shape
            c = wgrad_case(cb, cs, S, shape)
            assert check_wgrad(cb, cs, S, shape, wgrad_ref(c["big"], c["small"], S, F32), "mfma") <= 1.0
            for cut_rows in (False, True):
                small = c["small"].clone()
                if cut_rows:
                    small[:, Hs // 4 * 4:] = 0.0
                else:
                    small[:, :, Ws // 16 * 16:] = 0.0
                bad = wgrad_ref(c["big"], small, S).to(F32)
                dropped = (Hs % 4 if cut_rows else Ws % 16) != 0
                assert _rejected(lambda: check_wgrad(cb, cs, S, shape, bad, "mfma")) == dropped, (cb, cs, S, shape, cut_rows)


def test_sensitivity_dropped_split_product():
    """One of the six products of the exact bf16x3 form (x1 w1) left out: the rms criterion sees it."""
    for shape in RMS_SHAPES:
        for cin, cout, mode in ((32, 32, 1), (16, 32, 2), (32, 16, UP)):
            c = conv_case(cin, cout, mode, shape)
            r = conv_reference(cin, cout, mode, shape, "fp32")
            xs, ws = _bf16_pieces(c["x"]), _bf16_pieces(c["w"])
            six = sum(conv_ref(xs[a], ws[b], mode) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)))
            assert check_conv(cin, cout, mode, shape, six.to(F32), "mfma", rms=True) <= 1.0
            five = (six - conv_ref(xs[1], ws[1], mode)).to(F32)
            by = rel_rms(five, r["y"], r["B"]) / conv_rms32(cin, cout, mode, shape, "fp32")
            print(f"x1 w1 dropped, ({cin}, {cout}, {mode}) on {shape}: rms {by:.3g} x the float32 evaluation's")
            assert by > 4.0 and _rejected(lambda: check_conv(cin, cout, mode, shape, five, "mfma", rms=True))
    for shape in ((2, 4, 33), (2, 5, 33)):
        cb, cs, S = 16, 32, 2
        c = wgrad_case(cb, cs, S, shape)
        bs, ss = _bf16_pieces(c["big"]), _bf16_pieces(c["small"])
        six = sum(wgrad_ref(bs[a], ss[b], S) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)))
        assert check_wgrad(cb, cs, S, shape, six.to(F32), "mfma", rms=True) <= 1.0
        five = (six - wgrad_ref(bs[1], ss[1], S)).to(F32)
        assert _rejected(lambda: check_wgrad(cb, cs, S, shape, five, "mfma", rms=True)), shape


def _as_kernel(x, skip, r, before_relu=False):
    """What a float32 kernel with the statistics r would hand to check_inorm."""
    mean, rstd = r["mean"].to(F32), r["rstd"].to(F32)
    own = torch.clamp_min((x - mean) * rstd, 0.0)
    if before_relu:
        own = torch.clamp_min((x - mean) * rstd + skip, 0.0)
    elif skip is not None:
        own = own + skip
    return mean, rstd, own


def test_sensitivity_instance_norm():
    """Unbiased variance, eps = 1e-6, the skip added before the ReLU, var = E[x^2] - mean^2 of x itself on the large-mean
    inputs, a backward gate of >=."""
    for C in (8, 64):
        for kind, HW, N in inorm_cases(C):
            c = inorm_case(kind, C, HW, N)
            x, skip = c["x"], c["skip"]
            r = inorm_ref(x)
            what = ("emulated", kind, C, HW, N)
            assert check_inorm(what, x, skip, r, *_as_kernel(x, skip, r))[0] <= 1.0
            muts = (["unbiased"] if 1 < HW <= 2049 else []) + (["eps6"] if HW > 1 and kind == "normal" else []) + (["raw"] if kind in LARGE else [])
            for mut in muts:
                bad = inorm_ref(x, mut)
                assert _rejected(lambda: check_inorm(what, x, skip, r, *_as_kernel(x, skip, bad))), (mut,) + what
                if mut == "raw":
                    print(f"{kind}: E[x^2] - mean^2 in float64 puts rstd off by "
                          f"{float(((bad['rstd'] - r['rstd']).abs() / ulp32(r['rstd'])).max()):.3g} float32 ulp")
            if HW > 1:
                assert _rejected(lambda: check_inorm(what, x, skip, r, *_as_kernel(x, skip, r, before_relu=True))), what
    for C in INORM_BWD_CHANNELS:
        for hw in inorm_bwd_sizes(C):
            c = inorm_bwd_case(C, hw, 3)
            good = inorm_bwd_ref(c["x"], c["dy"], c["mean"], c["rstd"])
            assert check_inorm_bwd(C, hw, 3, good["dx"].to(F32)) <= 1.0
            if hw >= 5:
                bad = inorm_bwd_ref(c["x"], c["dy"], c["mean"], c["rstd"], gate_ge=True)["dx"].to(F32)
                assert _rejected(lambda: check_inorm_bwd(C, hw, 3, bad)), (C, hw)


# ------------------------------------------------------------------------------------------------------------------
# A. the measured margins of the module docstring
# ------------------------------------------------------------------------------------------------------------------


def _recorded(label):
    m = re.search(rf"^\s+{re.escape(label)}\s+(\S+) \.\. (\S+)$", __doc__, re.M)
    return float(m.group(1)), float(m.group(2))


def measured_rms():
    out = {}
    every = CONV_CASES + [(ci, co, UP) for ci, co in DECONV_CASES]
    for shape in RMS_SHAPES:
        for variant, cases in (("fp32", every), ("bf16", MFMA_CASES)):
            v = [conv_rms32(ci, co, m, shape, variant) for ci, co, m in cases]
            out[f"conv {variant} {shape}"] = (min(v), max(v))
    for shape in WGRAD_RMS[:3]:
        v = [wgrad_rms32(cb, cs, S, shape, "fp32") for cb, cs, S in (WGRAD_BIG_CASES if shape == WGRAD_BIG else WGRAD_CASES)]
        out[f"wgrad fp32 {shape[0] * shape[1] * shape[2]}"] = (min(v), max(v))
    for variant in ("fp32", "bf16"):
        v = [wgrad_rms32(cb, cs, S, shape, variant) for cb, cs, S in WGRAD_CASES for shape in WGRAD_RMS[3:]]
        out[f"wgrad {variant} mfma shapes"] = (min(v), max(v))
    return out


def test_measured_margins_are_recorded():
    """The rms lines of the module docstring are the ones these inputs give (the float32 evaluation adds one term at a time, so
    they do not depend on a BLAS; 10 % of slack for a platform's float64 matmul behind the reference)."""
    measured = measured_rms()
    for label, (lo, hi) in measured.items():
        print(f"    {label:<27s} {lo:.1e} .. {hi:.1e}")
    for label, (lo, hi) in measured.items():
        rlo, rhi = _recorded(label)
        assert abs(lo / rlo - 1.0) < 0.1 and abs(hi / rhi - 1.0) < 0.1, (label, lo, hi)


# ------------------------------------------------------------------------------------------------------------------
# GPU side: guarded buffers, the entry points
# ------------------------------------------------------------------------------------------------------------------

GUARD = 256          # elements of sentinel on either side of an output or a workspace


def _guarded(n, dtype=F32, fill=SENTINEL):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
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


def run_conv(x, w, mode, cout, precision, valu):
    """surf_conv3x3_p / surf_deconv3x3_s2_p into a guarded buffer -> (N, Ho, Wo, cout) on the CPU."""
    from surf_amd import _lib, ops
    L, p, s = _lib.lib(), ops._p, ops._stream
    N, H, W, cin = x.shape
    Ho, Wo = out_size(mode, H, W)
    n = N * Ho * Wo * cout
    buf, out = _guarded(n)

    def call():
        if mode == UP:
            L.surf_deconv3x3_s2_p(p(x), p(w), N, H, W, cin, cout, p(out), precision, s())
        else:
            L.surf_conv3x3_p(p(x), p(w), N, H, W, cin, cout, mode, p(out), precision, s())
    _env("SURF_FPN_VALU", call) if valu else call()
    _intact(buf, n, ("conv", cin, cout, mode, (N, H, W)))
    return out.cpu().reshape(N, Ho, Wo, cout)


def run_wgrad(big, small, S, precision, switch):
    """surf_conv3x3_wgrad_p, output and workspace (sized exactly by surf_conv3x3_wgrad_workspace_floats) guarded."""
    from surf_amd import _lib, ops
    L, p, s = _lib.lib(), ops._p, ops._stream
    N, Hs, Ws, cs = small.shape
    cb = big.shape[3]
    nws = int(L.surf_conv3x3_wgrad_workspace_floats(N, Hs, Ws, cb, cs))
    wbuf, ws = _guarded(nws)
    obuf, out = _guarded(9 * cb * cs)

    def call():
        L.surf_conv3x3_wgrad_p(p(big), p(small), N, Hs, Ws, cb, cs, S, p(ws), p(out), precision, s())
    _env(switch, call) if switch else call()
    _intact(wbuf, nws, ("wgrad workspace", cb, cs, S, (N, Hs, Ws)))
    _intact(obuf, 9 * cb * cs, ("wgrad", cb, cs, S, (N, Hs, Ws)))
    return out.cpu().reshape(3, 3, cb, cs)


# ------------------------------------------------------------------------------------------------------------------
# B. forward and input-gradient convolutions
# ------------------------------------------------------------------------------------------------------------------


def _conv_valu(cin, cout, mode):
    worst = 0.0
    for shape in shapes_for(mode):
        c = conv_case(cin, cout, mode, shape)
        got = run_conv(c["x"].to(dev()), c["w"].to(dev()), mode, cout, 0, valu=True)
        worst = max(worst, check_conv(cin, cout, mode, shape, got, "valu", rms=shape in RMS_SHAPES))
    print(f"({cin}, {cout}, {mode}) VALU: worst |error| / bound {worst:.3g}")


@gpu
@pytest.mark.parametrize("cin,cout,stride", CONV_CASES)
def test_conv_valu_per_element(cin, cout, stride):
    """conv3x3_kernel, every instantiated pair: maps of 1 x 1 to 22 x 38, tiles of two images, a partial last wave, dead waves."""
    _conv_valu(cin, cout, stride)


@gpu
@pytest.mark.parametrize("cin,cout", DECONV_CASES)
def test_deconv_valu_per_element(cin, cout):
    """deconv3x3_s2_kernel, every instantiated pair, the four parity classes at every border."""
    _conv_valu(cin, cout, UP)


@gpu
@pytest.mark.parametrize("cin,cout,mode", MFMA_CASES)
def test_conv_mfma_per_element(cin, cout, mode):
    """conv3x3_mfma_kernel, exact bf16x3 and one product: the same shapes - among them whole waves without a source for six of
    the nine taps, tiles of two images, lanes beyond the last output, three dead waves in the last workgroup."""
    from surf_amd import ops
    d, worst = dev(), {}
    for shape in shapes_for(mode):
        c = conv_case(cin, cout, mode, shape)
        x, w = c["x"].to(d), c["w"].to(d)
        for precision, path in ((0, "mfma"), (1, "bf16")):
            got = run_conv(x, w, mode, cout, precision, valu=False)
            worst[path] = max(worst.get(path, 0.0), check_conv(cin, cout, mode, shape, got, path, rms=shape in RMS_SHAPES))
            via_ops = ops.deconv3x3_s2(x, w, cout, precision) if mode == UP else ops.conv3x3(x, w, cout, mode, precision)
            assert torch.equal(via_ops.cpu(), got)
        if shape == RMS_SHAPES[0]:                                       # ... and precision 1 really is another kernel
            assert not torch.equal(got, run_conv(x, w, mode, cout, 1, valu=True))
    print(f"({cin}, {cout}, {mode}) matrix cores: worst |error| / bound {worst}")


# ------------------------------------------------------------------------------------------------------------------
# C. InstanceNorm forward and backward
# ------------------------------------------------------------------------------------------------------------------


def run_inorm(x, skip, in_place):
    """surf_inorm_relu (in place) / surf_inorm_relu_out with guarded statistics, workspace and output.  x (N, HW, C) on the
    device -> (mean, rstd (N, 1, C), out (N, HW, C)) on the CPU."""
    from surf_amd import _lib, ops
    L, p, s = _lib.lib(), ops._p, ops._stream
    N, HW, C = x.shape
    H, W = (HW // 3, 3) if HW % 3 == 0 else (1, HW)
    nws = int(L.surf_inorm_workspace_doubles(N, H, W, C))
    assert nws == N * ((HW + 1023) // 1024) * C * 2
    wbuf, ws = _guarded(nws, F64)
    sbuf, stats = _guarded(N * C * 2)
    obuf, out = _guarded(x.numel())
    if in_place:
        out.copy_(x.reshape(-1))
        L.surf_inorm_relu(p(out), N, H, W, C, p(skip), p(ws), p(stats), s())
    else:
        keep = x.clone()
        L.surf_inorm_relu_out(p(x), N, H, W, C, p(skip), p(ws), p(stats), p(out), s())
        assert torch.equal(x, keep)
    for b, n, what in ((wbuf, nws, "workspace"), (sbuf, N * C * 2, "statistics"), (obuf, x.numel(), "output")):
        _intact(b, n, ("InstanceNorm " + what, C, HW, N))
    st = stats.cpu().reshape(N, C, 2)
    return st[:, None, :, 0].clone(), st[:, None, :, 1].clone(), out.cpu().reshape(N, HW, C)


@gpu
@pytest.mark.parametrize("C", INORM_CHANNELS)
def test_inorm_forward(C):
    """inorm_partial_kernel, inorm_finalize_kernel, inorm_relu_kernel: 1 to 2,049 pixels around the 1,024-pixel statistics block
    and the 4 G unrolling, one and three images, in place and out of place, with and without skip, means of 0, 300 (c + 1) and
    - for C = 8 and 64 - 10^5 x the spread; C = 8 also 65 statistics blocks.  Statistics and output per element."""
    from surf_amd import ops
    d, worst, ulps = dev(), 0.0, {}
    for kind, HW, N in inorm_cases(C):
        c = inorm_case(kind, C, HW, N)
        r = inorm_ref(c["x"])
        x, skip = c["x"].to(d), c["skip"].to(d)
        for in_place, sk in ((False, skip), (True, None), (True, skip), (False, None)):
            mean, rstd, out = run_inorm(x, sk, in_place)
            w, ulp = check_inorm((kind, C, HW, N, in_place, sk is not None), c["x"], None if sk is None else c["skip"], r, mean, rstd, out)
            worst, ulps[kind] = max(worst, w), max(ulps.get(kind, 0.0), ulp)
        x4 = x.reshape(N, 1, HW, C)
        o, st = ops.inorm_relu_(x4.clone(), skip=skip.reshape(x4.shape), want_stats=True, in_place=False)
        assert torch.equal(o.cpu().reshape(N, HW, C), out + c["skip"]) and torch.equal(st.cpu()[:, None, :, 1], rstd)
        assert torch.equal(ops.inorm_relu_(x4.clone()).cpu().reshape(N, HW, C), out)
    print(f"InstanceNorm C={C}: worst |error| / bound {worst:.3g}; worst rstd error in float32 ulp per input kind {ulps}")


@gpu
@pytest.mark.parametrize("C", INORM_BWD_CHANNELS)
def test_inorm_backward(C):
    """surf_inorm_relu_backward at 1, 5 and 1,025 pixels, one and three views, elements with xhat = 0 exactly; C = 64 also 4,097
    pixels: the 1,024 workgroups x 4 rows of inorm_bwd_partial_kernel take a second trip."""
    from surf_amd import _lib, ops
    L, p, s, d, worst = _lib.lib(), ops._p, ops._stream, dev(), 0.0
    for hw in inorm_bwd_sizes(C):
        for N in (1, 3):
            c = inorm_bwd_case(C, hw, N)
            x, dy = c["x"].to(d), c["dy"].to(d)
            stats = torch.stack([c["mean"][:, 0], c["rstd"][:, 0]], dim=2).contiguous().to(d)
            nws = int(L.surf_inorm_backward_workspace_bytes(N, C))
            wbuf, ws = _guarded(nws, torch.uint8, 0xA5)
            obuf, dx = _guarded(x.numel())
            L.surf_inorm_relu_backward(p(x), p(dy), N, hw, C, p(stats), p(ws), p(dx), s())
            _intact(wbuf, nws, ("InstanceNorm backward workspace", C, hw, N), 0xA5)
            _intact(obuf, x.numel(), ("InstanceNorm backward", C, hw, N))
            got = dx.cpu().reshape(N, hw, C)
            worst = max(worst, check_inorm_bwd(C, hw, N, got))
            via_ops = ops.inorm_relu_backward(x.reshape(N, 1, hw, C), dy.reshape(N, 1, hw, C), stats)
            assert torch.equal(via_ops.cpu().reshape(N, hw, C), got)
    print(f"InstanceNorm backward C={C}: worst |error| / bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------------------------
# D. weight gradients
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("cb,cs,S", WGRAD_CASES)
def test_wgrad_valu_per_element(cb, cs, S):
    """wgrad_kernel + wgrad_finalize_kernel (one and two chunks), every instantiated triple, 1 to 2,049 pixels: partial 256- and
    64-pixel staging rounds, a chunk that spans rows and images, taps that are all padding."""
    d, worst = dev(), 0.0
    for shape in WGRAD_TOTALS:
        c = wgrad_case(cb, cs, S, shape)
        got = run_wgrad(c["big"].to(d), c["small"].to(d), S, 0, "SURF_FPN_VALU")
        worst = max(worst, check_wgrad(cb, cs, S, shape, got, "valu", rms=shape in WGRAD_RMS))
    print(f"wgrad ({cb}, {cs}, {S}) VALU: worst |error| / bound {worst:.3g}")


@gpu
@pytest.mark.parametrize("cb,cs,S", WGRAD_BIG_CASES)
def test_wgrad_valu_many_chunks(cb, cs, S):
    """16,641 pixels = 9 chunks: wgrad_finalize_kernel's paired loop and its tail; 512, 256 and 4 register blocks per tap."""
    c = wgrad_case(cb, cs, S, WGRAD_BIG)
    got = run_wgrad(c["big"].to(dev()), c["small"].to(dev()), S, 0, "SURF_FPN_VALU")
    print(f"wgrad ({cb}, {cs}, {S}) VALU, 9 chunks: worst |error| / bound {check_wgrad(cb, cs, S, WGRAD_BIG, got, 'valu', rms=True):.3g}")


@gpu
@pytest.mark.parametrize("cb,cs,S", WGRAD_MFMA + WGRAD_THIN)
def test_wgrad_mfma_per_element(cb, cs, S):
    """wgrad_mfma_kernel, exact bf16x3 and one product, the dispatched triples and (under SURF_FPN_WGRAD_THIN_MFMA) the thin
    ones: rows of 1 to 33 pixels (partial 16-pixel k-steps), 1, 4 and 5 rows (a partial group of four), one and two images."""
    from surf_amd import ops
    d, worst = dev(), {}
    switch = "SURF_FPN_WGRAD_THIN_MFMA" if (cb, cs, S) in WGRAD_THIN else None
    for shape in WGRAD_MFMA_SHAPES:
        c = wgrad_case(cb, cs, S, shape)
        big, small = c["big"].to(d), c["small"].to(d)
        for precision, path in ((0, "mfma"), (1, "bf16")):
            got = run_wgrad(big, small, S, precision, switch)
            worst[path] = max(worst.get(path, 0.0), check_wgrad(cb, cs, S, shape, got, path, rms=shape in WGRAD_RMS))
        if shape == WGRAD_MFMA_SHAPES[-1]:                                # precision 1 really ran on the matrix cores
            assert not torch.equal(got, run_wgrad(big, small, S, 1, "SURF_FPN_VALU"))
            if switch is None:
                assert torch.equal(ops.conv3x3_wgrad(big, small, S, 1).cpu(), got)
    print(f"wgrad ({cb}, {cs}, {S}) matrix cores: worst |error| / bound {worst}")


# ------------------------------------------------------------------------------------------------------------------
# E. argument checks
# ------------------------------------------------------------------------------------------------------------------


@gpu
def test_argument_checks_raise_and_launch_nothing():
    """Stride 2 with an odd side, a channel pair without a kernel, precision 2, C = 12: SurfHipError, the output untouched."""
    from surf_amd import _lib, ops
    L, p, s, d = _lib.lib(), ops._p, ops._stream, dev()
    x = torch.randn(1, 6, 5, 8, device=d)
    w = torch.randn(3, 3, 8, 32, device=d)
    buf, out = _guarded(4096)
    ws = torch.empty(4096, dtype=F64, device=d)
    stats = torch.empty(64, device=d)
    for kind, call in (("invalid argument", lambda: L.surf_conv3x3_p(p(x), p(w), 1, 6, 5, 8, 16, 2, p(out), 0, s())),
                       ("invalid argument", lambda: L.surf_conv3x3_p(p(x), p(w), 1, 5, 6, 8, 16, 2, p(out), 0, s())),
                       ("exceeds", lambda: L.surf_conv3x3_p(p(x), p(w), 1, 6, 5, 8, 32, 1, p(out), 0, s())),
                       ("exceeds", lambda: L.surf_deconv3x3_s2_p(p(x), p(w), 1, 6, 5, 8, 32, p(out), 0, s())),
                       ("invalid argument", lambda: L.surf_conv3x3_p(p(x), p(w), 1, 6, 5, 8, 8, 1, p(out), 2, s())),
                       ("invalid argument", lambda: L.surf_deconv3x3_s2_p(p(x), p(w), 1, 6, 5, 16, 8, p(out), 2, s())),
                       ("invalid argument", lambda: L.surf_conv3x3_wgrad_p(p(x), p(x), 1, 6, 5, 8, 8, 1, p(ws), p(out), 2, s())),
                       ("exceeds", lambda: L.surf_conv3x3_wgrad_p(p(x), p(x), 1, 6, 5, 8, 32, 1, p(ws), p(out), 0, s())),
                       ("invalid argument", lambda: L.surf_inorm_relu_out(p(x), 1, 4, 5, 12, None, p(ws), p(stats), p(out), s())),
                       ("invalid argument", lambda: L.surf_inorm_relu(p(out), 1, 4, 5, 12, None, p(ws), p(stats), s()))):
        with pytest.raises(_lib.SurfHipError, match=kind):
            call()
    with pytest.raises(_lib.SurfHipError, match="invalid argument"):
        ops.conv3x3(x, w[..., :16].contiguous(), 16, 2)
    with pytest.raises(ValueError):
        ops.inorm_relu_(torch.randn(1, 4, 5, 12, device=d))
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENTINEL).all())
