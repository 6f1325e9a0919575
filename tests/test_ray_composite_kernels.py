"""The two per-ray kernels at either end of the render path, each fed directly at ragged sizes: surf_ray_setup
(csrc/ray_setup.hip), surf_composite (csrc/composite.hip), surf_composite_backward[_s] (csrc/composite_bwd.hip), and
surf_pack_texel4.

Part A (no GPU): a float64 restatement of the ray set-up, of the compositing forward (all eleven outputs) and of its backward,
written with a `dt` argument so that dt = float32 is the oracle's arithmetic; its anchor to O.ray_zsample / O.render_core on the
golden scene; the conditions every input set of parts B-D has to meet, evaluated from the float64 reference alone; the
sensitivity of the comparator to planted mistakes.  Parts B-E (gpu): the kernels through surf_amd.ops against that restatement.

How a float output is compared.  For each part, output and case, E is the largest |restatement(float32) - restatement(float64)|
over that output on those very inputs, measured on the CPU; the kernel has to stay within 8 E of the float64 values per element
(the 8 allows for the kernel's operation order, the contraction into FMAs and the device's expf / division, as in
test_volume_forward.py).  z_sdf0 is compared relatively (E is the largest relative difference) on rays that have a crossing; on
rays without one only sdf_depth == 0 and mid_inside == 0 are required.  Integer and boolean outputs are compared exactly: the
input conditions keep every selection (|pts| against 1 and 1.2, cosd against 0.5, the sign tests) away from its threshold.

How vmask is compared.  The kernel's own fp32 points are taken; g = ((p + 1) D - 1) / 2 is evaluated per axis and level in
float64.  A sample is UNDECIDED when some g is within EPS_MASK of a half-integer and the levels that are certain do not already
give "occupied"; flags are compared on decided samples.  EPS_MASK is 8 x the largest |g_fp32 - g_float64| on these inputs.

How the backward is compared.  float64 autograd through O.composite_differentiable, one backward pass per ray for d_inv_s.  The
eikonal term's gradient is defined as zero where |grad| = 0 (the kernel's n > 0 guard); the restatement differentiates the
eikonal term on its own and writes zero there, whatever autograd gives.  Samples with a gated argument (r1, r2, ic +- 10, al,
al - 1) closer than 1e-5 to its kink are left out of d_sdf / d_grad; they stay under 1 % of a case's unmasked samples.  r2 = -d . grad
of an all-zero grad is exactly zero in every arithmetic and relu'(0) = 0 in autograd as in the kernel's r2 > 0: that is certain.

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest):
    part B  largest fp32-vs-float64 difference E_SETUP = 1.27e-06    EPS_MASK = 3.10e-05    largest undecided share UNDECIDED = 5.76e-04 (cap 1e-2)
    part C  largest fp32-vs-float64 difference E_FORWARD = 1.14e-03
    part D  largest fp32-vs-float64 difference E_BACKWARD = 1.82e-02    largest left-out share LEFT_OUT = 0.00e+00 (cap 1e-2)
Seen on an MI355X, largest |kernel - float64| / (8 E): part B 0.17 (mid_z, r5-s128-nd33-dm16); part C 0.74 (eik, r1-s193), 0.50 (eik,
r4-s65); part D 0.77 (d_inv_s, r1-s64), 0.48 (d_inv_s, r1-s3); everything else under 0.45.  The four are per-ray sums of a case with
few rays, where E is the fp32 error of a handful of numbers.
"""
import functools
import re
import types

import numpy as np
import pytest
import torch

from oracle import surf_oracle as O
from tests.golden_cfg import CFG, pipeline_views

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
FACTOR = 8.0
KINK = 1e-5


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _s(v, dt):
    """A scalar the kernels take as a C float: float32(v), promoted."""
    return torch.tensor(float(v), dtype=F32).to(dt)


# ------------------------------------------------------------------------------------------------------------------
# the float64 restatement (dt = float64) - the same statements at dt = float32 are the oracle's arithmetic
# ------------------------------------------------------------------------------------------------------------------


def _unnorm(p, D):
    return ((p + 1.0) * D - 1.0) / 2.0


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


def occupancy(pts, tables, eps=0.0):
    """pts (N,3) float64, tables: int tables (D,D,D), -1 = empty, any order, not assumed nested.
    -> (flag, decided): nearest (half-to-even) lookup ORed over the levels, and whether rounding within eps could change it."""
    n = pts.shape[0]
    flag = torch.zeros(n, dtype=torch.bool)
    sure = torch.zeros(n, dtype=torch.bool)
    shaky = torch.zeros(n, dtype=torch.bool)
    for t in tables:
        D = t.shape[0]
        g = _unnorm(pts, D)
        near_half = ((g - torch.floor(g) - 0.5).abs() < eps).any(dim=1) if eps > 0 else torch.zeros(n, dtype=torch.bool)
        i = torch.round(g).long()
        ok = ((i >= 0) & (i < D)).all(dim=1)
        i = i.clamp(0, D - 1)
        v = (t[i[:, 0], i[:, 1], i[:, 2]] >= 0) & ok
        flag |= v
        sure |= v & ~near_half
        shaky |= near_half
    return flag, sure | ~shaky


def ray_setup_ref(c, dt=F64, plant=None):
    """c: a set-up case (rays_o, rays_d (R,3), near, far (R), mvol (Dm,Dm,Dm), tables, n_samples, ranges, n_depth, jitter)."""
    o, d = c["rays_o"].to(dt), c["rays_d"].to(dt)
    near, far = c["near"].to(dt)[:, None], c["far"].to(dt)[:, None]
    ns, rg, nd = c["n_samples"], c["ranges"], c["n_depth"]
    jit = None if c["jitter"] is None else c["jitter"].to(dt)
    lin = lambda n: torch.linspace(0.0, 1.0, int(n), dtype=F32).to(dt)
    zc = near + (far - near) * lin(nd)[None]
    p = o[:, None, :] + d[:, None, :] * zc[..., None]
    rho = _trilinear(c["mvol"].to(dt), _unnorm(p.reshape(-1, 3), c["mvol"].shape[0])).reshape(zc.shape)
    if plant == "drop_partial_trip" and nd % 32:
        rho, zc = rho[:, :32 * (nd // 32)], zc[:, :32 * (nd // 32)]
    zs = (zc * torch.softmax(rho, dim=-1)).sum(dim=1, keepdim=True)
    z0 = near + (far - near) * lin(ns[0])[None]
    if jit is not None:
        z0 = z0 + jit[:, 0:1] * 2.0 / ns[0]
    z_all, hi_fired, lo_fired = [z0], [], []
    for s in range(1, len(ns)):
        half = (far - near) * _s(rg[s], dt)
        a, b = zs - half, zs + half
        hi_fired.append(b - far)
        if plant != "no_hi_shift":
            a = torch.where(b > far, a - (b - far), a)
        lo_fired.append(near - a)
        if plant != "no_lo_shift":
            b = torch.where(a < near, b + (near - a), b)
        a = torch.minimum(torch.maximum(a, near), far)
        b = torch.minimum(torch.maximum(b, near), far)
        zb = a + (b - a) * lin(ns[s])[None]
        if jit is not None:
            zb = zb + (jit[:, s:s + 1] * 2.0 / ns[0] if plant == "jitter_scale" else jit[:, s:s + 1] * (b - a) / ns[s])
        z_all.append(zb)
    z = torch.sort(torch.cat(z_all, dim=-1), dim=-1).values
    R, S = z.shape
    last = z[:, -1:] - z[:, -2:-1] if plant == "last_dist_prev" else _s(2.0 / ns[0], dt).expand(R, 1)
    dists = torch.cat([z[:, 1:] - z[:, :-1], last], dim=-1)
    mid = z + dists * 0.5
    pts = (o[:, None, :] + d[:, None, :] * mid[..., None]).reshape(-1, 3)
    tabs = c["tables"]
    if plant == "or_smallest_only":
        tabs = [min(tabs, key=lambda t: t.shape[0])]
    vmask, _ = occupancy(pts.to(F64), tabs)
    return {"z_vals": z, "mid_z": mid, "dists": dists, "pts": pts, "vmask": vmask, "surf_z": zs,
            "hi_fired": hi_fired, "lo_fired": lo_fired}


def _lanes(S):
    P = (S + 63) // 64
    return P, torch.arange(S) // P


def composite_ref(c, dt=F64, plant=None):
    """c: a compositing case: sdf, mid_z, dists (R,S), grad, color, pts (R,S,3), n_valid (R,S) uint8, vmask (R,S) bool,
    rays_d (R,3), rot (3,3), inv_s, anneal.  Masked-out rows of sdf / grad / color / n_valid are never read."""
    vm = c["vmask"]
    R, S = vm.shape
    vmf = vm.to(dt)
    sdf = torch.where(vm, c["sdf"].to(dt), torch.full((R, S), 100.0, dtype=dt))
    g3 = torch.where(vm[..., None], c["grad"].to(dt), torch.zeros(R, S, 3, dtype=dt))
    col = torch.where(vm[..., None], c["color"].to(dt), torch.zeros(R, S, 3, dtype=dt))
    nv = torch.where(vm, c["n_valid"], torch.zeros_like(c["n_valid"]))
    mid, dists, pts, d = c["mid_z"].to(dt), c["dists"].to(dt), c["pts"].to(dt), c["rays_d"].to(dt)
    rot, inv_s, A = c["rot"].to(dt), _s(c["inv_s"], dt), _s(c["anneal"], dt)
    tc = (d[:, None, :] * g3).sum(-1)
    ic = -(torch.relu(-tc * 0.5 + 0.5) * (1.0 - A) + torch.relu(-tc) * A) * vmf
    half = ic.clamp(-10.0, 10.0) * dists * 0.5
    pc, nc = torch.sigmoid((sdf - half) * inv_s), torch.sigmoid((sdf + half) * inv_s)
    e5 = 0.0 if plant == "no_1e-5" else 1e-5
    al = (pc - nc + e5) / (pc + 1e-5)
    alpha = al.clamp(0.0, 1.0) * vmf
    pn = torch.linalg.norm(pts, dim=-1)
    inside = (pn < 1.0).to(dt) * vmf
    relax = inside if plant == "inside_for_relax" else (pn < 1.2).to(dt) * vmf
    f = 1.0 - alpha + (0.0 if plant == "no_1e-7" else 1e-7)
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dt), f], dim=-1), dim=-1)[:, :-1]
    P, lane = _lanes(S)
    if plant == "inclusive_T":          # the scan's inclusive value handed to the lane itself: its whole run is in T already
        run = torch.ones(R, S, dtype=dt)
        for l in range(int(lane.max()) + 1):
            if l > 0:
                run[:, lane == l] = f[:, lane == l].prod(dim=1, keepdim=True)
        T = T * run
    w = alpha * T
    color = (col * w[..., None]).sum(dim=1)
    nsum = (g3 * w[..., None]).sum(dim=1)
    normal = nsum @ rot.t()
    normal_val = (g3 * (w * inside)[..., None]).sum(dim=1)
    cz = (d @ rot.t())[:, 2]
    depth = (mid * w).sum(dim=1) * cz
    gn = torch.linalg.norm(g3, dim=-1) - 1.0
    eik = torch.stack([(relax * gn * gn).sum(dim=1), relax.sum(dim=1)], dim=1)
    valid = ((nv > 1).sum(dim=1, keepdim=True) > 8)
    # first zero crossing
    nxt_s, nxt_m = sdf[:, 1:], vm[:, 1:]
    if plant == "neighbour_same_lane":  # the run's last sample looks at its own lane's first sample
        k = torch.arange(S - 1)
        src = torch.where(k % P == P - 1, k - (P - 1), k + 1)
        nxt_s, nxt_m = sdf[:, src], vm[:, src]
    sign = ((sdf[:, :-1] * nxt_s) <= 0) & vm[:, :-1] & nxt_m
    any_ = sign.any(dim=1)
    order = torch.arange(1, S) if plant == "last_crossing" else torch.arange(S - 1, 0, -1)
    pi = torch.argmax(sign.long() * order[None], dim=1, keepdim=True)
    ni = pi + 1
    mis = ((0.5 * (inside.gather(1, pi) + inside.gather(1, ni))) > 0.5) & any_[:, None]
    g1 = g3.gather(1, pi[..., None].expand(-1, -1, 3))[:, 0]
    g2 = g3.gather(1, ni[..., None].expand(-1, -1, 3))[:, 0]
    cosd = (g1 * g2).sum(-1) / (torch.linalg.norm(g1, dim=-1) * torch.linalg.norm(g2, dim=-1) + 1e-8)
    mis = mis & (cosd > 0.5)[:, None]
    s1, s2 = sdf.gather(1, pi), sdf.gather(1, ni)
    z1, z2 = mid.gather(1, pi), mid.gather(1, ni)
    z0 = (s1 * z2 - s2 * z1) / (s1 - s2 + 1e-10)
    return {"color_fine": color, "render_depth": depth, "sdf_depth": z0 * cz[:, None] * mis.to(dt), "normal": normal,
            "normal_val": normal_val, "valid_mask": valid, "mid_inside_sphere": mis, "weights": w, "inside_sphere": inside,
            "eik": eik, "z_sdf0": z0[:, 0],
            "_k": torch.where(any_, pi[:, 0], torch.full((R,), -1)), "_cosd": cosd, "_al": al, "_pn": pn, "_sdf": sdf,
            "_tc": tc, "_ic": ic, "_alpha": alpha}


FWD_FLOAT = ("color_fine", "render_depth", "sdf_depth", "normal", "normal_val", "weights", "eik")
FWD_EXACT = ("valid_mask", "mid_inside_sphere", "inside_sphere")


def _bwd_inputs(c, dt):
    vm = c["vmask"].reshape(-1)
    vmf = vm.to(dt)
    sdf = torch.where(vm, c["sdf"].reshape(-1).to(dt), torch.full_like(vmf, 100.0))
    grad = torch.where(vm[:, None], c["grad"].reshape(-1, 3).to(dt), torch.zeros(vm.numel(), 3, dtype=dt))
    col = torch.where(vm[:, None], c["color"].reshape(-1, 3).to(dt), torch.zeros(vm.numel(), 3, dtype=dt))
    return vm, vmf, sdf, grad, col


def composite_bwd_autograd(c, dt=F64):
    """Autograd through O.composite_differentiable with the masked rows prepared as test_composite_backward_matches_autograd does
    (sdf 100, grad 0).  -> d_sdf (R,S), d_grad, d_color (R,S,3), d_inv_s (R): each ray's own loss term differentiated."""
    R, S = c["vmask"].shape
    vm, vmf, sdf, grad, col = _bwd_inputs(c, dt)
    x_sdf, x_grad, x_col = sdf.requires_grad_(True), grad.requires_grad_(True), col.requires_grad_(True)
    x_is = _s(c["inv_s"], dt).requires_grad_(True)
    mid, dists, pts, d = c["mid_z"].to(dt), c["dists"].to(dt), c["pts"].reshape(-1, 3).to(dt), c["rays_d"].to(dt)
    color, depth, gerr = O.composite_differentiable(x_sdf, x_grad, x_col, vmf, mid, dists, pts, d, x_is, float(_s(c["anneal"], F64)),
                                                    c["rot"].to(dt))
    per_ray = (color * c["g_color"].to(dt)).sum(dim=1)
    if c["g_depth"] is not None:
        per_ray = per_ray + depth * c["g_depth"].to(dt)
    d_is = torch.stack([torch.autograd.grad(per_ray[r], x_is, retain_graph=True)[0] for r in range(R)])
    d_sdf, d_grad, d_col = torch.autograd.grad(per_ray.sum(), (x_sdf, x_grad, x_col), retain_graph=True)
    if c["eik_scale"] != 0.0:
        relax = (torch.linalg.norm(pts, dim=-1) < 1.2).to(dt) * vmf
        g_eik = _s(c["eik_scale"], dt) * (relax.sum() + 1e-5)                  # so that eik_scale is the kernel's argument
        e_grad, = torch.autograd.grad(gerr * g_eik, x_grad)
        zero = (grad.detach() == 0).all(dim=1)
        e_grad = torch.where(zero[:, None], torch.zeros_like(e_grad), e_grad)  # defined as zero at |grad| = 0, whatever autograd gives
        d_grad = d_grad + e_grad
    return {"d_sdf": d_sdf.detach().view(R, S), "d_grad": d_grad.detach().view(R, S, 3), "d_color": d_col.detach().view(R, S, 3),
            "d_inv_s": d_is.detach()}


def composite_bwd_ref(c, dt=F64, plant=None):
    """The backward in closed form (the kernel's header formulas), for planting mistakes; pinned to the autograd above."""
    vm = c["vmask"]
    R, S = vm.shape
    _, vmf, sdf, g3, col = _bwd_inputs(c, dt)
    vmf, sdf, g3, col = vmf.view(R, S), sdf.view(R, S), g3.view(R, S, 3), col.view(R, S, 3)
    mid, dists, pts, d = c["mid_z"].to(dt), c["dists"].to(dt), c["pts"].to(dt), c["rays_d"].to(dt)
    inv_s, A = _s(c["inv_s"], dt), _s(c["anneal"], dt)
    cz = (d @ c["rot"].to(dt).t())[:, 2]
    gC = c["g_color"].to(dt)
    gD = c["g_depth"].to(dt) * cz if c["g_depth"] is not None else torch.zeros(R, dtype=dt)
    tc = (d[:, None, :] * g3).sum(-1)
    r1, r2 = -tc * 0.5 + 0.5, -tc
    ic = -(torch.relu(r1) * (1.0 - A) + torch.relu(r2) * A) * vmf
    k1, k2 = (0.5 * A, 1.0 - A) if plant == "anneal_swapped" else (0.5 * (1.0 - A), A)
    dic = ((r1 > 0).to(dt) * k1 + (r2 > 0).to(dt) * k2) * vmf
    inr = torch.ones_like(vm) if plant == "clamp_ungated" else (ic > -10.0) & (ic < 10.0)
    h = ic.clamp(-10.0, 10.0) * dists * 0.5
    dh = torch.where(inr, dic * dists * 0.5, torch.zeros_like(dic))
    pc, nc = torch.sigmoid((sdf - h) * inv_s), torch.sigmoid((sdf + h) * inv_s)
    den = pc + 1e-5
    al = (pc - nc + 1e-5) / den
    alpha = al.clamp(0.0, 1.0) * vmf
    opn = ((al > 0) & (al < 1)).to(dt) * vmf
    da_dp, da_dn = nc / (den * den), -1.0 / den
    dp, dn = pc * (1.0 - pc), nc * (1.0 - nc)
    da_ds = opn * (da_dp * dp + da_dn * dn) * inv_s
    da_dtc = opn * (-da_dp * dp + da_dn * dn) * inv_s * dh
    lo, hi = (sdf + h, sdf - h) if plant == "dinvs_swapped" else (sdf - h, sdf + h)
    da_dis = opn * (da_dp * dp * lo + da_dn * dn * hi)
    u = gD[:, None] * mid + (gC[:, None, :] * col).sum(-1)
    f = 1.0 - alpha + 1e-7
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=dt), f], dim=-1), dim=-1)[:, :-1]
    w = alpha * T
    uw = u * w
    tail = torch.flip(torch.cumsum(torch.flip(uw, [1]), dim=1), [1]) - uw
    if plant == "inclusive_suffix":      # the lane's own sum is in the scanned value it starts from
        P, lane = _lanes(S)
        own = torch.zeros(R, int(lane.max()) + 1, dtype=dt).index_add_(1, lane, uw)
        tail = tail + own[:, lane]
    dal = u * T - tail / f
    d_grad = (dal * da_dtc)[..., None] * d[:, None, :]
    if c["eik_scale"] != 0.0:
        n = torch.linalg.norm(g3, dim=-1)
        relax = (torch.linalg.norm(pts, dim=-1) < 1.2).to(dt) * vmf
        fe = torch.where(n > 0, _s(c["eik_scale"], dt) * 2.0 * (n - 1.0) / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
        d_grad = d_grad + (fe * relax)[..., None] * g3
    return {"d_sdf": dal * da_ds, "d_grad": d_grad * vmf[..., None], "d_color": (w * vmf)[..., None] * gC[:, None, :],
            "d_inv_s": (dal * da_dis).sum(dim=1),
            "_kinks": torch.stack([r1.abs(), torch.where((g3 == 0).all(dim=-1), torch.ones_like(r2), r2.abs()), (ic + 10.0).abs(), (ic - 10.0).abs(), al.abs(), (al - 1.0).abs()]).amin(0),
            "_open": opn > 0}


BWD_OUT = ("d_sdf", "d_grad", "d_color", "d_inv_s")


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------

PLANS = {
    "1stage": ([2], [1.0]),
    "2stage": ([3, 2], [1.0, 0.3]),
    "s65": ([33, 17, 9, 6], [1.0, 0.4, 1.0, 0.01]),            # a band that collapses onto [near, far]: exact ties with stage 0
    "s128": ([64, 32, 16, 16], [1.0, 0.4, 0.1, 0.01]),
    "s193": ([100, 50, 29, 14], [1.0, 0.4, 0.1, 1.5]),
    "s256": ([128, 64, 32, 32], [1.0, 0.4, 0.1, 0.01]),
}
# name: (R, plan, n_depth, Dm, table sides in the order passed, jitter)
SETUP_CASES = {
    "r9-1stage-nd1-dm2": (9, "1stage", 1, 2, [9], False),
    "r3-2stage-nd2-dm7": (3, "2stage", 2, 7, [16, 4], True),
    "r4-s65-nd31-dm16": (4, "s65", 31, 16, [33, 4, 16], False),
    "r5-s128-nd33-dm16": (5, "s128", 33, 16, [64, 9, 33, 4], True),
    "r9-s193-nd64-dm7": (9, "s193", 64, 7, [64, 16], False),
    "r5-s256-nd255-dm16": (5, "s256", 255, 16, [9, 64, 16], True),
    "r3-s256-nd256-dm2": (3, "s256", 256, 2, [64, 4, 33, 9], False),
    "r1-s128-nd256-dm16": (1, "s128", 256, 16, [16], True),
    "r4-s65-nd255-dm7": (4, "s65", 255, 7, [33, 4], True),
}


def _seed(name):
    return int(np.frombuffer(name.encode(), np.uint8).astype(np.int64).sum()) * 7919 % 100003


def _unit(g, n):
    v = torch.randn(n, 3, generator=g, dtype=F64)
    return v / v.norm(dim=1, keepdim=True)


@functools.lru_cache(maxsize=None)
def setup_case(name):
    R, plan, nd, Dm, sides, jitter = SETUP_CASES[name]
    ns, rg = PLANS[plan]
    g = torch.Generator().manual_seed(_seed(name))
    # matching volume: a shell of radius 0.6 with logits in [-20, 20] plus voxel noise
    ax = (torch.arange(Dm, dtype=F64) + 0.5) * 2.0 / Dm - 1.0
    X = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    mvol = (20.0 - 40.0 * ((X.norm(dim=-1) - 0.6).abs() / 0.5).clamp(max=1.0) + 2.0 * torch.randn(Dm, Dm, Dm, generator=g, dtype=F64)).clamp(-20, 20)
    if Dm == 2:                                                          # too coarse for a shell: eight logits spread over [-20, 20]
        mvol = (torch.randperm(8, generator=g).to(F64).view(2, 2, 2) / 7.0 * 40.0 - 20.0)
    mvol = mvol.to(F32).contiguous()
    # occupancy tables: a ball per level with its own centre and radius plus scattered voxels - not nested
    tables = []
    for D in sides:
        ax = (torch.arange(D, dtype=F64) + 0.5) * 2.0 / D - 1.0
        X = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
        ctr = (torch.rand(3, generator=g, dtype=F64) - 0.5) * 0.3
        rad = 0.55 + 0.3 * float(torch.rand(1, generator=g))
        if len(sides) > 1 and D == min(sides):                           # the smallest table alone misses much of what the others hold
            rad = 0.4
        occ = ((X - ctr).norm(dim=-1) < rad) | (torch.rand(D, D, D, generator=g) < 0.08)
        t = torch.full((D, D, D), -1, dtype=torch.int32)
        t[occ] = torch.arange(int(occ.sum()), dtype=torch.int32)
        tables.append(t.contiguous())
    # rays from radius 1.8 towards a point near the centre: they leave [-1,1]^3 at both ends, |p| stays under 1.5
    o = _unit(g, R) * 1.8
    aim = _unit(g, R) * 0.35 * torch.rand(R, 1, generator=g, dtype=F64)
    d = aim - o
    d = d / d.norm(dim=1, keepdim=True)
    o, d = o.to(F32), d.to(F32)
    near = 0.3 + 0.2 * torch.rand(R, generator=g, dtype=F64)
    far = 3.0 + 0.3 * torch.rand(R, generator=g, dtype=F64)
    # every third ray ends at the shell (the estimate sits at `far`), the next one starts there: both band shifts fire
    t = torch.linspace(1.0, 3.0, 801, dtype=F64)
    for r in range(R):
        if r % 3 == 2:
            continue
        p = o[r].to(F64)[None] + d[r].to(F64)[None] * t[:, None]
        tb = float(t[int(torch.argmax(_trilinear(mvol.to(F64), _unnorm(p, Dm))))])
        if r % 3 == 0:
            far[r] = tb + 0.01
        else:
            near[r] = tb - 0.01
    jit = (torch.rand(R, len(ns), generator=g) - 0.5).to(F32).contiguous() if jitter else None
    c = {"name": name, "rays_o": o.contiguous(), "rays_d": d.contiguous(), "near": near.to(F32), "far": far.to(F32), "mvol": mvol,
         "tables": tables, "n_samples": ns, "ranges": rg, "n_depth": nd, "jitter": jit}
    c["ref64"] = ray_setup_ref(c, F64)
    c["ref32"] = ray_setup_ref(c, F32)
    return c


SETUP_FLOAT = ("z_vals", "mid_z", "dists", "pts")


def setup_E(c):
    return {k: float((c["ref32"][k].to(F64) - c["ref64"][k]).abs().max()) for k in SETUP_FLOAT}


@functools.lru_cache(maxsize=None)
def eps_mask():
    worst = 0.0
    for name in SETUP_CASES:
        c = setup_case(name)
        p32 = c["ref64"]["pts"].to(F32)
        for t in c["tables"]:
            D = t.shape[0]
            worst = max(worst, float((_unnorm(p32, D).to(F64) - _unnorm(p32.to(F64), D)).abs().max()))
    return FACTOR * worst


def check_setup(got, c, want_z=True):
    """The comparator of part B: -> list of complaints (empty = accepted).  got: float32 outputs + vmask."""
    bad = []
    ref, E = c["ref64"], setup_E(c)
    for k in SETUP_FLOAT:
        if k == "z_vals" and not want_z:
            continue
        a = got[k].to(F64).reshape(ref[k].shape)
        err = (a - ref[k]).abs()
        if not bool(torch.isfinite(a).all()) or float(err.max()) > FACTOR * E[k]:
            bad.append(f"{k}: max err {float(err.max()):.3e} > 8 x {E[k]:.3e}")
    if want_z and bool((got["z_vals"][:, 1:] < got["z_vals"][:, :-1]).any()):
        bad.append("z_vals decrease")
    flag, decided = occupancy(got["pts"].to(F64).reshape(-1, 3), c["tables"], eps_mask())
    vm = got["vmask"].reshape(-1).bool()
    if not torch.equal(vm[decided], flag[decided]):
        bad.append(f"vmask: {int((vm != flag)[decided].sum())} decided samples differ")
    return bad


def setup_ratios(got, c):
    ref, E = c["ref64"], setup_E(c)
    return {k: float((got[k].to(F64).reshape(ref[k].shape) - ref[k]).abs().max()) / (FACTOR * E[k]) for k in SETUP_FLOAT if k in got}


# ---- compositing cases

S_LIST = (2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
INV_S = (20.0, 90.0, 640.0)
ANNEAL = (0.0, 0.7, 1.0)
FWD_CASES = [(R, S) for S in S_LIST for R in (1, 4, 5)] + [(9, 129)]
BWD_CASES = [(R, S) for S in S_LIST for R in (1, 5)] + [(9, 129)]
FWD_IDS = [f"r{R}-s{S}" for R, S in FWD_CASES]
BWD_IDS = [f"r{R}-s{S}" for R, S in BWD_CASES]
KINDS = ("lane", "last", "none", "allmasked", "maskedside", "eight", "nine", "zerograd")


def _rotation(g):
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.to(F32).contiguous()


def _comp_case(i, R, S, tame, draw=0):
    """tame (part D): no saturated or negative-distance samples, every unmasked sample within the sigmoid's open range."""
    inv_s, anneal = INV_S[i % 3], ANNEAL[(i // 3 + i) % 3]
    if S == 256:
        inv_s = 20.0 if R != 5 else 90.0
    g = torch.Generator().manual_seed(1000 * i + 17 * S + R + (500000 if tame else 0) + 7000003 * draw)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    P = (S + 63) // 64
    d = _unit(g, R)
    perp = torch.cross(d, _unit(g, R), dim=1)
    o = -1.8 * d + perp / perp.norm(dim=1, keepdim=True) * (0.3 + 0.3 * rnd(R, 1))
    tau = 0.3 + 3.0 * (torch.arange(S, dtype=F64)[None] + rnd(R, S)) / S
    pts = (o[:, None] + d[:, None] * tau[..., None]).to(F32)
    pn = pts.to(F64).norm(dim=-1)
    close = ((pn - 1.0).abs() < 2e-4) | ((pn - 1.2).abs() < 2e-4)
    pts = torch.where(close[..., None], pts * 1.0005, pts)               # off the two sphere tests
    dists = (0.3 + 1.4 * rnd(R, S)) * 0.25 / inv_s
    mid = 0.5 + torch.cumsum(dists, dim=1) - dists
    grad = _unit(g, R * S).view(R, S, 3) * (0.7 + 0.6 * rnd(R, S, 1))
    color = rnd(R, S, 3)
    n_valid = torch.randint(0, 7, (R, S), generator=g).to(torch.uint8)
    n_valid[:, ::5] = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, n_valid[:, ::5].shape, generator=g)]
    # mask in runs of 1..6 samples, about two thirds occupied
    vm = torch.zeros(R, S, dtype=torch.bool)
    for r in range(R):
        k = 0
        while k < S:
            n = 1 + int(torch.randint(0, 6, (1,), generator=g))
            vm[r, k:k + n] = bool(rnd(1) < 0.68)
            k += n
    x = 2.5 + 5.5 * rnd(R, S)                                             # sdf * inv_s before the crossing
    kinds = []
    for r in range(R):
        kind = KINDS[(i + r) % 8] if R >= 4 else [k for k in KINDS if k != "allmasked"][(i // (3 if not tame else 2)) % 7]
        if tame and kind == "allmasked":
            kind = "lane"
        if not tame and (R, S) == (1, 256):
            kind = "last"
        kinds.append(kind)
        if S <= 3:
            vm[r] = torch.tensor(([True, False, True] if (i + r) % 2 == 0 else [True, True, True])[:S]) if R > 1 else torch.tensor([True, False, True][:S])
            x[r] = 0.1 + 0.4 * rnd(S)            # d alpha / d inv_s changes sign near sdf * inv_s = 1.3: stay clear of it
            dists[r] *= 6.0
            mid[r] = 0.5 + torch.cumsum(dists[r], dim=0) - dists[r]
            x[r, S - 1] = -x[r, S - 1]
            continue
        lane_k = [k for k in range(S // 3, S - 1) if k % P == P - 1]
        kc = {"last": S - 2, "none": S}.get(kind, lane_k[int(torch.randint(0, len(lane_k), (1,), generator=g))] if lane_k else S - 2)
        if kind == "allmasked":
            vm[r] = False
            continue
        if kc < S:
            vm[r, kc] = vm[r, kc + 1] = True
            ramp = torch.arange(S, dtype=F64)
            x[r] = torch.where(ramp <= kc, torch.minimum(x[r], 0.3 + 0.9 * (kc - ramp)), -(0.2 + 7.8 * rnd(S)))
        if kind == "maskedside" and kc >= 6:                             # a sign change whose far side is masked out: no crossing there
            x[r, 3] = -x[r, 3]
            vm[r, 2], vm[r, 3], vm[r, 4] = True, True, False
            vm[r, 5] = False
            x[r, 2] = abs(x[r, 2])
            # ... and its near side: 2|3 is a crossing unless 3 is masked
            vm[r, 3] = False
        if kind in ("eight", "nine") and int(vm[r].sum()) >= 9:
            want = 8 if kind == "eight" else 9
            idx = torch.nonzero(vm[r])[:, 0]
            n_valid[r, idx] = torch.tensor([0, 1], dtype=torch.uint8)[torch.arange(len(idx)) % 2]
            n_valid[r, idx[:want]] = torch.tensor([2, 255, 3], dtype=torch.uint8)[torch.arange(want) % 3]
        if kind == "zerograd":
            grad[r, 1::7] = 0.0
        if kind in ("nine", "lane"):                                      # the +-10 clamp is active: |grad| >= 12, d . grad < -10
            grad[r, 2::9] = -d[r] * (22.0 + 8.0 * rnd(len(range(2, S, 9)), 1))
    sdf = x / inv_s
    for r in range(R):
        if S > 3 and kinds[r] == "eight" and vm[r].any():                # exact zeros of both signs
            idx = torch.nonzero(vm[r])[:, 0]
            sdf[r, idx[0]] = 0.0
            if len(idx) > 4:
                sdf[r, idx[len(idx) // 2]] = -0.0
        if not tame and (R, S) == (1, 256):
            # a saturated first sample (alpha = 1): everything behind it is scaled by the 1e-7 that keeps the transmittance from
            # vanishing - or is exactly zero without it.  Along an ordinary ray the term cannot be seen: 1 - a + 1e-7f rounds to
            # 1 - a + 2 ulp in fp32, so the oracle's own arithmetic is off by 0.19e-7 per factor and 8 E exceeds 256 x 1e-7.
            sdf[r, 0] = -60.0 / inv_s
            vm[r, 0] = True
        if not tame and S > 16 and kinds[r] in ("lane", "zerograd"):     # saturated samples (alpha clipped at 1) behind the crossing ...
            sdf[r, S - 3:] = -60.0 / inv_s
            vm[r, S - 3:] = True
        if not tame and S > 16 and kinds[r] == "none":                   # ... and negative section lengths (alpha clipped at 0)
            dists[r, 4::11] = -dists[r, 4::11]
    # occupancy share within (0.2, 0.9) for every case
    share = float(vm.double().mean())
    assert 0.2 <= share <= 0.9, (R, S, share)
    c = {"sdf": sdf.to(F32), "grad": grad.to(F32), "color": color.to(F32), "n_valid": n_valid, "mid_z": mid.to(F32),
         "dists": dists.to(F32), "pts": pts, "vmask": vm, "rays_d": d.to(F32), "rot": _rotation(g), "inv_s": inv_s, "anneal": anneal,
         "kinds": kinds, "R": R, "S": S, "P": P}
    c["g_color"] = (torch.randn(R, 3, generator=g) * (8.0 if S <= 3 else 1.0) * inv_s / 20.0).contiguous()   # d_inv_s goes with 1 / inv_s
    c["g_depth"] = torch.randn(R, generator=g).contiguous() if (i % 2 == 0 or not tame) else None
    c["eik_scale"] = 2.0 ** -6 if (i % 3 != 1 and tame) else 0.0
    return c


@functools.lru_cache(maxsize=None)
def fwd_case(i):
    c = _comp_case(i, *FWD_CASES[i], tame=False)
    c["ref64"], c["ref32"] = composite_ref(c, F64), composite_ref(c, F32)
    return c


def _has_cross(c):
    return c["ref64"]["_k"] >= 0


def fwd_E(c):
    E = {k: float((c["ref32"][k].to(F64) - c["ref64"][k]).abs().max()) for k in FWD_FLOAT}
    m = _has_cross(c)
    z64 = c["ref64"]["z_sdf0"][m]
    E["z_sdf0"] = float(((c["ref32"]["z_sdf0"][m].to(F64) - z64).abs() / z64.abs()).max()) if bool(m.any()) else 0.0
    return E


def check_forward(got, c):
    bad = []
    ref, E = c["ref64"], fwd_E(c)
    for k in FWD_FLOAT:
        a = got[k].to(F64).reshape(ref[k].shape)
        err = (a - ref[k]).abs()
        if not bool(torch.isfinite(a).all()) or float(err.max()) > FACTOR * E[k]:
            bad.append(f"{k}: max err {float(err.max()):.3e} > 8 x {E[k]:.3e}")
    for k in FWD_EXACT:
        if not torch.equal(got[k].reshape(ref[k].shape).to(F64), ref[k].to(F64)):
            bad.append(f"{k}: differs")
    m = _has_cross(c)
    z = got["z_sdf0"].to(F64)
    if bool(m.any()):
        rel = ((z - ref["z_sdf0"]).abs() / ref["z_sdf0"].abs())[m]
        if not bool(torch.isfinite(z[m]).all()) or float(rel.max()) > FACTOR * E["z_sdf0"]:
            bad.append(f"z_sdf0: max rel err {float(rel.max()):.3e} > 8 x {E['z_sdf0']:.3e}")
        # the bracket [mid_z[k], mid_z[k+1]] the kernel's z_sdf0 lies in is the reference's k
        mid = c["mid_z"].to(F64)
        k = ref["_k"].clamp(min=0)
        lo, hi = mid.gather(1, k[:, None])[:, 0], mid.gather(1, (k + 1)[:, None])[:, 0]
        slack = FACTOR * E["z_sdf0"] * z.abs()
        if bool((((z < lo - slack) | (z > hi + slack)) & m).any()):
            bad.append("z_sdf0: outside the reference's bracket")
    if bool((got["sdf_depth"].reshape(-1)[~m] != 0).any()) or bool((got["mid_inside_sphere"].reshape(-1)[~m] != 0).any()):
        bad.append("a ray without a crossing has a surface depth")
    return bad


def fwd_ratios(got, c):
    ref, E = c["ref64"], fwd_E(c)
    return {k: float((got[k].to(F64).reshape(ref[k].shape) - ref[k]).abs().max()) / (FACTOR * E[k]) for k in FWD_FLOAT if E[k] > 0}


def _as_got(ref):
    """A reference's outputs as a kernel would hand them over (float32)."""
    return {k: (v.to(F32) if torch.is_tensor(v) and v.dtype == F64 else v) for k, v in ref.items() if not k.startswith("_")}


@functools.lru_cache(maxsize=None)
def bwd_case(i):
    """With R = 1, d_inv_s is one number and its E a single draw of the fp32 error.  A draw under half an ulp of the value itself
    (2^-24 |value|, which no fp32 evaluation of a sum can be held to) says nothing about fp32: such inputs are drawn again.  The
    rule looks at the two CPU evaluations only."""
    for draw in range(16):
        c = _comp_case(i, *BWD_CASES[i], tame=True, draw=draw)
        c["ref64"], c["ref32"] = composite_bwd_autograd(c, F64), composite_bwd_autograd(c, F32)
        c["closed64"] = composite_bwd_ref(c, F64)
        c["keep"] = (c["closed64"]["_kinks"] >= KINK) | ~c["vmask"]
        big = all(float(c["ref64"][k].abs().max()) >= 1e-3 for k in ("d_sdf", "d_grad", "d_inv_s"))
        if big and all(v >= 2.0 ** -24 * float(c["ref64"][k].abs().max()) for k, v in bwd_E(c).items()):
            return c
    raise AssertionError(f"no representative draw for {BWD_IDS[i]}")


def _bwd_sel(c, k, t):
    t = t.to(F64)
    return t[c["keep"]] if k in ("d_sdf", "d_grad") else t.reshape(-1)


def bwd_E(c):
    return {k: float((_bwd_sel(c, k, c["ref32"][k]) - _bwd_sel(c, k, c["ref64"][k])).abs().max()) for k in BWD_OUT}


def check_backward(got, c):
    bad = []
    E = bwd_E(c)
    for k in BWD_OUT:
        a = _bwd_sel(c, k, got[k].reshape(c["ref64"][k].shape))
        err = (a - _bwd_sel(c, k, c["ref64"][k])).abs()
        if not bool(torch.isfinite(got[k]).all()) or float(err.max()) > FACTOR * E[k]:
            bad.append(f"{k}: max err {float(err.max()):.3e} > 8 x {E[k]:.3e}")
    m = ~c["vmask"]
    if any(bool((got[k].reshape(c["ref64"][k].shape)[m] != 0).any()) for k in ("d_sdf", "d_grad", "d_color")):
        bad.append("a masked row has a gradient")
    return bad


def bwd_ratios(got, c):
    E = bwd_E(c)
    return {k: float((_bwd_sel(c, k, got[k].reshape(c["ref64"][k].shape)) - _bwd_sel(c, k, c["ref64"][k])).abs().max()) / (FACTOR * E[k])
            for k in BWD_OUT if E[k] > 0}


# ------------------------------------------------------------------------------------------------------------------
# A. anchor, input conditions, sensitivity, recorded margins (no GPU)
# ------------------------------------------------------------------------------------------------------------------


def _close(a, b, what):
    a, b = a.to(F64), b.to(F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
    assert err <= 1e-6, (what, err)


def test_restatement_matches_the_oracle_on_the_golden_scene(scene, weights, golden_fpn, golden_pipe):
    """dt = float32 is O.ray_zsample and O.render_core's tail: integer / boolean outputs equal, floats to 1e-6 relative (of
    max(|value|, 1): the sums cancel).  The closed-form backward is pinned to float64 autograd."""
    vols, tabs, masks, mvol = pipeline_views(golden_pipe)
    feats = [golden_fpn[f"out{i}"] for i in range(4)][::-1]
    R = scene["rays_o"].shape[0]
    near, far = scene["near"].repeat(R, 1), scene["far"].repeat(R, 1)
    g = torch.Generator().manual_seed(5)
    for jit in (None, torch.rand(R, 4, generator=g) - 0.5):
        c = {"rays_o": scene["rays_o"], "rays_d": scene["rays_d"], "near": near[:, 0], "far": far[:, 0], "mvol": mvol,
             "tables": [t.to(torch.int32) for t in tabs], "n_samples": CFG["n_samples"], "ranges": CFG["sample_ranges"],
             "n_depth": CFG["n_depth"], "jitter": jit}
        st = ray_setup_ref(c, F32)
        z = O.ray_zsample(scene["rays_o"], scene["rays_d"], near, far, mvol, CFG["n_samples"], CFG["sample_ranges"], CFG["n_depth"], jit)
        _close(st["z_vals"], z, "z_vals")
    S = z.shape[1]
    anneal = 0.3
    z = st["z_vals"]
    out = O.render_core(weights, scene["rays_o"], scene["rays_d"], z, 2.0 / CFG["n_samples"][0], vols, tabs, masks, feats, scene["imgs"],
                        scene["intrs"], scene["c2ws"], anneal)
    _close(st["mid_z"], out["mid_z_vals"], "mid_z")
    assert torch.equal(st["vmask"].view(R, S), out["voxel_mask"] > 0)
    vm = st["vmask"]
    _, _, mvalid = O.lookup_feature(st["pts"][vm], scene["imgs"], scene["intrs"], scene["c2ws"], feats)
    n_valid = torch.zeros(R * S, dtype=torch.uint8)
    n_valid[vm] = mvalid.sum(dim=1).to(torch.uint8)
    inv_s = float(torch.exp(weights["implicit_surface.deviation_network.variance"] * 10.0).clamp(1e-6, 1e6))
    cc = {"sdf": out["sdf"], "grad": out["gradients"], "color": out["sampled_color"], "n_valid": n_valid.view(R, S), "mid_z": st["mid_z"],
          "dists": st["dists"], "pts": st["pts"].view(R, S, 3), "vmask": vm.view(R, S), "rays_d": scene["rays_d"],
          "rot": torch.inverse(scene["c2ws"][0, :3, :3]), "inv_s": inv_s, "anneal": anneal}
    f = composite_ref(cc, F32)
    for k, ko in (("color_fine", "color_fine"), ("render_depth", "render_depth"), ("sdf_depth", "sdf_depth"), ("normal", "normal"),
                  ("weights", "weights"), ("inside_sphere", "inside_sphere")):
        _close(f[k], out[ko], k)
    assert torch.equal(f["valid_mask"], out["valid_mask"])
    assert torch.equal(f["mid_inside_sphere"].float(), out["mid_inside_sphere"])
    gerr = f["eik"][:, 0].sum() / (f["eik"][:, 1].sum() + 1e-5)
    _close(gerr, out["gradient_error"], "gradient_error")
    assert int((f["_k"] >= 0).sum()) >= 5 and bool(f["mid_inside_sphere"].any())
    # closed form against autograd, float64, on a ragged case of each P
    for i in (BWD_IDS.index("r5-s63"), BWD_IDS.index("r5-s127"), BWD_IDS.index("r9-s129"), BWD_IDS.index("r5-s193")):
        c = bwd_case(i)
        for k in BWD_OUT:
            a, b = _bwd_sel(c, k, c["closed64"][k]), _bwd_sel(c, k, c["ref64"][k])
            assert float((a - b).abs().max()) <= 1e-9 * max(float(b.abs().max()), 1.0), (BWD_IDS[i], k)


def _setup_stats():
    und = 0.0
    for name in SETUP_CASES:
        c = setup_case(name)
        _, decided = occupancy(c["ref64"]["pts"].to(F32).to(F64), c["tables"], eps_mask())
        und = max(und, float((~decided).double().mean()))
    return und


def test_setup_inputs_meet_their_conditions():
    hi = lo = ties = outside = 0
    for name, (R, plan, nd, Dm, sides, jitter) in SETUP_CASES.items():
        c = setup_case(name)
        ref = c["ref64"]
        assert 0.2 <= float(ref["vmask"].double().mean()) <= 0.9, (name, float(ref["vmask"].double().mean()))
        _, decided = occupancy(ref["pts"].to(F32).to(F64), c["tables"], eps_mask())
        assert float((~decided).double().mean()) <= 0.01, name
        assert float(c["mvol"].abs().max()) > 15 and float(ref["pts"].norm(dim=1).max()) <= 2.0
        assert len(set(c["near"].tolist())) == R and len(set(c["far"].tolist())) == R
        hi += sum(int((h > 1e-3).sum()) for h in ref["hi_fired"])
        lo += sum(int((l > 1e-3).sum()) for l in ref["lo_fired"])
        ties += int((ref["dists"][:, :-1] == 0).sum())
        outside += int((ref["pts"].abs().max(dim=1).values > 1.0).sum())
        assert sides != sorted(sides) or len(sides) == 1
        assert all(v > 0 for v in setup_E(c).values()), name
    assert hi > 0 and lo > 0 and ties > 0 and outside > 0
    assert {c[0] for c in SETUP_CASES.values()} == {1, 3, 4, 5, 9}
    assert {c[1] for c in SETUP_CASES.values()} == set(PLANS)
    assert {c[2] for c in SETUP_CASES.values()} == {1, 2, 31, 33, 64, 255, 256}
    assert {c[3] for c in SETUP_CASES.values()} == {2, 7, 16}
    assert {len(c[4]) for c in SETUP_CASES.values()} == {1, 2, 3, 4} and {s for c in SETUP_CASES.values() for s in c[4]} == {4, 9, 16, 33, 64}
    assert {c[5] for c in SETUP_CASES.values()} == {True, False}
    assert any(r >= 1 for _, rg in PLANS.values() for r in rg[1:])


def test_forward_inputs_meet_their_conditions():
    seen = set()
    for i, (R, S) in enumerate(FWD_CASES):
        c = fwd_case(i)
        ref, vm, P = c["ref64"], c["vmask"], c["P"]
        assert 0.2 <= float(vm.double().mean()) <= 0.9, FWD_IDS[i]
        pn = ref["_pn"]
        assert float((pn - 1.0).abs().min()) >= 1e-4 and float((pn - 1.2).abs().min()) >= 1e-4, FWD_IDS[i]
        k = ref["_k"]
        assert float((ref["_cosd"] - 0.5).abs()[k >= 0].min() if bool((k >= 0).any()) else 1.0) >= 1e-4, FWD_IDS[i]
        s = c["sdf"].to(F64)[vm]
        assert bool(((s.abs() >= 1e-12) | (s == 0)).all())
        for r in range(R):
            kr = int(k[r])
            seen.add("none" if kr < 0 else "cross")
            if kr >= 0 and kr % P == P - 1:
                seen.add(f"lane{P}")
            if kr == S - 2:
                seen.add("last")
            sr, mr = c["sdf"][r], vm[r]
            if bool(((sr == 0) & ~torch.signbit(sr) & mr).any()):
                seen.add("+0")
            if bool(((sr == 0) & torch.signbit(sr) & mr).any()):
                seen.add("-0")
            if not bool(mr.any()):
                seen.add("allmasked")
            raw = c["sdf"][r].to(F64)
            if bool((((raw[:-1] * raw[1:]) <= 0) & (mr[:-1] ^ mr[1:])).any()):
                seen.add("maskedside")
            n = int(((c["n_valid"][r] > 1) & mr).sum())
            seen.add(f"valid{n}" if n in (8, 9) else "")
            for v in (0, 1, 2, 255):
                if bool(((c["n_valid"][r] == v) & mr).any()):
                    seen.add(f"nv{v}")
            g = c["grad"][r].to(F64)
            if bool(((g.norm(dim=1) >= 12) & (ref["_tc"][r] < -10) & (ref["_ic"][r] < -10) & mr).any()):
                seen.add("clamp")
            if bool(((g == 0).all(dim=1) & mr).any()):
                seen.add("zerograd")
            al = ref["_al"][r][mr]
            seen.update({"clip0"} if bool((al <= 0).any()) else set())
            seen.update({"clip1"} if bool((c["ref32"]["_al"][r][mr] >= 1).any()) else set())
        al = ref["_al"][vm]
        assert float(((al > 0) & (al < 1)).double().mean()) > 0.5
        assert bool(ref["inside_sphere"].any()) or S <= 3
        assert all(v > 0 for k, v in fwd_E(c).items() if k not in ("sdf_depth", "z_sdf0")), (FWD_IDS[i], fwd_E(c))
    want = {"none", "cross", "lane1", "lane2", "lane3", "lane4", "last", "+0", "-0", "allmasked", "maskedside", "valid8", "valid9",
            "nv0", "nv1", "nv2", "nv255", "clamp", "zerograd", "clip0", "clip1"}
    assert want <= seen, want - seen
    assert {c["inv_s"] for c in map(fwd_case, range(len(FWD_CASES)))} == set(INV_S)
    assert {c["anneal"] for c in map(fwd_case, range(len(FWD_CASES)))} == set(ANNEAL)
    assert any(bool(fwd_case(i)["ref64"]["mid_inside_sphere"].any()) for i in range(len(FWD_CASES)))
    assert any(bool(((fwd_case(i)["ref64"]["_k"] >= 0) & ~fwd_case(i)["ref64"]["mid_inside_sphere"][:, 0]).any()) for i in range(len(FWD_CASES)))


def _left_out():
    worst = 0.0
    for i in range(len(BWD_CASES)):
        c = bwd_case(i)
        worst = max(worst, float((~c["keep"])[c["vmask"]].double().mean()))
    return worst


def test_backward_inputs_meet_their_conditions():
    combos = set()
    for i, (R, S) in enumerate(BWD_CASES):
        c = bwd_case(i)
        vm = c["vmask"]
        assert 0.2 <= float(vm.double().mean()) <= 0.9, BWD_IDS[i]
        for k in ("d_sdf", "d_grad", "d_inv_s"):
            assert float(c["ref64"][k].abs().max()) >= 1e-3, (BWD_IDS[i], k)
        assert float(c["closed64"]["_open"][vm].double().mean()) >= 0.5, BWD_IDS[i]
        assert float((~c["keep"])[vm].double().mean()) <= 0.01, BWD_IDS[i]
        assert all(bool(torch.isfinite(c["ref64"][k]).all()) for k in BWD_OUT)
        assert all(v >= 2.0 ** -24 * float(c["ref64"][k].abs().max()) for k, v in bwd_E(c).items()), BWD_IDS[i]
        combos.add((c["g_depth"] is not None, c["eik_scale"] != 0.0))
    assert len(combos) == 4
    assert {bwd_case(i)["inv_s"] for i in range(len(BWD_CASES))} == set(INV_S)
    assert {bwd_case(i)["anneal"] for i in range(len(BWD_CASES))} == set(ANNEAL)
    # the clamp's gate and the zero-gradient guard are exercised where the eikonal term is on
    assert any("nine" in bwd_case(i)["kinds"] or "lane" in bwd_case(i)["kinds"] for i in range(len(BWD_CASES)))
    assert any("zerograd" in bwd_case(i)["kinds"] and bwd_case(i)["eik_scale"] != 0 for i in range(len(BWD_CASES)))


SETUP_PLANTS = {
    "no_hi_shift": lambda c: any(bool((h > 1e-3).any()) for h in c["ref64"]["hi_fired"]),
    "no_lo_shift": lambda c: any(bool((l > 1e-3).any()) for l in c["ref64"]["lo_fired"]),
    "jitter_scale": lambda c: c["jitter"] is not None and len(c["n_samples"]) > 1,
    "drop_partial_trip": lambda c: c["n_depth"] % 32 != 0 and len(c["n_samples"]) > 1,
    "last_dist_prev": lambda c: True,
    "or_smallest_only": lambda c: len(c["tables"]) > 1,
}


@pytest.mark.parametrize("plant", sorted(SETUP_PLANTS))
def test_setup_comparator_rejects(plant):
    """Each planted mistake, applied to the float64 restatement, is rejected in every case whose shape can show it."""
    hit = 0
    for name in SETUP_CASES:
        c = setup_case(name)
        assert check_setup(_as_got(c["ref64"]), c) == [], name             # the float64 reference itself passes ...
        assert check_setup(_as_got(c["ref32"]), c) == [], name             # ... and so does the oracle's arithmetic
        if SETUP_PLANTS[plant](c):
            hit += 1
            assert check_setup(_as_got(ray_setup_ref(c, F64, plant)), c) != [], (plant, name)
    assert hit >= 2, plant


FWD_PLANTS = ("neighbour_same_lane", "inclusive_T", "no_1e-7", "no_1e-5", "inside_for_relax", "last_crossing")
BWD_PLANTS = ("inclusive_suffix", "clamp_ungated", "anneal_swapped", "dinvs_swapped")


@pytest.mark.parametrize("plant", FWD_PLANTS)
def test_forward_comparator_rejects(plant):
    """Rejected at every P = ceil(S / 64) in 1..4 (some case of that P), `+1e-7 dropped` at S = 256 in particular."""
    caught = set()
    for i, (R, S) in enumerate(FWD_CASES):
        c = fwd_case(i)
        if plant == FWD_PLANTS[0]:
            assert check_forward(_as_got(c["ref64"]), c) == [] and check_forward(_as_got(c["ref32"]), c) == [], FWD_IDS[i]
        if S > 3 and check_forward(_as_got(composite_ref(c, F64, plant)), c) != []:
            caught.add(c["P"])
            caught.add(f"S{S}")
    assert {1, 2, 3, 4} <= caught, (plant, caught)
    assert "S256" in caught, plant


@pytest.mark.parametrize("plant", BWD_PLANTS)
def test_backward_comparator_rejects(plant):
    caught = set()
    for i, (R, S) in enumerate(BWD_CASES):
        c = bwd_case(i)
        if plant == BWD_PLANTS[0]:
            assert check_backward(_as_got(c["closed64"]), c) == [] and check_backward(_as_got(c["ref32"]), c) == [], BWD_IDS[i]
        if S > 3 and check_backward(_as_got(composite_bwd_ref(c, F64, plant)), c) != []:
            caught.add(c["P"])
    assert {1, 2, 3, 4} <= caught, (plant, caught)


def _recorded(label):
    m = re.search(label + r"\s*=\s*([0-9.e+-]+)", __doc__)
    return float(m.group(1))


def measured():
    return {
        "E_SETUP": max(max(setup_E(setup_case(n)).values()) for n in SETUP_CASES),
        "EPS_MASK": eps_mask(),
        "UNDECIDED": _setup_stats(),
        "E_FORWARD": max(max(fwd_E(fwd_case(i)).values()) for i in range(len(FWD_CASES))),
        "E_BACKWARD": max(max(bwd_E(bwd_case(i)).values()) for i in range(len(BWD_CASES))),
        "LEFT_OUT": _left_out(),
    }


def test_measured_margins_are_recorded():
    """The numbers of the module docstring are the ones these inputs give (10 % of slack for another host's libm / summation
    order; the two shares are counts and are held to their caps as well)."""
    m = measured()
    for label, v in m.items():
        rec = _recorded(label)
        assert abs(v - rec) <= 0.1 * rec + 1e-30, (label, v, rec)
    assert m["UNDECIDED"] <= 0.01 and m["LEFT_OUT"] <= 0.01


# ------------------------------------------------------------------------------------------------------------------
# B. surf_ray_setup
# ------------------------------------------------------------------------------------------------------------------


def _report(kind, name, ratios):
    print(f"[margin] {kind} {name} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))


def _run_setup(c, want_z):
    from surf_amd import ops
    d = dev()
    sv = ops.SparseVolumes([torch.zeros(1, 8).to(d) for _ in c["tables"]], [t.to(d) for t in c["tables"]])
    out = ops.ray_setup(c["rays_o"].to(d), c["rays_d"].to(d), c["near"].to(d), c["far"].to(d), c["mvol"].to(d), sv, c["n_samples"],
                        c["ranges"], c["n_depth"], want_z=want_z, jitter=None if c["jitter"] is None else c["jitter"].to(d))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("name", list(SETUP_CASES))
def test_ray_setup_matches_float64(name):
    c = setup_case(name)
    got = _run_setup(c, True)
    _report("setup", name, setup_ratios(got, c))
    assert check_setup(got, c) == []
    lean = _run_setup(c, False)
    assert "z_vals" not in lean
    for k in ("mid_z", "dists", "pts", "vmask"):
        assert torch.equal(lean[k], got[k]), k
    assert set(got["vmask"].unique().tolist()) <= {0, 1}


@gpu
def test_ray_setup_refuses_what_it_cannot_hold():
    from surf_amd import _lib
    c = dict(setup_case("r3-2stage-nd2-dm7"))
    for over in ({"n_samples": [129, 64, 32, 32], "ranges": [1.0, 0.4, 0.1, 0.01]}, {"n_depth": 257}):
        with pytest.raises(_lib.SurfHipError):
            _run_setup({**c, **over, "jitter": None}, True)


# ------------------------------------------------------------------------------------------------------------------
# C. surf_composite
# ------------------------------------------------------------------------------------------------------------------


def _comp_gpu(c, poison=False):
    d = dev()
    vm = c["vmask"]
    sdf, grad, col, nv = c["sdf"].clone(), c["grad"].clone(), c["color"].clone(), c["n_valid"].clone()
    if poison:
        sdf[~vm], grad[~vm], col[~vm], nv[~vm] = float("nan"), float("nan"), float("nan"), 255
    R, S = vm.shape
    setup = {"mid_z": c["mid_z"].to(d).contiguous(), "dists": c["dists"].to(d).contiguous(), "pts": c["pts"].reshape(-1, 3).to(d).contiguous(),
             "vmask": vm.reshape(-1).to(torch.uint8).to(d)}
    cams = types.SimpleNamespace(rot_ref=np.ascontiguousarray(c["rot"].numpy()))
    return (sdf.reshape(-1).to(d).contiguous(), grad.reshape(-1, 3).to(d).contiguous(), col.reshape(-1, 3).to(d).contiguous(),
            nv.reshape(-1).to(d).contiguous(), setup, c["rays_d"].to(d).contiguous(), cams)


def _run_forward(c, poison=False, **kw):
    from surf_amd import ops
    sdf, grad, col, nv, setup, rays_d, cams = _comp_gpu(c, poison)
    out = ops.composite(sdf, grad, col, nv, setup, rays_d, c["inv_s"], c["anneal"], cams, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("i", range(len(FWD_CASES)), ids=FWD_IDS)
def test_composite_matches_float64(i):
    c = fwd_case(i)
    got = _run_forward(c, want_z0=True)
    _report("forward", FWD_IDS[i], fwd_ratios(got, c))
    assert check_forward(got, c) == []
    # the optional outputs change nothing else
    lean = _run_forward(c, per_sample=False, want_z0=False)
    assert "weights" not in lean and "inside_sphere" not in lean and "z_sdf0" not in lean
    for k, v in lean.items():
        assert torch.equal(v, got[k]), k
    # masked-out rows are never read: NaN / 255 there changes no bit
    dirty = _run_forward(c, poison=True, want_z0=True)
    for k, v in dirty.items():
        assert bool(torch.isfinite(v.float()).all()), k
        assert torch.equal(v, got[k]) and torch.equal(torch.signbit(v.float()), torch.signbit(got[k].float())), k


@gpu
def test_composite_refuses_what_it_cannot_hold():
    from surf_amd import _lib
    base = fwd_case(FWD_IDS.index("r4-s64"))
    for S in (1, 257):
        c = {k: (v[:, :1].repeat(1, S, *([1] * (v.dim() - 2))) if torch.is_tensor(v) and v.dim() >= 2 and v.shape[:2] == (4, 64) else v)
             for k, v in base.items()}
        with pytest.raises(_lib.SurfHipError):
            _run_forward(c)


# ------------------------------------------------------------------------------------------------------------------
# D. surf_composite_backward[_s]
# ------------------------------------------------------------------------------------------------------------------


def _run_backward(c, poison=False, eik=None, per_ray=True):
    """-> d_sdf, d_grad, d_color and d_inv_s (R): ops.composite_backward adds the per-ray partial sums, so each ray's own value
    comes from a launch whose upstream gradients are zero on every other ray (their partial sums are then exact zeros)."""
    from surf_amd import ops
    d = dev()
    sdf, grad, col, _, setup, rays_d, cams = _comp_gpu(c, poison)
    R = c["R"]
    gC = c["g_color"].to(d)
    gD = None if c["g_depth"] is None else c["g_depth"].to(d)
    scale, up = (c["eik_scale"], None) if eik is None else eik
    d_sdf, d_grad, d_col, total = ops.composite_backward(sdf, grad, col, setup, rays_d, c["inv_s"], c["anneal"], cams, gC, gD,
                                                         eik_scale=scale, eik_upstream=up)
    out = {"d_sdf": d_sdf.cpu(), "d_grad": d_grad.cpu(), "d_color": d_col.cpu(), "_total": total.cpu()}
    if per_ray:
        rows = []
        for r in range(R):
            one = torch.zeros(R, 1, device=d)
            one[r] = 1.0
            rows.append(ops.composite_backward(sdf, grad, col, setup, rays_d, c["inv_s"], c["anneal"], cams, (gC * one).contiguous(),
                                               None if gD is None else gD * one[:, 0])[3].cpu())
        out["d_inv_s"] = torch.stack(rows)
    torch.cuda.synchronize()
    return out


@gpu
@pytest.mark.parametrize("i", range(len(BWD_CASES)), ids=BWD_IDS)
def test_composite_backward_matches_float64_autograd(i):
    c = bwd_case(i)
    got = _run_backward(c)
    _report("backward", BWD_IDS[i], bwd_ratios(got, c))
    assert check_backward(got, c) == []
    E = bwd_E(c)["d_inv_s"]
    assert abs(float(got["_total"]) - float(c["ref64"]["d_inv_s"].sum())) <= FACTOR * E * c["R"]
    dirty = _run_backward(c, poison=True, per_ray=False)
    for k in ("d_sdf", "d_grad", "d_color", "_total"):
        assert bool(torch.isfinite(dirty[k]).all()) and torch.equal(dirty[k], got[k]), k
    # the device-scalar variant: eik_scale e times a device upstream u against the plain float e u (dyadic, so exact)
    e, u = 2.0 ** -4, 2.0 ** -3 * 3.0
    a = _run_backward(c, eik=(e, torch.tensor([u], device=dev())), per_ray=False)
    b = _run_backward(c, eik=(float(np.float32(e * u)), None), per_ray=False)
    for k in ("d_sdf", "d_grad", "d_color", "_total"):
        assert torch.equal(a[k], b[k]), k
    if bool(((c["pts"].to(F64).norm(dim=-1) < 1.2) & c["vmask"]).any()):           # ... and the term is there at all
        assert not torch.equal(a["d_grad"], _run_backward(c, eik=(0.0, None), per_ray=False)["d_grad"])


# ------------------------------------------------------------------------------------------------------------------
# E. surf_pack_texel4
# ------------------------------------------------------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("C", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (3, 17, 19)])
def test_pack_texel4_copies_and_pads(C, shape):
    from surf_amd import ops
    n, H, W = shape
    x = torch.randn(n, C, H, W, generator=torch.Generator().manual_seed(C * 100 + H))
    t4 = ops.pack_texel4(x.to(dev()).contiguous()).cpu()
    assert t4.shape == (n, H, W, 4)
    assert torch.equal(t4[..., :C], x.permute(0, 2, 3, 1))
    assert bool((t4[..., C:] == 0).all()) and not bool(torch.signbit(t4[..., C:]).any())
