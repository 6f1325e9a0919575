"""The SDF inference kernels per element against a float64 restatement: surf_sdf_mlp (fp32 MFMA), surf_sdf_mlp_bf16x3 and
surf_sdf_mlp_f16x2 (gradient and forward-only instantiations, mask / idx / device-count addressing), the lattice and brick
modes of the split kernels, and the forward second-order kernel surf_sdf_smooth.  Every kernel is held to float64
independently, never to another kernel; the one exception is the bit equality of brick and lattice values, which the header
promises.

What is compared.  restate_forward writes the network once in plain torch as forward streams (value, the three axis tangents,
the tangent along u = (1,1,1) and the three mixed terms u^T H e_a) on the stream helpers of tests/test_sdf_train_kernels.py.
dt = float64 is the reference, dt = float32 the oracle's arithmetic, operands="f16pair" a second float32 restatement in which
both operands of the six hidden matrix products pass through the fp16 pair split as the f16x2 code does it (weights and biases
x 2^8 and lin3's 1/sqrt(2) folded into the matrix before the split, activations unscaled, second piece = fp16 of the fp32
residual, second x second dropped; lin6 stays fp32 as in the kernel).  Part A anchors it on the CPU: at float32 it reproduces
O.lookup_sparse_volume + O.sdf_mlp + O.sdf_mlp_smooth on the golden scene's points, at float64 it equals
autograd.grad(create_graph=True) through network_f64 for sdf, grad and smooth, the planted edge points included.

The bound.  For every output column (sdf, grad x/y/z, smooth x/y/z) of a case, E = max |restate(float32) - restate(float64)|
over the case's points together with a fixed 301-point pool on the same weights and volumes; a kernel must lie within 8 E of
float64 element by element (f16x2: 8 max(E, E16), E16 from the "f16pair" restatement), no point, element or case left out.

Buffers are the test's: outputs NaN-filled with 4 rows behind the last, the scratch exactly ..._scratch_bytes(n) at the head
of a larger byte buffer whose patterned tail must come back unchanged.  Part B: point mode (plain, mask, idx lists, _dn, bit
equality of repeated launches and of 0xFF-filled scratch).  Part C: lattice (unequal axes, slabs, both signs) and bricks
(res 8, 13, 17, unordered lists, upper faces).  Part D: surf_sdf_smooth.  Part E: refusals.  The sensitivity tests plant
thirteen mistakes into the float32 restatement or its output layout; the same comparator must reject each.

Statements of the issue that could not hold as worded, and what stands in their place:
  - a lattice axis of length 1 or 2 cannot hold -1, +1 and a value outside the box: axes of 3 or more values hold all three,
    shorter ones hold off-plane values (and +1 at length 2).
  - a brick list has 512 points per brick = four whole rounds of 128: no brick list has a ragged last round.  In its place: a
    three-brick unordered list (12 rounds, no power of two) beside one brick and all bricks; every upper brick of res 13 and 17
    is partial, so the last rounds of those lists are the ones with masked points.
  - "pre-activations inside fp16 range in the units the f16x2 kernel holds them in": the kernel keeps pre-activations in fp32
    accumulators (x 2^8); what it holds in fp16 are the layer inputs (unscaled), the weights and biases (x 2^8) and the reverse
    sweep's deltas (x 2^8).  All four are asserted below 65504 for every case.
  - lin6 is no matrix product in any kernel (fp32 FMAs on unsplit operands), so the "f16pair" restatement leaves it in fp32.
  - surf_sdf_smooth has no device-count form and no mask: part D runs plain and idx addressing.
  - "lattice / brick calls with grad, mask or d_n set": surf_sdf_lattice_* / surf_sdf_bricks_* have no such parameters; the
    shared launcher's check for them cannot be reached through the C ABI.  Their other refusals are in part E.
  - the golden checkpoint has no pre-activation below -0.9 at all: its cases are held to the count rule for the two regimes it
    has (curved part, linear branch).

Measured on the CPU (test_measured_margins_are_recorded keeps these lines honest): the largest E / E16 over the cases, per part
    part B sdf     E_B_SDF = 5.70e-07      E16_B_SDF = 7.24e-07
    part B grad    E_B_GRAD = 1.69e-05     E16_B_GRAD = 1.52e-05
    part C sdf     E_C_SDF = 6.85e-07      E16_C_SDF = 7.16e-07
    part D grad    E_D_GRAD = 1.69e-05
    part D smooth  E_D_SMOOTH = 1.31e-03
Seen on an MI355X, largest |kernel - float64| / bound per part and kernel (gradient | forward-only instantiation):
    part B (short, planted, golden scene; all addressing modes)
        f32      0.22 (grad z, edge-pow2)       | 0.19 (sdf, n = 257)
        bf16x3   0.17 (sdf, n = 127)            | 0.17 (sdf, n = 127)
        f16x2    0.18 (sdf, edge-pow2)          | 0.18 (sdf, edge-pow2)
    part B long  f32 0.15 | 0.13    bf16x3 0.13 | 0.13    f16x2 0.13 | 0.12    (grad z | sdf)
    part C lattice   bf16x3 0.20, f16x2 0.17 (both (2, 33, 65))      bricks   bf16x3 0.17, f16x2 0.18 (both res 13, all bricks)
    part D surf_sdf_smooth 0.15 (grad x, n = 301; smooth: 0.15, y, n = 64)
Every kernel stayed inside 8 E (f16x2: 8 max(E, E16)) everywhere: no bound term was added, and no kernel or entry point had to
be changed.  No output row, scratch byte or slab outside a call's own was written in any mode.
"""
import ctypes
import functools
import math
import re
import types

import pytest
import torch

from oracle import surf_oracle as O
from tests.test_sdf_train_kernels import (FACTOR, SENTINEL, VOLSETS, _cell_measure, _g, _mm, _near, corners, edge_points,
                                          encoding_streams, feature_streams, golden, network_f64, one_empty_cell,
                                          random_points, softplus_family, stream_weights, synthetic_layers, volset)

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
TAIL = 4                                            # NaN rows behind every output
SCRATCH_TAIL = 256 * 1024                           # patterned bytes behind the scratch
POOL_N = 301
SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257, 301)
LONG_N = 65536 + 37                                 # the first size at which a workgroup of every variant takes a second round
N_L = (128, 128, 101, 128, 128, 128)
INV_SQRT2 = 1.0 / math.sqrt(2.0)
RSQRT2_F32 = float(torch.tensor(INV_SQRT2, dtype=F32))
W_SCALE = 256.0                                     # Scales<PolH2>::W = ::D
F16_MAX = 65504.0


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------
# A. the forward restatement
# ------------------------------------------------------------------------------------------------------------------


def split16(x, scale):
    """PolH2::split / split_host<PolH2> on x * scale: the fp16 of the value and the fp16 of the fp32 residual, as floats."""
    xs = x * scale
    hi = xs.half().float()
    return hi, (xs - hi).half().float()


def _product(x, Wt, plant, operands):
    """x (Q, n, K) @ Wt (K, N).  "f16pair": three fp16 x fp16 products with fp32 accumulation, smallest terms first, the
    accumulator x 2^8 as the kernel's."""
    if operands == "f16pair":
        xh, xl = split16(x, 1.0)
        wh, wl = split16(Wt, W_SCALE)
        return (xh @ wl + xl @ wh + xh @ wh) * (1.0 / W_SCALE)
    return _mm(x, Wt, plant)


def _inputs(p, vols, tabs, dt, plant, smooth):
    """The input streams (Q, n, 27) and (Q, n, 28): value | [tangent along u] | tangents along x, y, z | [mixed u^T H e_a]."""
    n = p.shape[0]
    enc, phi = [], []
    for a in range(3):
        v = torch.zeros(n, 3, dtype=dt)
        v[:, a] = 1.0
        enc.append(encoding_streams(p, v, dt, plant))
        phi.append(feature_streams(stream_weights(p, v, vols, tabs, dt, plant), vols, dt, n))
    pick = lambda s: [s[0][0]] + ([s[0][1]] if smooth else []) + [s[a][2] for a in range(3)] + ([s[a][3] for a in range(3)] if smooth else [])
    return torch.stack(pick(enc)), torch.stack(pick(phi))


def _forward_chunk(p, L, vols, tabs, dt, operands, plant, smooth, detail):
    f16 = operands == "f16pair"
    enc, phi = _inputs(p, vols, tabs, dt, plant, smooth)
    x, pre, s1s, xs = enc, [], [], []
    for l in range(6):
        W, b = L[l]
        Wt = W.t()
        if f16:
            if l == 3:                              # the packer folds lin3's 1/sqrt(2) into the hidden and encoding columns
                Wt = Wt.clone()
                Wt[:128] = Wt[:128] * RSQRT2_F32
            bh, bl = split16(b, W_SCALE)            # the bias rides the matrix as one more k-element against a 1.0
            b = (bl + bh) * (1.0 / W_SCALE)
        xs.append(x[0])
        a = _product(x, Wt, plant, operands)
        a0 = a[0] + b
        pre.append(a0)
        h, s1, s2, _ = softplus_family(a0)
        s1s.append(s1)
        if smooth:
            out = [h, s1 * a[1]] + [s1 * a[2 + k] for k in range(3)] + [s2 * a[1] * a[2 + k] + s1 * a[5 + k] for k in range(3)]
        else:
            out = [h] + [s1 * a[1 + k] for k in range(3)]
        post = INV_SQRT2 if (l == 2 and plant != "skip_fwd" and not f16) else 1.0
        hq = torch.stack(out) * post
        if l == 2:
            hq = torch.cat([hq, enc * post], dim=-1)
        x = torch.cat([hq, phi], dim=-1)
    xs.append(x[0])
    w6, b6 = L[6][0][0], L[6][1][0]
    y = x @ w6
    t0 = 2 if smooth else 1
    r = types.SimpleNamespace(sdf=y[0] + b6, grad=y[t0:t0 + 3].t(), smooth=y[5:8].t() if smooth else None)
    if detail:
        r.pre, r.s1, r.x = pre, s1s, xs
    return r


def restate_forward(pts, layers, vols, tabs, dt, operands=None, plant=None, smooth=True, detail=False, chunk=4096):
    """sdf (n), grad (n, 3), smooth (n, 3) = H.1 of the SDF network at pts, in dt; vols: (N_s, >= 7) rows, tabs int64 tables.
    plant: a mistake (sensitivity tests).  detail: also the value stream's pre-activations, sp' and layer inputs."""
    assert operands in (None, "f16pair") and (operands is None or dt == F32)
    L = [(W.to(dt), b.to(dt)) for W, b in layers]
    vols = [v[:, :7].to(dt) for v in vols]
    tabs = list(tabs)
    if plant == "absent_kept":                      # an absent level's rows read through level 0's table and not discarded
        vols, tabs = vols + [vols[0]] * (4 - len(vols)), tabs + [tabs[0]] * (4 - len(tabs))
    parts = [_forward_chunk(pts[i:i + chunk].to(dt), L, vols, tabs, dt, operands, plant, smooth, detail)
             for i in range(0, pts.shape[0], chunk)]
    r = types.SimpleNamespace(sdf=torch.cat([q.sdf for q in parts]), grad=torch.cat([q.grad for q in parts]),
                              smooth=torch.cat([q.smooth for q in parts]) if smooth else None)
    if detail:
        r.pre = [torch.cat([q.pre[l] for q in parts]) for l in range(6)]
        r.s1 = [torch.cat([q.s1[l] for q in parts]) for l in range(6)]
        r.x = [torch.cat([q.x[l] for q in parts]) for l in range(7)]
    return r


def deltas_f64(r, layers):
    """d sdf / d pre-activation of lin0..lin5 (n, N_l) from a detailed float64 restatement: what the reverse sweep carries."""
    g = layers[6][0][0].double()[None, :].expand(r.sdf.shape[0], -1)
    out = [None] * 6
    for l in range(6, 0, -1):
        hb = g[:, :N_L[l - 1]] * (INV_SQRT2 if l == 3 else 1.0)
        out[l - 1] = r.s1[l - 1] * hb
        g = out[l - 1] @ layers[l - 1][0].double()
    return out


def columns(r):
    """name -> (n,) column of a restatement's outputs."""
    out = {"sdf": r.sdf}
    out.update({f"grad{a}": r.grad[:, a] for a in range(3)})
    if r.smooth is not None:
        out.update({f"smooth{a}": r.smooth[:, a] for a in range(3)})
    return out


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------

CASES = {}                      # name -> (weights, volume set, n, planted)
_VS = ("pow2", "odd", "empty", "single", "two")
for _i, _n in enumerate(SIZES):
    CASES[f"n{_n}"] = ("synthetic" if _i % 2 == 0 else "golden", _VS[_i % len(_VS)], _n, False)
CASES["edge-pow2"] = ("synthetic", "pow2", 131, True)
CASES["edge-empty"] = ("golden", "empty", 131, True)
CASES["golden-scene"] = ("golden", "scene", 65, False)
CASES["long"] = ("synthetic", "odd", LONG_N, False)
SHORT = [k for k in CASES if k != "long"]
SMOOTH_EXTRA = {"s4": ("golden", "odd", 4, False), "s5": ("synthetic", "two", 5, False)}     # 4 points per wavefront (part D)
CASES.update(SMOOTH_EXTRA)
PLANTED = ("edge-pow2", "edge-empty")


def weights_of(name):
    return synthetic_layers() if name == "synthetic" else golden().layers


def volumes_of(name):
    if name == "scene":
        g = golden()
        return [torch.cat([v, torch.full((v.shape[0], 1), SENTINEL)], 1).contiguous() for v in g.vols], g.tabs
    return volset(name)


@functools.lru_cache(maxsize=None)
def pool(vname):
    """The fixed 301 points that every E of a volume set is also taken over."""
    if vname == "scene":
        return golden().pts[:POOL_N].clone()
    dims = [t.shape[0] for t in volset(vname)[1]]
    return random_points(POOL_N, dims, torch.Generator().manual_seed(77 + sum(map(ord, vname))))[0]


@functools.lru_cache(maxsize=None)
def case(name):
    wname, vname, n, planted = CASES[name]
    g = torch.Generator().manual_seed(3000 + sum(map(ord, name)))
    c = types.SimpleNamespace(name=name, n=n, planted=planted, weights=wname, volset=vname, n_edge=0)
    c.layers = weights_of(wname)
    c.vols, c.tabs = volumes_of(vname)
    if vname == "scene":
        c.pts, c.eps_cell = golden().pts[:n].clone(), None
    else:
        dims = [t.shape[0] for t in c.tabs]
        c.pts, c.eps_cell = random_points(n, dims, g)
        if planted:
            cx = one_empty_cell(c.tabs[0])
            e = torch.cat([edge_points(), torch.tensor([[(ci + f) * 0.25 - 1.0 for ci, f in zip(cx, (0.3125, 0.6875, 0.4375))]], dtype=F32)])
            c.pts[:e.shape[0]] = e
            c.n_edge = e.shape[0]
    c.pts = c.pts.contiguous()
    return c


def _reference(pts, layers, vols, tabs, vname, smooth):
    """float64 outputs at pts and, per output column, E and E16 over pts together with the volume set's pool."""
    allp = torch.cat([pts, pool(vname)])
    r64 = restate_forward(allp, layers, vols, tabs, F64, smooth=smooth)
    c64 = columns(r64)
    c32 = columns(restate_forward(allp, layers, vols, tabs, F32, smooth=smooth))
    c16 = columns(restate_forward(allp, layers, vols, tabs, F32, "f16pair", smooth=False))
    n = pts.shape[0]
    return types.SimpleNamespace(
        col={k: v[:n].clone() for k, v in c64.items()},
        E={k: float((c32[k].double() - c64[k]).abs().max()) for k in c64},
        E16={k: float((c16[k].double() - c64[k]).abs().max()) for k in c16})


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return _reference(c.pts, c.layers, c.vols, c.tabs, c.volset, smooth=name != "long")


def bounds(ref, kernel):
    """name -> the largest admissible |kernel - float64| of an output column."""
    if kernel == "f16x2":
        return {k: FACTOR * max(ref.E[k], ref.E16.get(k, 0.0)) for k in ref.E}
    return {k: FACTOR * v for k, v in ref.E.items()}


# ------------------------------------------------------------------------------------------------------------------
# the comparator: outputs in the kernels' layouts
# ------------------------------------------------------------------------------------------------------------------


def lay_rows(col, n_rows, rows, points=None, plant=None):
    """What a kernel leaves in NaN-filled buffers of n_rows + TAIL rows when it writes the values `col` (name -> per-point float64
    or float32 columns) of the points `points` to the rows `rows` (default: the rows' own points)."""
    rows = torch.as_tensor(rows, dtype=torch.long)
    points = rows if points is None else torch.as_tensor(points, dtype=torch.long)
    out = {}
    for k, v in col.items():
        b = torch.full((n_rows + TAIL,), NAN, dtype=v.dtype)
        b[rows] = v[points]
        if plant == "tail":                          # the clamped last point written behind the last row
            b[n_rows] = v[n_rows - 1] if n_rows - 1 < v.shape[0] else 0.0
        out[k] = b
    return out


def judge(got, want, bound):
    """got / want: name -> flat buffers of equal length; want is float64 with NaN where nothing may be written.
    -> (name -> largest |got - want| / bound, list of structural violations)."""
    ratios, bad = {}, []
    for k, w in want.items():
        g = got[k].double()
        assert g.shape == w.shape, (k, g.shape, w.shape)
        keep = torch.isnan(w)
        if not bool(torch.isnan(g[keep]).all()):
            bad.append(f"{k}: {int((~torch.isnan(g[keep])).sum())} rows written that must stay untouched")
        d = (g[~keep] - w[~keep]).abs()
        if d.numel() == 0:
            ratios[k] = 0.0
        elif not bool(torch.isfinite(d).all()):
            ratios[k] = float("inf")
        else:
            m = float(d.max())
            ratios[k] = m / bound[k] if bound[k] > 0 else (0.0 if m == 0 else float("inf"))
    return ratios, bad


def verdict(got, want, bound):
    r, bad = judge(got, want, bound)
    return max(r.values()) <= 1.0 and not bad


def blocked_order(flags, G, B):
    """The indices surf_compact_blocked emits for an (R, S) flag array: traversal order (ray / G, s / B, ray % G, s % B)."""
    R, S = flags.shape
    out = []
    for rb in range(0, R, G):
        for sb in range(0, S, B):
            for r in range(rb, min(rb + G, R)):
                out += [r * S + s for s in range(sb, sb + B) if flags[r, s]]
    return out


def idx_lists(n):
    """name -> the index lists of part B.3 on n rows (every entry < n)."""
    g = torch.Generator().manual_seed(500 + n)
    flags = torch.rand(9, 16, generator=g) < 0.6
    flags.view(-1)[n:] = False
    flags.view(-1)[min(n, 144) - 1] = True
    return {"third": list(range(0, n, 3)), "blocked": blocked_order(flags, 4, 8), "single": [n // 2]}


def masks(n):
    """name -> the mask patterns of part B.2 (n bytes)."""
    every = torch.zeros(n, dtype=torch.uint8)
    every[::2] = 1
    tile = torch.ones(n, dtype=torch.uint8)
    t0 = 32 * ((n - 1) // 32 // 2)
    tile[t0:t0 + 32] = 0
    lone = torch.ones(n, dtype=torch.uint8)
    lone[t0:t0 + 32] = 0
    lone[min(t0 + 13, n - 1)] = 1
    return {"every-other": every, "tile-out": tile, "single-lane": lone, "none": torch.zeros(n, dtype=torch.uint8)}


def axis_values(m, dims, gen):
    """m axis values: -1, +1 and 1.15 (outside the box) when m >= 3 (+1 when m == 2), the others off every level's planes by
    the _cell_measure rule; in a shuffled order (the kernels take any axis arrays)."""
    special = [-1.0, 1.0, 1.15][:m] if m >= 3 else ([1.0] if m == 2 else [])
    free = random_points(m - len(special), dims, gen)[0][:, 0] if m > len(special) else torch.zeros(0)
    v = torch.cat([torch.tensor(special, dtype=F32), free])
    return v[torch.randperm(m, generator=gen)].contiguous()


def lattice_points(axes):
    return torch.cartesian_prod(*axes).reshape(-1, 3) if all(a.numel() > 0 for a in axes) else torch.zeros(0, 3)


def lay_lattice(vals, shape, sign, x0=0, nx=None, total=None, plant=None):
    """vals: (nx_total ny nz) per-point values of the whole lattice -> the buffer after a call for the slab [x0, x0 + nx)."""
    NX, ny, nz = shape
    nx = NX if nx is None else nx
    V = vals.reshape(NX, ny, nz) * (1.0 if plant == "sign" else sign)
    if plant == "yz":                               # point (ix, iy, iz) read as (ax[ix], ay[iz'], az[iy']) of the transposed walk
        V = V.transpose(1, 2).contiguous().reshape(NX, ny, nz)
    out = torch.full((NX * ny * nz + TAIL,), NAN, dtype=vals.dtype)
    out[x0 * ny * nz:(x0 + nx) * ny * nz] = V[x0:x0 + nx].reshape(-1)
    return {"sdf": out}


def lay_bricks(vals, res, bricks, sign, plant=None):
    """vals: (res^3) lattice values -> out[j 512 + (lx << 6 | ly << 3 | lz)] for the listed bricks, NaN past the upper faces."""
    V = vals.reshape(res, res, res) * sign
    nb = (res + 7) // 8
    out = torch.full((len(bricks) * 512 + TAIL,), NAN, dtype=vals.dtype)
    l = torch.arange(512)
    lx, ly, lz = l >> 6, (l >> 3) & 7, l & 7
    last = res - 1 if plant != "face" else res - 2   # "face": the upper face itself masked out (`<` for `<=`)
    for j, b in enumerate(bricks):
        x, y, z = b // (nb * nb) * 8 + lx, b // nb % nb * 8 + ly, b % nb * 8 + lz
        ok = (x <= last) & (y <= last) & (z <= last)
        slot = (lz << 6 | ly << 3 | lx) if plant == "xz" else l
        out[j * 512 + slot[ok]] = V[x[ok], y[ok], z[ok]]
    return {"sdf": out}


LATTICES = ((1, 1, 1), (3, 5, 7), (2, 33, 65), (5, 1, 9))
_LAT_SETS = (("synthetic", "odd"), ("golden", "pow2"), ("synthetic", "two"), ("golden", "empty"))
BRICK_RES = (8, 13, 17)


@functools.lru_cache(maxsize=None)
def lattice_case(key):
    """key: a shape of LATTICES or a brick resolution.  Axes, the float64 reference at every lattice point, E / E16."""
    if isinstance(key, tuple):
        shape, (wname, vname) = key, _LAT_SETS[LATTICES.index(key)]
    else:
        shape, (wname, vname) = (key,) * 3, _LAT_SETS[BRICK_RES.index(key) + 1]
    gen = torch.Generator().manual_seed(900 + sum(shape) + 7 * shape[0])
    vols, tabs = volumes_of(vname)
    dims = [t.shape[0] for t in tabs]
    c = types.SimpleNamespace(shape=shape, weights=wname, volset=vname, layers=weights_of(wname), vols=vols, tabs=tabs)
    c.axes = [axis_values(m, dims, gen) for m in shape]
    c.pts = lattice_points(c.axes)
    c.ref = _reference(c.pts, c.layers, vols, tabs, vname, smooth=False)
    return c


def brick_lists(res):
    nb = (res + 7) // 8
    g = torch.Generator().manual_seed(res)
    everything = torch.randperm(nb ** 3, generator=g).tolist()
    return {"one": [nb ** 3 - 1], "all": everything, "three": (everything * 3)[:3]}


# ------------------------------------------------------------------------------------------------------------------
# A. anchors and preconditions (CPU)
# ------------------------------------------------------------------------------------------------------------------


def test_restatement_float32_reproduces_the_oracle():
    """dt = float32 on the golden scene's points: sdf and grad of O.sdf_mlp on O.lookup_sparse_volume's gather, smooth of
    O.sdf_mlp_smooth (the oracle sweeps in reverse, the restatement forward: grad and smooth agree to the float32 error E)."""
    c = case("golden-scene")
    vols7 = [v[:, :7].contiguous() for v in c.vols]
    phi, jphi, mphi = O.lookup_sparse_volume(c.pts, vols7, c.tabs, with_mixed=True)
    sdf, grad, _ = O.sdf_mlp(c.layers, c.pts, phi, jphi)
    _, smooth = O.sdf_mlp_smooth(c.layers, c.pts, phi, jphi, mphi)
    r = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32)
    _near(r.sdf, sdf, 64, "sdf")
    ref = reference(c.name)
    for a in range(3):
        dg, ds = float((r.grad[:, a] - grad[:, a]).abs().max()), float((r.smooth[:, a] - smooth[:, a]).abs().max())
        assert dg <= FACTOR * ref.E[f"grad{a}"], ("grad", a, dg, ref.E[f"grad{a}"])
        assert ds <= FACTOR * ref.E[f"smooth{a}"], ("smooth", a, ds, ref.E[f"smooth{a}"])


@pytest.mark.parametrize("name", ["n3", "n33", "n63", "n64", "golden-scene", "edge-pow2", "edge-empty"])
def test_restatement_float64_equals_autograd(name):
    """dt = float64: sdf, grad and smooth = H.1 equal autograd.grad(create_graph=True) through network_f64; on the planted
    lattice-plane points both differentiate the cell the floor picks (one-sided)."""
    c = case(name)
    x = c.pts.double().requires_grad_(True)
    sdf = network_f64(x, [(W.double(), b.double()) for W, b in c.layers], [v[:, :7].double() for v in c.vols], c.tabs)
    grad = torch.autograd.grad(sdf.sum(), x, create_graph=True)[0]
    smooth = torch.autograd.grad(grad.sum(), x)[0]
    ref = reference(name).col
    for k, v in columns(types.SimpleNamespace(sdf=sdf.detach(), grad=grad.detach(), smooth=smooth)).items():
        scale = max(float(v.abs().max()), 1e-300)
        assert float((ref[k] - v).abs().max()) <= 1e-9 * scale, (k, float((ref[k] - v).abs().max()), scale)
    assert float(smooth.abs().max()) > 0


def test_f16pair_restatement_is_a_22_bit_one():
    """The split keeps 22 significant bits of an O(1) operand and drops nothing else: hi + lo reproduces x to 2^-22 |x| (or the
    2^-25 floor of an unscaled second piece), and the "f16pair" outputs differ from the float32 ones, by less than round16's."""
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    hi, lo = split16(x, 1.0)
    assert bool(((hi + lo - x).abs() <= torch.maximum(x.abs() * 2.0 ** -22, torch.tensor(2.0 ** -25))).all())
    hi, lo = split16(x * 1e-3, W_SCALE)
    assert bool((((hi + lo) / W_SCALE - x * 1e-3).abs() <= torch.maximum(x.abs() * 1e-3 * 2.0 ** -22, torch.tensor(2.0 ** -33))).all())
    c = case("n33")
    a = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32)
    b = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32, "f16pair")
    r = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32, plant="round16")
    assert 0 < float((a.sdf - b.sdf).abs().max()) < float((a.sdf - r.sdf).abs().max())


@functools.lru_cache(maxsize=None)
def detailed(name):
    c = case(name)
    return restate_forward(c.pts, c.layers, c.vols, c.tabs, F64, smooth=False, detail=True)


@pytest.mark.parametrize("name", list(CASES))
def test_f16x2_operands_stay_inside_fp16_range(name):
    """What the f16x2 kernel holds in fp16: layer inputs unscaled, weights / biases / reverse-sweep deltas x 2^8."""
    c, r = case(name), detailed(name)
    assert max(float(x.abs().max()) for x in r.x) < F16_MAX
    assert max(float(t.abs().max()) for t in r.pre) < F16_MAX
    assert W_SCALE * max(float(d.abs().max()) for d in deltas_f64(r, c.layers)) < F16_MAX
    assert W_SCALE * max(max(float(W.abs().max()), float(b.abs().max())) for W, b in c.layers) < F16_MAX


@pytest.mark.parametrize("key", LATTICES + BRICK_RES)
def test_f16x2_operands_stay_inside_fp16_range_on_the_lattices(key):
    c = lattice_case(key)
    r = restate_forward(c.pts, c.layers, c.vols, c.tabs, F64, smooth=False, detail=True)
    assert max(float(x.abs().max()) for x in r.x) < F16_MAX and max(float(t.abs().max()) for t in r.pre) < F16_MAX
    assert W_SCALE * max(float(d.abs().max()) for d in deltas_f64(r, c.layers)) < F16_MAX


@pytest.mark.parametrize("name", list(CASES))
def test_weights_exercise_the_softplus_regimes(name):
    """Per hidden layer at least min(64, 4 n) pre-activations on the curved part (|100 t| < 5), on the linear branch
    (100 t > 20) and - synthetic weights - below -0.9 (the exponential underflows in fp32; the golden checkpoint has none)."""
    need = min(64, 4 * case(name).n)
    for l, t in enumerate(detailed(name).pre):
        counts = (int(((100 * t).abs() < 5).sum()), int((100 * t > 20).sum()), int((t < -0.9).sum()))
        assert min(counts if case(name).weights == "synthetic" else counts[:2]) >= need, (name, l, counts, need)


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[1] != "scene"])
def test_points_keep_clear_of_lattice_planes(name):
    """Random points lie farther than EPS_CELL from every level's planes, planted ones are exact: float32 and float64 pick the
    same cell everywhere.  The long case's points are distinct."""
    c = case(name)
    dims = [t.shape[0] for t in c.tabs]
    eps, dist = _cell_measure(c.pts[c.n_edge:], dims)
    assert bool((dist > eps).all()) and c.pts.shape[0] == c.n == CASES[name][2]
    for D in dims:
        assert torch.equal(torch.floor(_g(c.pts, D, F32)).long(), torch.floor(_g(c.pts, D, F64)).long())
    if name == "long":
        assert torch.unique(c.pts, dim=0).shape[0] == LONG_N


@pytest.mark.parametrize("name", PLANTED)
def test_planted_classes_are_present(name):
    c = case(name)
    D = c.tabs[0].shape[0]
    g = _g(c.pts, D, F64)
    fl = torch.floor(g)
    assert int((g == fl).all(1).sum()) >= 1 and int((g == fl).any(1).sum()) >= 3                  # on lattice planes
    assert int((c.pts == 1.0).any(1).sum()) >= 3 and int((c.pts == -1.0).any(1).sum()) >= 3
    assert int((c.pts.abs() > 1.1).any(1).sum()) >= 5                                            # outside the box
    empties = (corners(c.pts.double(), D, c.tabs[0], F64)[0] < 0).sum(1)
    for k in (0, 1, 8):
        assert int((empties == k).sum()) >= 1, k
    lvl = VOLSETS[c.volset][1]
    if lvl is not None:
        assert bool((c.tabs[lvl] < 0).all())


@pytest.mark.parametrize("key", LATTICES + BRICK_RES)
def test_lattice_axes_are_what_they_claim(key):
    c = lattice_case(key)
    dims = [t.shape[0] for t in c.tabs]
    for m, ax in zip(c.shape, c.axes):
        assert ax.shape == (m,)
        if m >= 3:
            assert {-1.0, 1.0} <= set(ax.tolist()) and int((ax.abs() > 1.0).sum()) == 1
        free = ax[(ax.abs() != 1.0)]
        if free.numel():
            eps, dist = _cell_measure(free[:, None].expand(-1, 3), dims)
            assert bool((dist > eps).all())
    for D in dims:
        assert torch.equal(torch.floor(_g(c.pts, D, F32)).long(), torch.floor(_g(c.pts, D, F64)).long())
    if isinstance(key, tuple) and key != (1, 1, 1):
        assert len(set(key)) == 3                                               # axes of unequal length


def test_index_lists_and_masks_are_what_they_claim():
    for n in SIZES:
        L = idx_lists(n)
        assert all(0 <= i < n for l in L.values() for i in l) and all(len(set(l)) == len(l) > 0 for l in L.values())
        M = masks(n)
        assert int(M["none"].sum()) == 0 and int(M["every-other"].sum()) == (n + 1) // 2
        if n > 64:
            tiles = M["single-lane"][:n // 32 * 32].reshape(-1, 32).sum(1)
            assert int((tiles == 1).sum()) == 1 and int((M["tile-out"][:n // 32 * 32].reshape(-1, 32).sum(1) == 0).sum()) == 1
    big = idx_lists(301)["blocked"]
    assert big != sorted(big) and sorted(big) == sorted(set(big))                   # non-monotonic


# ------------------------------------------------------------------------------------------------------------------
# sensitivity (CPU): the comparator rejects planted mistakes
# ------------------------------------------------------------------------------------------------------------------

FORWARD_PLANTS = ("skip_fwd", "cos_sign", "empty_row0", "unclamped", "round16")


def _plain(c, col):
    return lay_rows(col, c.n, range(c.n))


def _restated(c, **kw):
    return columns(restate_forward(c.pts, c.layers, c.vols, c.tabs, F32, **kw))


@pytest.mark.parametrize("name", ["edge-pow2", "n33", "n1", "golden-scene"])
def test_comparator_accepts_the_float32_restatements(name):
    c, ref = case(name), reference(name)
    want = _plain(c, ref.col)
    r, bad = judge(_plain(c, _restated(c)), want, bounds(ref, "f32"))
    assert not bad and max(r.values()) <= 1.0 / FACTOR + 1e-12, r
    want16 = {k: v for k, v in want.items() if not k.startswith("smooth")}
    r, bad = judge(_plain(c, _restated(c, operands="f16pair", smooth=False)), want16, bounds(ref, "f16x2"))
    assert not bad and max(r.values()) <= 1.0 / FACTOR + 1e-12, r


@pytest.mark.parametrize("plant", FORWARD_PLANTS)
def test_comparator_rejects_a_planted_mistake(plant):
    """skip_fwd: the skip connection's 1/sqrt(2) dropped; cos_sign: the cosine tangent's sign; empty_row0: an empty corner read
    as row 0; unclamped: the upper corner index not clamped at +1; round16: operands of every product rounded to 16 significant
    bits (a dropped split product) - rejected under the f16x2 bound too."""
    c, ref = case("edge-pow2"), reference("edge-pow2")
    got, want = _plain(c, _restated(c, plant=plant)), _plain(c, ref.col)
    assert not verdict(got, want, bounds(ref, "f32")), plant
    if plant == "round16":                          # (on the golden checkpoint: the synthetic weights' own E is 16 ulps of the sdf)
        c, ref = case("edge-empty"), reference("edge-empty")
        want16 = {k: v for k, v in _plain(c, ref.col).items() if not k.startswith("smooth")}
        assert not verdict(_plain(c, _restated(c, plant=plant)), want16, bounds(ref, "f16x2"))


def test_comparator_rejects_an_absent_level_that_is_kept():
    c, ref = case("n32"), reference("n32")
    assert c.volset == "two" and len(c.tabs) == 2
    assert not verdict(_plain(c, _restated(c, plant="absent_kept")), _plain(c, ref.col), bounds(ref, "f32"))


def test_comparator_rejects_addressing_mistakes():
    """Value scattered to the slot instead of idx[slot]; device count ignored (capacity used); a write behind row n."""
    c, ref = case("n301"), reference("n301")
    got32, b = _restated(c), bounds(ref, "f32")
    idx = idx_lists(c.n)["blocked"]
    want = lay_rows(ref.col, c.n, idx)
    assert verdict(lay_rows(got32, c.n, idx), want, b)
    assert not verdict(lay_rows(got32, c.n, range(len(idx)), points=idx), want, b)
    perm = torch.randperm(c.n, generator=torch.Generator().manual_seed(5)).tolist()
    want = lay_rows(ref.col, c.n, perm[:31])
    assert verdict(lay_rows(got32, c.n, perm[:31]), want, b) and not verdict(lay_rows(got32, c.n, perm), want, b)
    assert not verdict(lay_rows(got32, c.n, range(c.n), plant="tail"), _plain(c, ref.col), b)


def test_comparator_rejects_lattice_and_brick_mistakes():
    """Lattice y / z transposed; sign dropped; brick local index with the x and z bit fields swapped; upper-face mask off by one."""
    c = lattice_case((3, 5, 7))
    got = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32, smooth=False).sdf
    b = {"sdf": FACTOR * c.ref.E["sdf"]}
    want = lay_lattice(c.ref.col["sdf"], c.shape, -1.0, x0=1, nx=1)
    assert verdict(lay_lattice(got, c.shape, -1.0, x0=1, nx=1), want, b)
    assert not verdict(lay_lattice(got, c.shape, -1.0, x0=1, nx=1, plant="yz"), want, b)
    assert not verdict(lay_lattice(got, c.shape, -1.0, x0=1, nx=1, plant="sign"), want, b)
    assert not verdict(lay_lattice(got, c.shape, -1.0, x0=1, nx=2), want, b)                     # a neighbouring slab written
    c = lattice_case(13)
    got = restate_forward(c.pts, c.layers, c.vols, c.tabs, F32, smooth=False).sdf
    b = {"sdf": FACTOR * c.ref.E["sdf"]}
    bricks = brick_lists(13)["all"]
    want = lay_bricks(c.ref.col["sdf"], 13, bricks, 1.0)
    assert verdict(lay_bricks(got, 13, bricks, 1.0), want, b)
    assert not verdict(lay_bricks(got, 13, bricks, 1.0, plant="xz"), want, b)
    assert not verdict(lay_bricks(got, 13, bricks, 1.0, plant="face"), want, b)


# ------------------------------------------------------------------------------------------------------------------
# recorded margins
# ------------------------------------------------------------------------------------------------------------------


def _recorded(label):
    return float(re.search(r"\b" + label + r"\s*=\s*([0-9.e+-]+)", __doc__).group(1))


def measured():
    m = {}
    B = [reference(k) for k in CASES if k not in SMOOTH_EXTRA]
    C = [lattice_case(k).ref for k in LATTICES + BRICK_RES]
    D = [reference(k) for k in list(SHORT) + list(SMOOTH_EXTRA)]
    top = lambda refs, attr, keys: max(getattr(r, attr)[k] for r in refs for k in keys)
    g3, s3 = ("grad0", "grad1", "grad2"), ("smooth0", "smooth1", "smooth2")
    m["E_B_SDF"], m["E16_B_SDF"] = top(B, "E", ["sdf"]), top(B, "E16", ["sdf"])
    m["E_B_GRAD"], m["E16_B_GRAD"] = top(B, "E", g3), top(B, "E16", g3)
    m["E_C_SDF"], m["E16_C_SDF"] = top(C, "E", ["sdf"]), top(C, "E16", ["sdf"])
    m["E_D_GRAD"], m["E_D_SMOOTH"] = top(D, "E", g3), top(D, "E", s3)
    return m


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

KERNELS = ("f32", "bf16x3", "f16x2")
SPLIT = ("bf16x3", "f16x2")
ENTRY = {"f32": "surf_sdf_mlp", "bf16x3": "surf_sdf_mlp_bf16x3", "f16x2": "surf_sdf_mlp_f16x2"}
SCRATCH_FN = {"f32": "surf_sdf_scratch_bytes", "bf16x3": "surf_sdf_bf16_scratch_bytes", "f16x2": "surf_sdf_f16_scratch_bytes"}
_WORST = {}                      # (part, kernel) -> (ratio, where)


def _note(part, kernel, ratios, where):
    top = max(ratios.items(), key=lambda kv: kv[1])
    if top[1] > _WORST.get((part, kernel), (-1.0, ""))[0]:
        _WORST[(part, kernel)] = (top[1], f"{top[0]}, {where}")
        print(f"[margin] part {part} {kernel}: {top[1]:.3f} ({top[0]}, {where})")


@functools.lru_cache(maxsize=None)
def _packed(wname, kernel):
    from surf_amd import ops
    layers = weights_of(wname)
    if kernel == "f32":
        host = ops.sdf_pack_weights_host(layers)
    elif kernel == "smooth":
        host = ops.sdf_smooth_pack_weights_host(layers)
    else:
        host = ops.sdf_pack_weights_split_host(layers, kernel)
    return torch.from_numpy(host).to(dev())


@functools.lru_cache(maxsize=None)
def _volumes(vname):
    from surf_amd import ops
    vols, tabs = volumes_of(vname)
    sv = ops.SparseVolumes([v.to(dev()) for v in vols], [t.to(dev()) for t in tabs])
    assert all(v.shape[1] == 8 for v in sv.vols) and sv.n == len(vols)
    return sv


@functools.lru_cache(maxsize=None)
def _points(name):
    return case(name).pts.to(dev())


def _nan(numel):
    return torch.full((numel,), NAN, dtype=F32, device=dev())


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=dev())


def point_launch(kernel, want_grad, name, mask=None, idx=None, count=None, scratch_fill=0, n=None):
    """One launch of a point-mode entry point on test-owned buffers.  -> (name -> flat CPU buffers of n_rows + TAIL rows,
    raw bits of sdf | grad).  idx: the list passed (its length is n, or the capacity with `count` = the device count)."""
    from surf_amd import _lib, ops
    L, c = _lib.lib(), case(name)
    sv, packed, pts = _volumes(c.volset), _packed(c.weights, kernel), _points(name)
    n_eval = (c.n if idx is None else len(idx)) if n is None else n
    sdf = _nan(c.n + TAIL)
    grad = _nan((c.n + TAIL) * 3) if want_grad else None
    scratch = None
    if want_grad:
        need = int(getattr(L, SCRATCH_FN[kernel])(n_eval))
        scratch = torch.empty(need + SCRATCH_TAIL, dtype=torch.uint8, device=dev())
        scratch[:need] = scratch_fill
        pattern = (torch.arange(SCRATCH_TAIL, device=dev()) * 37 + 11).to(torch.uint8)
        scratch[need:] = pattern
    d_idx = None if idx is None else _i32(idx)
    d_mask = None if mask is None else mask.to(dev())
    d_n = None if count is None else _i32([count])
    try:
        if count is not None:
            getattr(L, ENTRY[kernel] + "_dn")(ops._p(pts), ops._p(d_idx), n_eval, ops._p(d_n), sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed),
                                              ops._p(sdf), ops._p(grad), ops._p(scratch), ops._stream())
        else:
            getattr(L, ENTRY[kernel])(ops._p(pts), ops._p(d_mask), ops._p(d_idx), n_eval, sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed),
                                      ops._p(sdf), ops._p(grad), ops._p(scratch), ops._stream())
    finally:
        torch.cuda.synchronize()
    if want_grad:
        assert torch.equal(scratch[need:], pattern), "bytes behind the scratch changed"
    out = {"sdf": sdf.cpu()}
    bits = [sdf.cpu().view(torch.int32)]
    if want_grad:
        g = grad.cpu().reshape(-1, 3)
        out.update({f"grad{a}": g[:, a].contiguous() for a in range(3)})
        bits.append(grad.cpu().view(torch.int32))
    return out, torch.cat(bits)


def _check_rows(part, kernel, want_grad, name, got, rows, what=""):
    c, ref = case(name), reference(name)
    keys = ["sdf"] + (["grad0", "grad1", "grad2"] if want_grad else [])
    want = lay_rows({k: ref.col[k] for k in keys}, c.n, rows)
    r, bad = judge(got, want, bounds(ref, kernel))
    _note(part, kernel + ("" if want_grad else " fwd"), r, f"{name} {what}".strip())
    assert not bad, (name, what, bad)
    assert max(r.values()) <= 1.0, (name, what, r)


VARIANTS = [(k, g) for k in KERNELS for g in (True, False)]
_vid = lambda v: f"{v[0]}-{'grad' if v[1] else 'fwd'}"


@gpu
@pytest.mark.parametrize("name", SHORT)
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_point_mode_plain(variant, name):
    """Part B.1: mask = idx = NULL.  Every row within the bound of float64, the rows behind row n and the bytes behind the
    scratch untouched."""
    kernel, want_grad = variant
    got, _ = point_launch(kernel, want_grad, name)
    _check_rows("B", kernel, want_grad, name, got, range(case(name).n))


@gpu
@pytest.mark.parametrize("pattern", ["every-other", "tile-out", "single-lane", "none"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_point_mode_mask(variant, pattern):
    """Part B.2: mask given, no compaction, on every short case.  Masked rows keep their NaN."""
    kernel, want_grad = variant
    for name in SHORT:
        m = masks(case(name).n)[pattern]
        got, _ = point_launch(kernel, want_grad, name, mask=m)
        _check_rows("B", kernel, want_grad, name, got, m.nonzero()[:, 0].tolist(), "mask " + pattern)


@gpu
@pytest.mark.parametrize("which", ["third", "blocked", "single"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_point_mode_idx(variant, which):
    """Part B.3: idx lists on every short case.  Rows in idx hold the value of that row's point, the others keep their NaN."""
    kernel, want_grad = variant
    for name in SHORT:
        idx = idx_lists(case(name).n)[which]
        got, _ = point_launch(kernel, want_grad, name, idx=idx)
        _check_rows("B", kernel, want_grad, name, got, idx, "idx " + which)


@gpu
def test_blocked_list_is_the_compaction_kernels():
    """The non-monotonic list of part B.3 is what surf_compact_blocked emits (G = 4, B = 8 on (R, S) = (9, 16))."""
    from surf_amd import ops
    g = torch.Generator().manual_seed(500 + 301)
    flags = torch.rand(9, 16, generator=g) < 0.6
    flags.view(-1)[143] = True
    idx, total = ops.compact_counted(flags.to(torch.uint8).reshape(-1).to(dev()), block=(16, 4, 8))
    torch.cuda.synchronize()
    assert idx[:int(total.item())].tolist() == blocked_order(flags, 4, 8) == idx_lists(301)["blocked"]


@gpu
@pytest.mark.parametrize("count", [0, 1, 31, 32, 300, 301])
@pytest.mark.parametrize("want_grad", [True, False], ids=["grad", "fwd"])
@pytest.mark.parametrize("kernel", SPLIT)
def test_point_mode_device_count(kernel, want_grad, count):
    """Part B.4: capacity 301, the count read from device memory.  idx is a permutation of the 301 rows: the entries beyond the
    count are valid, distinct rows, which must keep their NaN."""
    perm = torch.randperm(301, generator=torch.Generator().manual_seed(5)).tolist()
    got, _ = point_launch(kernel, want_grad, "n301", idx=perm, count=count)
    _check_rows("B", kernel, want_grad, "n301", got, perm[:count], f"d_n = {count}")


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_long_case_second_rounds(kernel):
    """n = 65,536 + 37 distinct points: some workgroup of every variant (256 x 256, 256 x 128, 512 x 128 points per sweep of the
    grid) takes a second round, the last tile is ragged.  sdf and grad per element; the launch repeated gives the same bits."""
    got, bits = point_launch(kernel, True, "long")
    _check_rows("B long", kernel, True, "long", got, range(LONG_N))
    assert torch.equal(point_launch(kernel, True, "long")[1], bits)
    got, _ = point_launch(kernel, False, "long")
    _check_rows("B long", kernel, False, "long", got, range(LONG_N))


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_repeated_launch_and_dirty_scratch_give_the_same_bits(kernel):
    """n = 301, gradient kernels: the same launch twice is bit-equal (dealing must not show), and so is a launch on scratch
    pre-filled with 0xFF bytes (the header: contents need not be preserved)."""
    _, a = point_launch(kernel, True, "n301")
    _, b = point_launch(kernel, True, "n301")
    _, f = point_launch(kernel, True, "n301", scratch_fill=0xFF)
    assert torch.equal(a, b) and torch.equal(a, f)


# ---- part C ----------------------------------------------------------------------------------------------------------


def lattice_launch(kernel, c, sign, x0=0, nx=None):
    from surf_amd import _lib, ops
    NX, ny, nz = c.shape
    nx = NX if nx is None else nx
    sv, packed = _volumes(c.volset), _packed(c.weights, kernel)
    axes = [a.to(dev()) for a in c.axes]
    out = _nan(NX * ny * nz + TAIL)
    try:
        getattr(_lib.lib(), f"surf_sdf_lattice_{kernel}")(ops._p(axes[0][x0:]), ops._p(axes[1]), ops._p(axes[2]), nx, ny, nz, sv._vp, sv._tp,
                                                         sv._dp, sv.n, ops._p(packed), ops._p(out[x0 * ny * nz:]), float(sign), ops._stream())
    finally:
        torch.cuda.synchronize()
    return {"sdf": out.cpu()}


@gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("shape", LATTICES)
@pytest.mark.parametrize("kernel", SPLIT)
def test_lattice(kernel, shape, sign):
    """Part C: out[(ix ny + iy) nz + iz] = sign * sdf(ax[ix], ay[iy], az[iz]) on axes of unequal length, whole and as a slab
    (x0 > 0, nx less than the tensor's: the other slabs keep their NaN)."""
    c = lattice_case(shape)
    b = {"sdf": bounds(c.ref, kernel)["sdf"]}
    slabs = [(0, None)] + ([(1, max(1, shape[0] - 2))] if shape[0] > 1 else [])
    for x0, nx in slabs:
        got = lattice_launch(kernel, c, sign, x0, nx)
        r, bad = judge(got, lay_lattice(c.ref.col["sdf"], shape, sign, x0, nx), b)
        _note("C lattice", kernel, r, f"{shape} x0 = {x0}")
        assert not bad, bad
        assert max(r.values()) <= 1.0, r


@gpu
@pytest.mark.parametrize("which", ["one", "all", "three"])
@pytest.mark.parametrize("res", BRICK_RES)
@pytest.mark.parametrize("kernel", SPLIT)
def test_bricks(kernel, res, which):
    """Part C: brick mode on unordered lists; points with a coordinate >= res keep their NaN; every written value is bit-equal
    to the lattice kernel's at the same lattice point (the header's claim) and within the bound of float64."""
    from surf_amd import _lib, ops
    c = lattice_case(res)
    bricks = brick_lists(res)[which]
    sv, packed = _volumes(c.volset), _packed(c.weights, kernel)
    axes = [a.to(dev()) for a in c.axes]
    out = _nan(len(bricks) * 512 + TAIL)
    d_bricks = _i32(bricks)
    try:
        getattr(_lib.lib(), f"surf_sdf_bricks_{kernel}")(ops._p(axes[0]), ops._p(axes[1]), ops._p(axes[2]), res, ops._p(d_bricks),
                                                        len(bricks),
                                                        sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed), ops._p(out), -1.0, ops._stream())
    finally:
        torch.cuda.synchronize()
    got = {"sdf": out.cpu()}
    want = lay_bricks(c.ref.col["sdf"], res, bricks, -1.0)
    r, bad = judge(got, want, {"sdf": bounds(c.ref, kernel)["sdf"]})
    _note("C bricks", kernel, r, f"res {res} {which}")
    assert not bad, bad
    assert max(r.values()) <= 1.0, r
    lat = lattice_launch(kernel, c, -1.0)["sdf"][:res ** 3]
    same = lay_bricks(lat, res, bricks, 1.0)["sdf"]
    assert torch.equal(torch.isnan(same), torch.isnan(got["sdf"]))
    assert torch.equal(torch.nan_to_num(same, nan=7.0).view(torch.int32), torch.nan_to_num(got["sdf"], nan=7.0).view(torch.int32))


# ---- part D ----------------------------------------------------------------------------------------------------------


def smooth_launch(name, idx=None, want_grad=True):
    from surf_amd import _lib, ops
    c = case(name)
    sv, packed, pts = _volumes(c.volset), _packed(c.weights, "smooth"), _points(name)
    grad = _nan((c.n + TAIL) * 3) if want_grad else None
    smooth = _nan((c.n + TAIL) * 3)
    d_idx = None if idx is None else _i32(idx)
    try:
        _lib.lib().surf_sdf_smooth(ops._p(pts), ops._p(d_idx), c.n if idx is None else len(idx), sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed),
                                   ops._p(grad), ops._p(smooth), ops._stream())
    finally:
        torch.cuda.synchronize()
    out = {f"smooth{a}": smooth.cpu().reshape(-1, 3)[:, a].contiguous() for a in range(3)}
    if want_grad:
        out.update({f"grad{a}": grad.cpu().reshape(-1, 3)[:, a].contiguous() for a in range(3)})
    return out


def _check_smooth(name, got, rows, what):
    c, ref = case(name), reference(name)
    want = lay_rows({k: ref.col[k] for k in got}, c.n, rows)
    r, bad = judge(got, want, bounds(ref, "f32"))
    _note("D", "smooth", r, f"{name} {what}")
    assert not bad, (name, what, bad)
    assert max(r.values()) <= 1.0, (name, what, r)


@gpu
@pytest.mark.parametrize("name", SHORT + list(SMOOTH_EXTRA))
def test_smooth_plain(name):
    """Part D: grad and smooth = H.1 of surf_sdf_smooth within the fp32 bound of float64; grad = NULL leaves smooth the same."""
    got = smooth_launch(name)
    _check_smooth(name, got, range(case(name).n), "plain")
    alone = smooth_launch(name, want_grad=False)
    assert set(alone) == {"smooth0", "smooth1", "smooth2"}
    assert all(torch.equal(alone[k].view(torch.int32), got[k].view(torch.int32)) for k in alone)


@gpu
@pytest.mark.parametrize("which", ["third", "blocked", "single"])
def test_smooth_idx(which):
    """Part D: idx lists as in B.3; rows not listed keep their NaN."""
    for name in SHORT + list(SMOOTH_EXTRA):
        idx = idx_lists(case(name).n)[which]
        _check_smooth(name, smooth_launch(name, idx=idx), idx, "idx " + which)


# ---- part E ----------------------------------------------------------------------------------------------------------


def _refused(fn, args, code):
    from surf_amd import _lib
    kind = {"arg": "invalid argument", "limit": "exceeds a SURF_MAX_"}[code]
    with pytest.raises(_lib.SurfHipError, match=re.escape(kind)):
        fn(*args)


@gpu
@pytest.mark.parametrize("kernel", KERNELS + ("smooth",))
def test_point_refusals(kernel):
    """Part E: every documented SURF_E_ARG / SURF_E_LIMIT of the point-mode entry points returns its code and leaves the
    NaN-filled outputs untouched (nothing is launched)."""
    from surf_amd import _lib, ops
    L, c = _lib.lib(), case("n33")
    sv, packed, pts = _volumes(c.volset), _packed(c.weights, kernel), _points("n33")
    assert sv.n == 4
    out, grad, scratch = _nan(c.n + TAIL), _nan(3 * (c.n + TAIL)), torch.zeros(1 << 22, dtype=torch.uint8, device=dev())
    null = ctypes.c_void_p(0)
    five = lambda arr, ct: (ct * 5)(*(list(arr) + [arr[0]]))
    dims = lambda *d: (ctypes.c_int * 4)(*d)
    base = dict(pts=ops._p(pts), mask=null, idx=null, n=c.n, vols=sv._vp, tabs=sv._tp, dims=sv._dp, n_vol=4, packed=ops._p(packed),
                sdf=ops._p(out), grad=ops._p(grad), scratch=ops._p(scratch))

    def call(**over):
        a = dict(base, **over)
        if kernel == "smooth":
            return (L.surf_sdf_smooth, (a["pts"], a["idx"], a["n"], a["vols"], a["tabs"], a["dims"], a["n_vol"], a["packed"], a["grad"],
                                        a["sdf"],
                                        ops._stream()))
        return (getattr(L, ENTRY[kernel]), (a["pts"], a["mask"], a["idx"], a["n"], a["vols"], a["tabs"], a["dims"], a["n_vol"], a["packed"],
                                            a["sdf"], a["grad"], a["scratch"], ops._stream()))

    cases = [("arg", dict(n=0)), ("arg", dict(n=-3)), ("arg", dict(n_vol=0)),
             ("limit", dict(n_vol=5, vols=five(sv._vp, ctypes.c_void_p), tabs=five(sv._tp, ctypes.c_void_p),
                            dims=five(sv._dp, ctypes.c_int))),
             ("arg", dict(dims=dims(sv.dims[0], 1, sv.dims[2], sv.dims[3]))), ("arg", dict(dims=dims(0, *sv.dims[1:]))),
             ("arg", dict(pts=null)), ("arg", dict(packed=null)), ("arg", dict(sdf=null)),
             ("arg", dict(vols=None)), ("arg", dict(tabs=None)), ("arg", dict(dims=None))]
    if kernel in SPLIT:
        cases.append(("limit", dict(dims=dims(1025, *sv.dims[1:]))))
    if kernel != "smooth":
        cases.append(("arg", dict(scratch=null)))
    for code, over in cases:
        _refused(*call(**over), code)
    if kernel in SPLIT:
        idx, d_n = _i32(range(c.n)), _i32([c.n])
        dn = getattr(L, ENTRY[kernel] + "_dn")
        args = lambda **o: tuple(dict(dict(base, idx=ops._p(idx), d_n=ops._p(d_n)), **o)[k] for k in
                                 ("pts", "idx", "n", "d_n", "vols", "tabs", "dims", "n_vol", "packed", "sdf", "grad",
                                  "scratch")) + (ops._stream(),)
        for code, over in [("arg", dict(idx=null)), ("arg", dict(d_n=null)), ("arg", dict(n=0)), ("arg", dict(scratch=null)),
                           ("arg", dict(n_vol=0))]:
            _refused(dn, args(**over), code)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(grad).all())


@gpu
@pytest.mark.parametrize("kernel", SPLIT)
def test_lattice_and_brick_refusals(kernel):
    """Part E: the lattice / brick entry points.  (They have no grad, mask or d_n parameter: those refusals of the shared
    launcher cannot be reached from the C ABI.)  A point count >= 2^31 is refused by its size alone."""
    from surf_amd import _lib, ops
    L = _lib.lib()
    c = lattice_case((3, 5, 7))
    sv, packed = _volumes(c.volset), _packed(c.weights, kernel)
    keep = [a.to(dev()) for a in c.axes]
    axes = [ops._p(a) for a in keep]
    out = _nan(3 * 5 * 7 + 512 + TAIL)
    bricks = _i32([0])
    null = ctypes.c_void_p(0)
    lat, brk = getattr(L, f"surf_sdf_lattice_{kernel}"), getattr(L, f"surf_sdf_bricks_{kernel}")
    tail = (sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed), ops._p(out), -1.0, ops._stream())
    for code, (ax, ay, az, nx, ny, nz) in [("arg", (*axes, 3, 0, 7)), ("arg", (*axes, 0, 5, 7)), ("arg", (*axes, 3, 5, -1)),
                                           ("arg", (null, axes[1], axes[2], 3, 5, 7)), ("arg", (axes[0], null, axes[2], 3, 5, 7)),
                                           ("arg", (axes[0], axes[1], null, 3, 5, 7)), ("arg", (*axes, 2048, 1024, 1024))]:
        _refused(lat, (ax, ay, az, nx, ny, nz) + tail, code)
    _refused(lat, (*axes, 3, 5, 7, sv._vp, sv._tp, sv._dp, 0) + tail[4:], "arg")
    _refused(lat, (*axes, 3, 5, 7, sv._vp, sv._tp, sv._dp, sv.n, ops._p(packed), null, -1.0, ops._stream()), "arg")
    for code, (ax, res, bl, nb) in [("arg", (axes[0], 1, ops._p(bricks), 1)), ("arg", (axes[0], 8, null, 1)),
                                    ("arg", (axes[0], 8, ops._p(bricks), 0)),
                                    ("arg", (null, 8, ops._p(bricks), 1)), ("limit", (axes[0], 8, ops._p(bricks), 1 << 22))]:
        _refused(brk, (ax, axes[1], axes[2], res, bl, nb) + tail, code)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
