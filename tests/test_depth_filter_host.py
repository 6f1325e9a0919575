"""CPU: the multi-view geometric-consistency filter of surf_amd.fusion - pair_transforms, consistency_host (the numpy-fp32 mirror
of the rule written out in csrc/depth_filter.hip's header comment), filter_views(backend="host"), nearest_sources - on analytic
sphere scenes, against a float64 restatement of the same rule, and the two new entry points of the library.
tests/test_depth_filter_gpu.py compares the device path with these."""
import os

import numpy as np
import pytest

from surf_amd import fusion
from surf_amd.fusion import DepthView
from tests.test_fusion_host import look_at

F32_MAX = float(np.finfo(np.float32).max)
MARGIN = 1e-3            # a (pixel, source) pair is "clear" when e2 and rel are further than this (relative) from their thresholds
GEO = 1e-4               # ... and sx, sy further than this many pixels from a map border and from an integer (a change of taps)


def sphere_depth(K, w2c, H, W, radius=0.5):
    """z-depth (H, W) float64 of the sphere |p| = radius seen from the camera (0 where a ray misses it)."""
    c2w = np.linalg.inv(w2c)
    c = c2w[:3, 3]
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ np.linalg.inv(K).T @ c2w[:3, :3].T   # z component 1: the parameter is z-depth
    b, cc, aa = d @ c, c @ c - radius * radius, (d * d).sum(-1)
    disc = b * b - aa * cc
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / aa, 0.0)
    return np.where(t > 0, t, 0.0)


def sphere_view(centre, f, H, W, dscale=1.0, radius=0.5):
    """The DepthView of a pinhole camera at `centre` looking at the sphere; the stored depth is z-depth / dscale."""
    K, w2c = look_at(centre, f, H, W)
    return DepthView((K @ w2c[:3, :4]).astype(np.float32), (sphere_depth(K, w2c, H, W, radius) / dscale).astype(np.float32), dscale)


def ring_centres(n, radius=1.5, height=2.0):
    """n camera centres on a ring about the y axis, 2.5 from the origin and 37 degrees off the axis: with n = 6 neighbouring
    cameras look along directions 35 degrees apart, opposite ones 74, so most of what one camera sees several others see too."""
    return [(radius * np.sin(2 * np.pi * i / n), height, -radius * np.cos(2 * np.pi * i / n)) for i in range(n)]


def sphere_ring(n=6, H=40, W=56, f=80.0):
    """The exact scene: a sphere of radius 0.5 (about 33 pixels across), n ring cameras, analytic depth."""
    return [sphere_view(c, f, H, W) for c in ring_centres(n)]


def rule_f64(views, r, s, px_thresh=1.0, rel_thresh=0.01):
    """The rule of depth_filter.hip's header comment for the pair (r -> s) in float64, from the same fp32 inputs (depths, dscale,
    pair_transforms).  Returns (verdict, near, sx, sy): the pair's verdict per pixel of r, whether one of the chain's decisions
    lies within MARGIN / GEO of flipping (where fp32 may decide otherwise), and the projection into s."""
    A_rs, b_rs, A_sr, b_sr = (a.astype(np.float64) for a in fusion.pair_transforms(views[r], views[s]))
    d = np.asarray(views[r].depth, np.float64) * float(np.float32(views[r].dscale))
    depth_s = np.asarray(views[s].depth, np.float64) * float(np.float32(views[s].dscale))
    (H, W), (Hs, Ws) = d.shape, depth_s.shape
    with np.errstate(all="ignore"):
        measured = (d > 0) & (d <= F32_MAX)
        yy, xx = np.mgrid[:H, :W].astype(np.float64)
        u = np.stack([xx * d, yy * d, d], axis=-1) @ A_rs.T + b_rs
        sx, sy = u[..., 0] / u[..., 2], u[..., 1] / u[..., 2]
        ok = measured & (u[..., 2] > 0) & (sx >= 0) & (sx <= Ws - 1) & (sy >= 0) & (sy <= Hs - 1)
        near = measured & ((np.abs(u[..., 2]) < 1e-3) | (np.abs(sx - np.rint(sx)) < GEO) | (np.abs(sy - np.rint(sy)) < GEO))
        x0, y0 = np.where(ok, np.floor(sx), 0).astype(int), np.where(ok, np.floor(sy), 0).astype(int)
        x1, y1 = np.minimum(x0 + 1, Ws - 1), np.minimum(y0 + 1, Hs - 1)
        fx, fy = sx - x0, sy - y0
        taps = [depth_s[y0, x0], depth_s[y0, x1], depth_s[y1, x0], depth_s[y1, x1]]
        for t in taps:
            ok &= (t > 0) & (t <= F32_MAX)
        top, bot = taps[0] + (taps[1] - taps[0]) * fx, taps[2] + (taps[3] - taps[2]) * fx
        ds = top + (bot - top) * fy
        w = np.stack([sx * ds, sy * ds, ds], axis=-1) @ A_sr.T + b_sr
        ok &= w[..., 2] > 0
        e2 = (w[..., 0] / w[..., 2] - xx) ** 2 + (w[..., 1] / w[..., 2] - yy) ** 2
        rel = np.abs(w[..., 2] - d) / d
        px2 = float(np.float32(px_thresh) * np.float32(px_thresh))
        rel_thresh = float(np.float32(rel_thresh))
        near |= ok & ((np.abs(w[..., 2]) < 1e-3) | (np.abs(e2 / px2 - 1) <= MARGIN) | (np.abs(rel / rel_thresh - 1) <= MARGIN))
        return ok & (e2 < px2) & (rel < rel_thresh), near, sx, sy


@pytest.fixture(scope="module")
def ring():
    """(views, per view (count, zsum) of the mirror against every other view in index order)."""
    views = sphere_ring()
    return views, [fusion.consistency_host(views, r, [s for s in range(len(views)) if s != r]) for r in range(len(views))]


def test_pair_transforms_map_one_projection_to_the_other():
    g = np.random.default_rng(0)
    a = sphere_view((0.3, 0.4, -2.5), 80.0, 40, 56)
    b = sphere_view((2.0, -0.3, -1.4), 95.0, 37, 53, dscale=2.5)
    A_rs, b_rs, A_sr, b_sr = fusion.pair_transforms(a, b)
    assert all(t.dtype == np.float32 for t in (A_rs, b_rs, A_sr, b_sr)) and A_rs.shape == A_sr.shape == (3, 3) and b_rs.shape == (3,)
    X = g.uniform(-0.5, 0.5, (200, 3))                                   # in front of both cameras
    Pa, Pb = a.P.astype(np.float64), b.P.astype(np.float64)
    qa, qb = X @ Pa[:, :3].T + Pa[:, 3], X @ Pb[:, :3].T + Pb[:, 3]
    assert qa[:, 2].min() > 1.0 and qb[:, 2].min() > 1.0
    for A, t, src, dst in ((A_rs, b_rs, qa, qb), (A_sr, b_sr, qb, qa)):
        got = src @ A.astype(np.float64).T + t.astype(np.float64)
        err = float((np.abs(got - dst).max(axis=1) / np.abs(dst).max(axis=1)).max())
        print(f"pair_transforms: relative error {err:.2e}")
        assert err < 1e-5


def test_exact_scene_fp32_mirror_gives_the_float64_verdict(ring):
    views, state = ring
    n_measured = n_near = n_kept = n_rejected = 0
    for r, (count, zsum) in enumerate(state):
        pairs = [rule_f64(views, r, s) for s in range(len(views)) if s != r]
        count64 = sum(p[0].astype(np.int32) for p in pairs)
        near = np.any([p[1] for p in pairs], axis=0)
        measured = views[r].depth > 0
        clear = measured & ~near
        assert np.array_equal(count[clear], count64[clear]), (r, int((count[clear] != count64[clear]).sum()))
        assert not count[~measured].any() and not zsum[~measured].any()
        n_measured, n_near = n_measured + int(measured.sum()), n_near + int((measured & near).sum())
        n_kept, n_rejected = n_kept + int((count64[clear] >= 2).sum()), n_rejected + int((count64[clear] < 2).sum())
    print(f"exact scene: {n_measured} measured pixels, {n_near} within the margin, {n_kept} kept and {n_rejected} rejected by float64")
    # conditions on the scene, from the float64 restatement alone: few pixels near a threshold, both verdicts occur
    assert n_measured > 4000 and n_near <= 0.01 * n_measured
    assert n_kept > 0.5 * n_measured and n_rejected > 20
    # filter_views hands out exactly this verdict
    stats = {}
    out = fusion.filter_views(views, 2, backend="host", stats=stats)
    for r, (v, (count, zsum)) in enumerate(zip(out, state)):
        keep = (views[r].depth > 0) & (count >= 2)
        assert v.P is views[r].P and v.image is views[r].image and v.dscale == views[r].dscale and v.depth.dtype == np.float32
        assert np.array_equal(v.depth, np.where(keep, views[r].depth, np.float32(0)))
        assert stats["measured"][r] == int((views[r].depth > 0).sum()) and stats["kept"][r] == int(keep.sum())
        assert np.array_equal(stats["count_hist"][r], np.bincount(count[views[r].depth > 0], minlength=6))
    # an explicit source list in another order: the same counts (zsum is an fp32 sum in source order)
    count, zsum = fusion.consistency_host(views, 0, [5, 3, 1, 4, 2])
    assert np.array_equal(count, state[0][0]) and np.allclose(zsum, state[0][1], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        fusion.filter_views(views, 2, backend="host", sources=[[0]] + [[0]] * 5)              # a view lists itself


def test_a_corrupted_block_is_rejected_and_costs_the_others_one_vote(ring):
    views, state = ring
    clean = fusion.filter_views(views, 2, backend="host")
    bad = 2
    depth = views[bad].depth.copy()
    block = (slice(17, 23), slice(25, 31))
    assert (depth[block] > 0).all() and (clean[bad].depth[block] > 0).all()          # measured, and kept when it is right
    depth[block] *= np.float32(1.05)
    corrupted = list(views)
    corrupted[bad] = views[bad]._replace(depth=depth)
    out = fusion.filter_views(corrupted, 2, backend="host")
    assert not out[bad].depth[block].any()
    rest = np.ones(depth.shape, bool)
    rest[block] = False
    assert np.array_equal(out[bad].depth[rest], clean[bad].depth[rest])
    lost = 0
    for r in range(len(views)):
        if r != bad:
            count, _ = fusion.consistency_host(corrupted, r, [s for s in range(len(views)) if s != r])
            drop = state[r][0] - count
            assert drop.max() <= 1, (r, int(drop.max()))
            lost += int((drop == 1).sum())
    assert lost > 10                                                     # the block was a source of its neighbours


HOLES = (0.0, -1.5, np.nan, np.inf)


def test_holes_in_the_reference_and_in_a_source(ring):
    views, state = ring
    # in the reference
    r = 1
    depth = views[r].depth.copy()
    spots = [(18, 20), (20, 30), (15, 27), (22, 24)]
    assert all(state[r][0][p] >= 2 for p in spots)
    for p, h in zip(spots, HOLES):
        depth[p] = h
    holed = list(views)
    holed[r] = views[r]._replace(depth=depth)
    others = [s for s in range(len(views)) if s != r]
    count, zsum = fusion.consistency_host(holed, r, others)
    out = fusion.filter_views(holed, 1, backend="host")[r].depth
    for p in spots:
        assert count[p] == 0 and zsum[p] == 0 and out[p] == 0
    assert np.isfinite(out).all()
    untouched = np.ones(depth.shape, bool)
    for p in spots:
        untouched[p] = False
    assert np.array_equal(count[untouched], state[r][0][untouched])
    # in a source: the pairs whose four taps touch the hole skip that source, every other pair is as it was
    r, s = 0, 1
    single = {k: fusion.consistency_host(views, r, [k])[0] for k in range(1, len(views))}
    assert np.array_equal(sum(single.values()), state[r][0])
    _, near, sx, sy = rule_f64(views, r, s)
    for h in HOLES:
        hy, hx = 19, 22
        depth = views[s].depth.copy()
        depth[hy, hx] = h
        holed = list(views)
        holed[s] = views[s]._replace(depth=depth)
        with np.errstate(invalid="ignore"):
            touches = (np.floor(sx) >= hx - 1) & (np.floor(sx) <= hx) & (np.floor(sy) >= hy - 1) & (np.floor(sy) <= hy)
        touches &= views[r].depth > 0
        assert touches.sum() >= 3 and single[s][touches & ~near].sum() >= 3, "the hole lies where the pair agreed"
        one = fusion.consistency_host(holed, r, [s])[0]
        clear = ~near
        assert not one[touches & clear].any()
        assert np.array_equal(one[~touches & clear], single[s][~touches & clear])
        count = fusion.consistency_host(holed, r, list(range(1, len(views))))[0]
        assert np.array_equal(count, one + sum(single[k] for k in single if k != s))


def test_average_is_the_mean_over_the_agreeing_views(ring):
    views, state = ring
    scaled = [v._replace(depth=(v.depth / np.float32(2.5)).astype(np.float32), dscale=2.5) if i % 2 else v for i, v in enumerate(views)]
    out = fusion.filter_views(scaled, 2, average=True, backend="host")
    plain = fusion.filter_views(scaled, 2, backend="host")
    f32 = np.float32
    for r, v in enumerate(scaled):
        count, zsum = fusion.consistency_host(scaled, r, [s for s in range(len(views)) if s != r])
        keep = (v.depth > 0) & (count >= 2)
        assert keep.sum() > 400 and np.array_equal(keep, plain[r].depth > 0)
        d = v.depth * f32(v.dscale)
        want = ((zsum + d) / (count + 1).astype(f32)) / f32(v.dscale)
        assert out[r].depth.dtype == np.float32 and np.array_equal(out[r].depth[keep], want[keep]) and not out[r].depth[~keep].any()
        # every agreeing w.z lies within rel_thresh of d, and so does their mean with d
        dev = float(np.abs(out[r].depth[keep].astype(np.float64) / v.depth[keep] - 1).max())
        assert dev < 0.01, dev
        assert (out[r].depth[keep] != v.depth[keep]).any()


def test_min_consistent_zero_and_nearest_sources(ring):
    views, _ = ring
    assert fusion.filter_views(views, 0, backend="host") is views
    assert fusion.filter_views(views, 0) is views                        # nothing to do: no GPU is asked for either
    n = len(views)
    near = fusion.nearest_sources(views, 2)
    assert [sorted(x) for x in near] == [sorted([(i - 1) % n, (i + 1) % n]) for i in range(n)]
    assert fusion.nearest_sources(views, 0) == [[]] * n and all(len(x) == n - 1 for x in fusion.nearest_sources(views, 99))
    assert all(fusion.nearest_sources(views, 5)[i][-1] == (i + 3) % n for i in range(n))        # the opposite camera comes last
    # exact ties: two cameras mirrored in x are equally near the one on the mirror plane, and a duplicate is as near as its twin
    mirrored = [sphere_view(c, 80.0, 8, 8) for c in ((0.0, 0.4, -2.5), (1.5, 0.4, -2.0), (-1.5, 0.4, -2.0), (0.2, 0.4, 2.5))]
    mirrored.insert(1, mirrored[3])                                      # 0: middle, 1: far (a copy of 4), 2 / 3: the mirrored pair
    assert fusion.nearest_sources(mirrored, 2)[0] == [2, 3] and fusion.nearest_sources(mirrored, 4)[0] == [2, 3, 1, 4]
    assert fusion.nearest_sources(mirrored, 1)[4] == [1]


def test_depth_filter_entry_points_are_declared_bound_and_exported():
    from surf_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "surf_hip.h")).read()
    L = _lib.lib()
    for name in ("surf_depth_consistency", "surf_depth_consistency_finish"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).errcheck is not None
    assert _lib.ABI_VERSION == 41 and L.surf_abi_version() == 41
    assert callable(ops.depth_consistency) and callable(ops.depth_consistency_finish) and ops.DEPTH_FILTER_TILE_W in (64, 16, 8)
    sig = _lib.SIGNATURES["surf_depth_consistency"][1]
    c = _lib.ctypes
    assert len(sig) == 15 and sig[3] is c.c_float and sig[9:11] == [c.c_float] * 2 and sig[8] is c.c_int       # thresholds by value
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_depth_consistency(None, 0, 0, 1.0, None, None, None, None, 0, 1.0, 0.01, None, None, 64, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_depth_consistency_finish(None, 1.0, None, None, 0, 0, 0, None, None, None)
