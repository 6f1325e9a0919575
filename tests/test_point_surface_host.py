"""surf_amd/point_surface.py's numpy mirror (field_bricks_host: rules 1-6 of include/surf_hip.h above surf_cloud_brick_keys) against
an independent float64 restatement without bricks or order (tests/point_surface_scenes.py), against closed forms on a plane and a
sphere, and at the rule's edges.  No GPU: what needs marching cubes is in tests/test_point_surface_gpu.py."""
import functools

import numpy as np
import pytest

from surf_amd import point_surface as PS
from tests import point_surface_scenes as S

EPS = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def sphere_case(where, rv, side=23, min_points=4):
    P, N, lat = S.sphere_scene(where, side)
    R = rv * lat.voxel
    state = PS.field_bricks_host(P, N, None, lat.axes, R, min_points, lattice=(lat.lo, lat.voxel))
    r64 = S.restate(P, N, None, lat, R)
    r32 = S.restate(P, N, None, lat, R, dtype=np.float32)
    both = (r64.count > 0) & (r32.count > 0)
    E = float(np.abs(r32.f - r64.f)[both].max())
    return state, r64, E, float(np.float32(R))


def format_tol(count, R):
    """|mirror f - float64 f| from the number formats alone: w carries about 8 roundings (d2: 5, t: 2, the two squares), g 5 absolute
    ones of size R 2^-24, each of the two m-term sums m more, the division and the division by R two; |g| < R for unit normals.
    (2 m + 24) 2^-24 R covers them with room."""
    return (2.0 * count + 24.0) * EPS * R


def compare(state, r, lat, R, min_points, tol=None, colors=False):
    """The mirror's dense state against a restatement: observed sets equal outside the ambiguous nodes, counts equal, f within tol
    (default format_tol).  Returns the number of ambiguous nodes."""
    tsdf, weight, color, have = S.dense(state, lat.shape)
    clear = ~r.ambiguous
    obs64 = (r.count >= min_points) & (r.sw > 0)
    assert np.array_equal((weight > 0)[clear], obs64[clear])
    on = clear & obs64
    assert np.array_equal(weight[on], r.count[on].astype(np.float32))
    err = np.abs(tsdf[on].astype(np.float64) * R - r.f[on])
    bound = format_tol(r.count[on], R) if tol is None else tol
    assert (err <= bound).all(), (float(err.max()), float(np.min(bound)))
    assert have[r.count > 0].all()                                   # the allocation holds every node with a point in reach
    if colors:
        assert (np.abs(color[on] - r.color[on]) <= format_tol(r.count[on], 1.0)[:, None]).all()
    return int(r.ambiguous.sum())


# ---- 1. the float64 restatement ----

@pytest.mark.parametrize("where", list(S.CENTRES))
@pytest.mark.parametrize("rv", (2.5, 4.0))
def test_mirror_against_float64_restatement(where, rv):
    """1000-point Fibonacci sphere (r = 0.4) on a 23^3 lattice (voxel 0.0709), R = 2.5 and 4 voxels, at the origin and about
    (300, -150, 600).  Observed sets are equal outside the nodes where a float64 d2 lies within fp32 rounding of R2 (at most 1 % of
    the nodes), counts are equal there, and |tsdf R - float64 f| <= 8 E with E = max |fp32 restatement - float64 restatement|.
    Measured: E = 4.5e-8 (R = 2.5 voxels) and 1.6e-7 (R = 4) at the origin, 5.1e-8 and 1.3e-7 in the world frame, world units
    (voxel 0.0709); the mirror's largest error 6.1e-8 / 1.9e-7 / 5.3e-8 / 1.6e-7; no ambiguous node in any of the four."""
    state, r64, E, R = sphere_case(where, rv)
    lat = S.sphere_scene(where)[2]
    ambiguous = compare(state, r64, lat, R, 4, tol=8.0 * E)
    print(f"{where} R = {rv} voxels: E = {E:.3g}, ambiguous nodes {ambiguous} of {r64.count.size}")
    assert E < 1e-6 and ambiguous <= 0.01 * r64.count.size
    assert (r64.count >= 4).sum() > 1000


# ---- 2. the plane ----

@functools.lru_cache(maxsize=None)
def plane_state():
    P, N, lat = S.plane_scene()
    return PS.field_bricks_host(P, N, None, lat.axes, 3.0 * lat.voxel, 4, lattice=(lat.lo, lat.voxel))


def test_plane_is_reproduced_to_rounding():
    """3000 points on z = 0.125 with normals (0, 0, 1), voxel 1 / 32, R = 3 voxels: g = z - 0.125 for every point, so f is that
    number up to the rounding of two m-term sums and one division, |f - (z - 0.125)| <= (2 m + 2) 2^-24 |z - 0.125| at a node with
    m points.  Measured: the largest error is 1.9e-9 (the division by R and the product with it that the test reads f through)."""
    P, N, lat = S.plane_scene()
    R = float(np.float32(3.0 * lat.voxel))
    tsdf, weight, _, _ = S.dense(plane_state(), lat.shape)
    obs = weight > 0
    assert obs.sum() > 5000
    z = np.broadcast_to(lat.axes[2].astype(np.float64)[None, None, :], lat.shape) - 0.125
    err = np.abs(tsdf.astype(np.float64) * R - z)[obs]
    print(f"plane: {int(obs.sum())} observed nodes, max error {err.max():.3g}")
    assert (err <= (2.0 * weight[obs] + 2.0) * EPS * np.abs(z[obs])).all()
    # observed exactly within the support: |z - 0.125| < R, and the lattice planes at distance R are not
    assert (np.abs(z[obs]) < R).all()
    # every zero crossing of a z edge lies on the plane: the nodes of the lattice plane z = 0.125 carry f = 0 exactly
    k = int(np.argmin(np.abs(lat.axes[2] - 0.125)))
    assert lat.axes[2][k] == 0.125 and (tsdf[:, :, k][obs[:, :, k]] == 0).all() and obs[:, :, k].sum() > 900
    assert (tsdf[:, :, k + 1][obs[:, :, k + 1]] > 0).all() and (tsdf[:, :, k - 1][obs[:, :, k - 1]] < 0).all()


# ---- 3. the sphere ----

@pytest.mark.parametrize("rv", (2.5, 4.0))
def test_sphere_one_sided_bound(rv):
    """f is a convex combination of the points' plane distances n_i . (x - p_i), and for exact samples of a sphere of radius r
    d - R^2 / (2 r) < n_i . (x - p_i) <= d with d the node's signed distance: so d - R^2 / (2 r) - 8 E <= f <= d + 8 E at every
    observed node (E: test 1's; it also covers the samples' fp32 rounding, 3e-8).  Then every zero crossing of a lattice edge lies
    within R^2 / (2 r) + voxel of the sphere, a node inside (d < -8 E) is negative and a node with d > R^2 / (2 r) + 8 E positive.
    Measured: worst crossing 0.09 voxel (R = 2.5 voxels, bound 1.55) and 0.23 voxel (R = 4, bound 2.42) off the sphere.  The stricter
    reading sign(f) = sign(d) does NOT hold in the shell 0 < d < R^2 / (2 r), where the sagitta pulls f below 0 (12 and 108 nodes):
    the surface sits that far inside the samples, which is the bound above and no error."""
    state, r64, E, R = sphere_case("origin", rv)
    P, N, lat = S.sphere_scene("origin")
    tsdf, weight, _, _ = S.dense(state, lat.shape)
    f = tsdf.astype(np.float64) * R
    obs = weight > 0
    X = np.stack(np.meshgrid(*[a.astype(np.float64) for a in lat.axes], indexing="ij"), axis=-1)
    d = np.linalg.norm(X, axis=-1) - S.SPHERE_R
    sag = R * R / (2.0 * S.SPHERE_R)
    assert (f[obs] <= d[obs] + 8 * E).all() and (f[obs] >= d[obs] - sag - 8 * E).all()
    assert (f[obs & (d < -8 * E)] < 0).all() and (f[obs & (d > sag + 8 * E)] > 0).all()
    worst, crossings = 0.0, 0
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cut = obs[lo] & obs[hi] & ((f[lo] < 0) != (f[hi] < 0))
        s = f[lo][cut] / (f[lo][cut] - f[hi][cut])
        x = X[lo][cut] + s[:, None] * (X[hi][cut] - X[lo][cut])
        off = np.abs(np.linalg.norm(x, axis=1) - S.SPHERE_R)
        worst, crossings = max(worst, float(off.max())), crossings + int(cut.sum())
    loose = int((obs & ((f > 0) != (d > 0)) & (np.abs(d) > 8 * E)).sum())
    print(f"sphere R = {rv} voxels: {crossings} edge crossings, worst {worst / lat.voxel:.3f} voxel off (bound "
          f"{(sag + lat.voxel) / lat.voxel:.2f}); nodes with sign(f) != sign(d): {loose}")
    assert crossings > 500 and worst <= sag + lat.voxel


# ---- 4. the rule's edges ----

def run(P, N, lat, rv, min_points=4, colors=None, **kw):
    return PS.field_bricks_host(P, N, colors, lat.axes, rv * lat.voxel, min_points, lattice=(lat.lo, lat.voxel), **kw)


def same_state(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x, y))


def test_bad_rows_take_no_part():
    P, N, lat = S.sphere_scene("origin")
    bad_p = np.array([[np.nan, 0, 0], [0.1, np.inf, 0], [0, 0, 0.4], [0, 0.4, 0], [0.4, 0, 0], [0, 0, -0.4]], np.float32)
    bad_n = np.array([[0, 0, 1], [0, 1, 0], [np.nan, 0, 1], [0, -np.inf, 0], [0, 0, 0], [-0.0, 0.0, -0.0]], np.float32)
    at = np.array([0, 300, 300, 700, 1000, 1000])
    P2, N2 = np.insert(P, at, bad_p, axis=0), np.insert(N, at, bad_n, axis=0)
    col = np.random.default_rng(1).integers(0, 256, (len(P2), 3)).astype(np.uint8)
    keep = np.ones(len(P2), bool)
    keep[at + np.arange(6)] = False
    st = {}
    got = run(P2, N2, lat, 2.5, colors=col, stats=st)
    assert st["points"] == 1000
    same_state(got, run(P2[keep], N2[keep], lat, 2.5, colors=col[keep]))
    R = float(np.float32(2.5 * lat.voxel))
    compare(got, S.restate(P2, N2, col, lat, R), lat, R, 4, colors=True)


def test_duplicates_count_twice():
    P, N, lat = S.sphere_scene("origin")
    once, twice = run(P, N, lat, 2.5, 2), run(np.concatenate([P, P]), np.concatenate([N, N]), lat, 2.5, 4)
    assert np.array_equal(once[0], twice[0]) and np.array_equal(twice[3], 2 * once[3])
    R = float(np.float32(2.5 * lat.voxel))
    compare(twice, S.restate(np.concatenate([P, P]), np.concatenate([N, N]), None, lat, R), lat, R, 4)


def test_a_point_at_exactly_R_is_not_admitted():
    """voxel 2^-5 and R = 3 voxels are exact in fp32, and so is R2 = 9 2^-10: a point ON a node is at d2 == R2 from the node three
    steps along an axis, and the rule's test is strict."""
    lat = S.lattice((0, 0, 0), (0.75, 0.75, 0.75), 2.0 ** -5)
    P = np.array([[8, 8, 8]], np.float32) * np.float32(2.0 ** -5)
    N = np.array([[0, 0, 1]], np.float32)
    tsdf, weight, _, have = S.dense(run(P, N, lat, 3.0, 1), lat.shape)
    assert weight[8, 8, 8] == 1 and weight[10, 8, 8] == 1 and weight[8, 8, 10] == 1 and weight[6, 8, 8] == 1
    assert have[11, 8, 8] and weight[11, 8, 8] == 0 and weight[5, 8, 8] == 0 and weight[8, 11, 8] == 0 and weight[8, 8, 5] == 0
    assert int((weight > 0).sum()) == 123 - 30           # the lattice points with d2 <= 9, less the 6 + 24 with d2 == 9 ((2, 2, 1) too)
    assert tsdf[8, 8, 10] == np.float32(2.0 / 3.0) and tsdf[8, 8, 6] == -np.float32(2.0 / 3.0) and tsdf[10, 8, 8] == 0


def test_min_points_threshold():
    P, N, lat = S.sphere_scene("origin")
    R = float(np.float32(2.5 * lat.voxel))
    r = S.restate(P, N, None, lat, R)
    i = tuple(np.argwhere((r.count == 6) & ~r.ambiguous)[0])
    for mp, seen in ((5, True), (6, True), (7, False)):
        state = run(P, N, lat, 2.5, mp)
        _, weight, _, _ = S.dense(state, lat.shape)
        assert (weight[i] == 6) == seen and (seen or weight[i] == 0)
        compare(state, r, lat, R, mp)


def test_points_outside_the_lattice():
    """A point 1.5 steps below the lattice's lower x face is within R = 3 steps of its first two node planes and contributes; a
    point more than `ring` bricks outside takes no part (and is admitted nowhere)."""
    lat = S.lattice((0, 0, 0), (1.0, 1.0, 1.0), 1.0 / 20)
    v = lat.voxel
    P = np.array([[-1.5 * v, 0.5, 0.5], [-9.5 * v, 0.5, 0.5], [0.5, 1.0 + 12 * v, 0.5], [0.3, 0.3, 0.3]], np.float32)
    N = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (4, 1))
    st = {}
    state = run(P, N, lat, 3.0, 1, stats=st)
    assert st["points"] == 2
    _, weight, _, _ = S.dense(state, lat.shape)
    assert weight[0, 10, 10] == 1 and weight[1, 10, 10] == 1 and weight[2, 10, 10] == 0 and weight[6, 6, 6] == 1
    R = float(np.float32(3.0 * v))
    compare(state, S.restate(P, N, None, lat, R), lat, R, 1)
    same_state(state, run(P[[0, 3]], N[[0, 3]], lat, 3.0, 1))


def test_ragged_lattice_has_zero_state_past_its_faces():
    c = np.zeros(3)
    P, N = S.fibonacci_sphere(1000, S.SPHERE_R)
    v = 1.56 / 22
    lat = S.lattice(c - 0.78 + np.array([0.1, 0.0, -0.1]), c - 0.78 + np.array([0.1, 0.0, -0.1]) + v * np.array([20, 22, 25]), v)
    assert lat.shape == (21, 23, 26)
    state = run(P, N, lat, 2.5, 4, colors=np.full((1000, 3), 200, np.uint8))
    bricks, table, tsdf, weight, color = state
    nbp = 4
    B = np.stack([bricks // (nbp * nbp), (bricks // nbp) % nbp, bricks % nbp], axis=1)
    l = np.arange(512)
    idx = [B[:, a, None] * 8 + ((l >> s) & 7)[None, :] for a, s in enumerate((6, 3, 0))]
    past = ((idx[0] >= 21) | (idx[1] >= 23) | (idx[2] >= 26)).reshape(-1)
    assert past.sum() > 0 and not tsdf[past].any() and not weight[past].any() and not color[past].any()
    R = float(np.float32(2.5 * v))
    compare(state, S.restate(P, N, np.full((1000, 3), 200, np.uint8), lat, R), lat, R, 4, colors=True)
    assert np.abs(color[weight > 0].astype(np.float64) - 200.5 / 256).max() < 1e-5          # one colour in, that colour out


def test_radius_of_nine_voxels_reaches_two_bricks():
    P, N, lat = S.sphere_scene("origin", 25)                          # voxel 0.065: R = 9 voxels is 0.585, ring = 2
    R = float(np.float32(9.0 * lat.voxel))
    assert PS._ring(PS.support_reach(lat.axes, lat.voxel, R)) == 2
    compare(run(P, N, lat, 9.0, 4), S.restate(P, N, None, lat, R), lat, R, 4)
    with pytest.raises(ValueError):
        run(P, N, lat, 32.5, 4)                                       # ring 5: past the limit


def test_empty_and_one_point_clouds():
    lat = S.sphere_scene("origin")[2]
    bricks, table, tsdf, weight, color = run(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), lat, 2.5, 1,
                                             colors=np.zeros((0, 3), np.uint8))
    assert bricks.shape == (0,) and tsdf.shape == (0,) and weight.shape == (0,) and color.shape == (0, 3) and (table == -1).all()
    P, N = np.array([[0.01, 0.02, 0.03]], np.float32), np.array([[0.6, 0.0, 0.8]], np.float32)
    R = float(np.float32(2.5 * lat.voxel))
    state = run(P, N, lat, 2.5, 1)
    compare(state, S.restate(P, N, None, lat, R), lat, R, 1)
    assert (state[3] > 0).sum() > 30
    assert not run(P, N, lat, 2.5, 2)[3].any()


def test_field_does_not_depend_on_the_allocation():
    """Forcing the blanket (2 ring + 1)^3 neighbourhood allocates more bricks and changes no node: what it adds is unobserved.
    (The mesh of both allocations is compared in tests/test_point_surface_gpu.py.)"""
    P, N, lat = S.sphere_scene("origin", 45)
    tight, blanket = run(P, N, lat, 2.5, 4), run(P, N, lat, 2.5, 4, alloc_reach=8.0)
    assert set(tight[0]) < set(blanket[0])
    a, b = S.dense(tight, lat.shape), S.dense(blanket, lat.shape)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    extra = b[3] & ~a[3]
    assert extra.any() and not b[1][extra].any()


def test_bad_arguments():
    P, N, lat = S.sphere_scene("origin")
    for radius, mp in ((0.0, 4), (-1.0, 4), (float("nan"), 4), (float("inf"), 4), (0.2, 0), (0.2, 2.5)):
        with pytest.raises(ValueError):
            PS.field_bricks_host(P, N, None, lat.axes, radius, mp)
    with pytest.raises(ValueError):
        PS.field_bricks_host(P, N[:10], None, lat.axes, 0.2)
    with pytest.raises(ValueError):
        PS.field_bricks_host(P, N, np.zeros((1000, 3), np.float32), lat.axes, 0.2)


# ---- 5. the entry points ----

def test_cloud_entry_points_are_declared_bound_and_exported():
    """Header, binding table and library agree on the new entry points under ABI 41; the status codes arrive before any HIP call."""
    from surf_amd import _lib, ops
    L = _lib.lib()
    with open(_lib.HEADER_PATH) as f:
        hdr = f.read()
    assert _lib.ABI_VERSION == 41 and L.surf_abi_version() == 41
    for name in ("surf_cloud_brick_keys", "surf_cloud_mark_bricks", "surf_cloud_field_bricks"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
    assert f"#define SURF_CLOUD_MAX_RING {ops.CLOUD_MAX_RING}" in hdr
    assert L.surf_cloud_brick_keys(None, None, 0, 0.0, 0.0, 0.0, 1.0, 8, 8, 8, 3.0, None, None) == 0          # empty: no launch
    assert L.surf_cloud_mark_bricks(None, 0, 0.0, 0.0, 0.0, 1.0, 8, 8, 8, 3.0, None, None) == 0
    assert L.surf_cloud_field_bricks(None, None, None, None, 0, None, 0, None, None, None, 8, 8, 8, 0.0, 0.0, 0.0, 1.0, 3.0, 3.0, 4,
                                     None, None, None, None, None) == 0
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_cloud_brick_keys(None, None, 5, 0.0, 0.0, 0.0, 1.0, 8, 8, 8, 3.0, None, None)
    one = np.zeros(8, np.float32).ctypes.data
    with pytest.raises(_lib.SurfHipError, match="limit"):
        L.surf_cloud_mark_bricks(one, 1, 0.0, 0.0, 0.0, 1.0, 8, 8, 8, 32.5, one, None)                        # ring 5
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_cloud_mark_bricks(one, 1, 0.0, 0.0, 0.0, 0.0, 8, 8, 8, 3.0, one, None)                         # voxel 0
    for reach in (0.0, -1.0, float("nan"), 32.5):
        with pytest.raises(ValueError):
            ops.cloud_ring(reach)
    assert ops.cloud_ring(3.0) == 1 and ops.cloud_ring(8.0) == 1 and ops.cloud_ring(8.001) == 2 and ops.cloud_ring(32.0) == 4
