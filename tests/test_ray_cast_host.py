"""CPU: the host (numpy fp32) path of FusionVolume.ray_cast - the rule written out in csrc/ray_cast.hip's header comment - against an
independent float64 restatement (the same trilinear field over the observed cells, the root bracketed by dense sampling along the
ray and bisected), against the exact ray-sphere answer on an analytic sphere, on the rule's edge cases at the smallest lattices that
can break them, and dense against brick-sparse state on a fused scene (equal arrays).  tests/test_ray_cast_gpu.py compares the
device path with these, on the same lattices."""
import numpy as np
import pytest

from surf_amd import fusion
from surf_amd.fusion import DepthView, FusionVolume
from tests.test_fusion_gpu import camera, ragged_axes
from tests.test_fusion_sparse_host import dense_host, lattice_bricks, sphere_scene, uniform_axes

# |host - restatement| in lattice steps.  Both evaluate the same interpolant along the same (fp32-rounded) ray; the host path rounds
# the point c + z r (index units up to ~100: ulp 7.6e-6) a few times per evaluation and the field values (|f| <= 2: ulp 2.4e-7 against
# a slope of >= 1 / 4 per step), and a ray meets the surfaces of these tests at cos >= 0.55: about 2e-5 steps; 5 x that.  The
# restatement's own bisection ends far below (50 halvings of 1 / 32 step).
ULP_STEPS = 1e-4


# ---- the float64 restatement ----------------------------------------------------------------------------------------------

def restate(tsdf, weight, color, lift, hw, z_min=0.0, level=0.0, samples_per_step=32):
    """(depth, normal, color) float64 of the first + to - crossing of the trilinear interpolant of tsdf - level over the cells whose
    eight corners have weight > 0, ray by ray: sampled every 1 / samples_per_step lattice steps between the box's entry and exit,
    the first pair of consecutive samples (> 0, <= 0), both in counted cells, bisected.  lift: the fp32 camera, read as float64."""
    tsdf, weight = np.asarray(tsdf, np.float64), np.asarray(weight, np.float64)
    shape = np.array(tsdf.shape)
    L = np.asarray(lift, np.float64)
    H, W = hw
    depth, normal = np.zeros((H, W)), np.zeros((H, W, 3))
    col = None if color is None else np.zeros((H, W, 3))
    if shape.min() < 2:
        return depth, normal, col
    c = L[9:]

    def field(p):
        """(values, counted, cell, local coordinates) at points p (n, 3)"""
        cell = np.clip(np.floor(p), 0, shape - 2).astype(np.int64)
        u = p - cell
        val, counted = np.zeros(len(p)), np.ones(len(p), bool)
        for k in range(8):
            d = np.array([k >> 2, (k >> 1) & 1, k & 1])
            at = tuple((cell + d).T)
            wk = np.prod(np.where(d == 1, u, 1.0 - u), axis=1)
            val += wk * (tsdf[at] - level)
            counted &= weight[at] > 0
        return val, counted, cell, u

    for y in range(H):
        for x in range(W):
            r = L[:9].reshape(3, 3) @ np.array([x, y, 1.0])
            z0, z1 = float(z_min), np.inf
            miss = False
            for a in range(3):
                if r[a] != 0:
                    t0, t1 = (0.0 - c[a]) / r[a], (shape[a] - 1.0 - c[a]) / r[a]
                    z0, z1 = max(z0, min(t0, t1)), min(z1, max(t0, t1))
                elif not 0 <= c[a] <= shape[a] - 1:
                    miss = True
            if miss or not z0 < z1 or not np.isfinite(z1):
                continue
            n = int(np.ceil((z1 - z0) * np.abs(r).max() * samples_per_step)) + 1
            zs = np.linspace(z0, z1, n + 1)
            val, counted, _, _ = field(c + zs[:, None] * r)
            cross = np.flatnonzero(counted[:-1] & counted[1:] & (val[:-1] > 0) & (val[1:] <= 0))
            if len(cross) == 0:
                continue
            a, b = zs[cross[0]], zs[cross[0] + 1]
            for _ in range(50):
                mid = 0.5 * (a + b)
                if field((c + mid * r)[None])[0][0] > 0:
                    a = mid
                else:
                    b = mid
            z = 0.5 * (a + b)
            # the cell of the root, from a point pushed a hair to the FRONT of it (the positive side: the cell that holds the crossing
            # when the root sits on a face)
            _, _, cell, _ = field((c + a * r)[None])
            cell = cell[0]
            u = (c + z * r) - cell
            g, cc = np.zeros(3), np.zeros(3)
            for k in range(8):
                d = np.array([k >> 2, (k >> 1) & 1, k & 1])
                wts = np.where(d == 1, u, 1.0 - u)
                at = tuple(cell + d)
                for ax in range(3):
                    others = np.prod(np.delete(wts, ax))
                    g[ax] += (1.0 if d[ax] else -1.0) * others * tsdf[at]
                if color is not None:
                    cc += np.prod(wts) * np.asarray(color[at], np.float64)
            depth[y, x] = z
            normal[y, x] = g / np.linalg.norm(g) if np.linalg.norm(g) > 0 else 0.0
            if color is not None:
                col[y, x] = cc
    return depth, normal, col


def host_cast(tsdf, weight, color, lift, hw, z_min=0.0, level=0.0):
    return fusion.ray_cast_host(tsdf, weight, color, tsdf.shape, lift, hw, z_min, level)


def assert_matches_restatement(tsdf, weight, color, lift, hw, z_min=0.0, level=0.0):
    """Host path against the restatement: the same pixels hit, depths within ULP_STEPS lattice steps along the ray (|r| steps per
    unit of z), normals and colours to the matching accuracy.  Returns the host arrays."""
    d, n, c = host_cast(tsdf, weight, color, lift, hw, z_min, level)
    rd, rn, rc = restate(tsdf, weight, color, lift, hw, z_min, level)
    assert d.dtype == np.float32 and d.shape == tuple(hw) and n.shape == tuple(hw) + (3,)
    assert np.array_equal(d > 0, rd > 0), (np.argwhere((d > 0) != (rd > 0))[:5], d, rd)
    hit = rd > 0
    assert (d[~hit] == 0).all() and (n[~hit] == 0).all()
    if hit.any():
        L = np.asarray(lift, np.float64)
        yy, xx = np.nonzero(hit)
        speed = np.linalg.norm(np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ L[:9].reshape(3, 3).T, axis=-1)    # steps per unit z
        err = np.abs(d[hit] - rd[hit]) * speed
        print(f"  {int(hit.sum())} hits, |host - restatement| <= {err.max():.2e} steps, "
              f"normals <= {np.abs(n[hit] - rn[hit]).max():.2e}")
        assert err.max() <= ULP_STEPS
        assert np.abs(n[hit] - rn[hit]).max() <= 1e-3           # a gradient of differences of values rounded at 6e-8: far below
        assert np.abs(np.linalg.norm(n[hit], axis=-1) - 1.0).max() <= 1e-6
        if color is not None:
            assert np.abs(c[hit] - rc[hit]).max() <= 1e-4 and (c[~hit] == 0).all()
    return d, n, c


# ---- the analytic sphere ------------------------------------------------------------------------------------------------

SPHERE_SHAPE = (40, 37, 43)                    # the three sizes differ, none is a multiple of 8
SPHERE_H = 0.05
SPHERE_LO = np.array([-1.0, -0.9, -1.1])
SPHERE_CENTRE = SPHERE_LO + SPHERE_H * np.array([19.3, 18.6, 21.4])
SPHERE_R = 10 * SPHERE_H
SPHERE_TRUNC = 4 * SPHERE_H
# a camera outside the lattice, and one INSIDE it (and outside the sphere); the sphere fills most of either image
SPHERE_CAMERAS = {"outside": ((0.9, -0.7, -3.2), 120.0), "inside": ((-0.85, -0.7, -0.9), 48.0)}      # focal length at 64 pixels


def sphere_lattice():
    """(tsdf, weight, color) fp32 of the sphere written straight into the lattice: tsdf = clip((|p - centre| - R) / trunc, -1, 1),
    unobserved (weight 0) deeper than trunc inside, a smooth colour field."""
    axes = [SPHERE_LO[a] + SPHERE_H * np.arange(SPHERE_SHAPE[a]) for a in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    dist = np.sqrt((X - SPHERE_CENTRE[0]) ** 2 + (Y - SPHERE_CENTRE[1]) ** 2 + (Z - SPHERE_CENTRE[2]) ** 2) - SPHERE_R
    tsdf = np.clip(dist / SPHERE_TRUNC, -1.0, 1.0).astype(np.float32)
    weight = (dist >= -SPHERE_TRUNC).astype(np.float32) * 2.0
    color = np.stack([0.5 + 0.4 * np.sin(3 * X), 0.5 + 0.4 * np.cos(2 * Y), 0.5 + 0.3 * np.sin(X + Z)], axis=-1).astype(np.float32)
    return tsdf, weight, color


def sphere_camera(which, hw):
    centre, f = SPHERE_CAMERAS[which]
    H, W = hw
    return camera(centre, SPHERE_CENTRE - np.asarray(centre), f * max(H, W) / 64.0, H, W)


def sphere_volume(backend="host", device=None):
    """A dense FusionVolume over the sphere lattice with the analytic state written into it."""
    vol = FusionVolume((SPHERE_LO, SPHERE_LO + SPHERE_H * (np.array(SPHERE_SHAPE) - 1), SPHERE_H), trunc=SPHERE_TRUNC, colors=True,
                       backend=backend, device=device)
    assert vol.shape == SPHERE_SHAPE
    return vol


def exact_sphere(P, hw):
    """(z-depth, outward normal, impact parameter) float64 of the pixel rays of P against the sphere; depth 0 where a ray misses."""
    P = np.asarray(P, np.float64)
    M_inv = np.linalg.inv(P[:, :3])
    o = -M_inv @ P[:, 3] - SPHERE_CENTRE
    yy, xx = np.mgrid[:hw[0], :hw[1]].astype(np.float64)
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ M_inv.T
    a, b, cc = (d * d).sum(-1), d @ o, o @ o - SPHERE_R ** 2
    disc = b * b - a * cc
    z = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)
    z = np.where(z > 0, z, 0.0)
    impact = np.sqrt(np.maximum(o @ o - b * b / a, 0.0))
    return z, (o + z[..., None] * d) / SPHERE_R, impact


@pytest.fixture(scope="module")
def sphere():
    """(tsdf, weight, color, {camera: (P, lift, hw, host arrays, restatement arrays)}), computed once."""
    tsdf, weight, color = sphere_lattice()
    hw = (24, 32)
    casts = {}
    for which in SPHERE_CAMERAS:
        P = sphere_camera(which, hw)
        lift = fusion.ray_lift(P, SPHERE_LO, SPHERE_H)
        casts[which] = (P, lift, hw, host_cast(tsdf, weight, color, lift, hw), restate(tsdf, weight, color, lift, hw))
    return tsdf, weight, color, casts


@pytest.mark.parametrize("which", ["outside", "inside"])
def test_analytic_sphere(sphere, which):
    """Depth and normal against the exact ray-sphere answer.  The tolerance is what the float64 restatement of the same trilinear
    field itself shows against the exact answer (the interpolation error of the lattice), with a margin of 10 % plus the fp32
    allowance ULP_STEPS; measured (outside / inside camera): restatement 3.86e-2 / 3.89e-2 lattice steps along the ray, host the same
    to 2.1e-5 / 8.2e-6 steps; normals (largest component error) 4.84e-2 / 4.83e-2 for both (DESIGN.md quotes these)."""
    tsdf, weight, color, casts = sphere
    P, lift, hw, (d, n, c), (rd, rn, rc) = casts[which]
    ez, en, impact = exact_sphere(P, hw)
    if which == "inside":                                   # the camera is inside the lattice box and outside the sphere
        cam = -np.linalg.inv(np.asarray(P, np.float64)[:, :3]) @ np.asarray(P, np.float64)[:, 3]
        idx = (cam - SPHERE_LO) / SPHERE_H
        assert (idx > 0).all() and (idx < np.array(SPHERE_SHAPE) - 1).all() and np.linalg.norm(cam - SPHERE_CENTRE) > SPHERE_R + SPHERE_TRUNC
    # rays well inside the silhouette must hit, rays well outside must miss, in both paths; in between the lattice decides
    inner, outer = impact < SPHERE_R - 2 * SPHERE_H, impact > SPHERE_R + 1 * SPHERE_H
    assert inner.sum() >= 40 and outer.sum() >= 40
    for depth in (d, rd):
        assert (depth[inner] > 0).all() and (depth[outer] == 0).all()
    assert np.array_equal(d > 0, rd > 0)
    speed = np.linalg.norm(np.stack(list(np.mgrid[:hw[0], :hw[1]][::-1]) + [np.ones(hw)], axis=-1) @
                           np.asarray(lift, np.float64)[:9].reshape(3, 3).T, axis=-1)            # lattice steps per unit of z
    ref_err, host_err = (np.abs(rd - ez) * speed)[inner].max(), (np.abs(d - ez) * speed)[inner].max()
    ref_n, host_n = np.abs(rn - en)[inner].max(), np.abs(n - en)[inner].max()
    both = (np.abs(d - rd) * speed)[rd > 0].max()
    print(f"{which}: vs exact, lattice steps along the ray: restatement {ref_err:.3e}, host {host_err:.3e}; host - restatement "
          f"{both:.2e}; normals: restatement {ref_n:.3e}, host {host_n:.3e}; {int(inner.sum())} inner pixels, {int((d > 0).sum())} hits")
    # the restatement itself is a sphere to the lattice's accuracy: a trilinear interpolant of a distance function of curvature 1 / R
    # is off by up to 3 h^2 / (8 R) (the cell's diagonal), seen along a ray at cos >= 0.6 here; its gradient, piecewise differences
    # over one cell, by up to sqrt(2) h / (2 R)
    assert ref_err < 3.0 / (8 * 10) / 0.6 and ref_n < np.sqrt(2) / 20 + 0.01
    assert host_err <= 1.1 * ref_err + ULP_STEPS
    assert host_n <= 1.1 * ref_n + 1e-4
    assert both <= ULP_STEPS
    hit = rd > 0
    assert np.abs(c[hit] - rc[hit]).max() <= 1e-4 and (c[~hit] == 0).all() and (n[~hit] == 0).all()
    assert (np.einsum("ijk,ijk->ij", n, en)[inner] > 0.99).all()                 # outward: into free space


def test_volume_method_equals_the_function(sphere):
    """FusionVolume.ray_cast (host backend) on state written into the volume: ray_cast_host's arrays, the voxel size, numpy arrays
    or (return_tensors) tensors; normals=False and a volume without colours drop those arrays."""
    import torch
    tsdf, weight, color, casts = sphere
    P, lift, hw, (d, n, c), _ = casts["outside"]
    vol = sphere_volume()
    vol.tsdf[...], vol.weight[...], vol.color[...] = tsdf, weight, color
    out = vol.ray_cast(P, hw)
    assert np.array_equal(out["depth"], d) and np.array_equal(out["normal"], n) and np.array_equal(out["color"], c)
    assert out["voxel"] == SPHERE_H and (d > 0).sum() > 100
    t = vol.ray_cast(P, hw, normals=False, return_tensors=True)
    assert torch.is_tensor(t["depth"]) and t["normal"] is None and np.array_equal(t["depth"].numpy(), d)
    # the same lattice given as coordinate arrays: uniform to fp32 rounding, the same lift up to the rounding of lo and voxel
    arrays = FusionVolume(uniform_axes(SPHERE_LO, SPHERE_H, SPHERE_SHAPE), trunc=SPHERE_TRUNC, backend="host")
    arrays.tsdf[...], arrays.weight[...] = tsdf, weight
    lo, voxel = arrays.lattice()
    assert abs(voxel - SPHERE_H) < 1e-8 and np.abs(lo - SPHERE_LO).max() < 1e-7
    a = arrays.ray_cast(P, hw)
    assert a["color"] is None and np.array_equal(a["depth"] > 0, d > 0) and np.abs(a["depth"] - d).max() < 1e-5


# ---- rule cases at the smallest sizes that can break them ------------------------------------------------------------------------

RULE_SHAPE = (6, 5, 7)                         # lo = 0, voxel = 1: world = lattice-index units


def plane_field(z0=3.4):
    """tsdf = clip((z0 - k) / 2, -1, 1): free space at small k, the surface at k = z0, seen by a camera looking along +z."""
    k = np.arange(RULE_SHAPE[2], dtype=np.float64)
    tsdf = np.broadcast_to(np.clip((z0 - k) / 2.0, -1.0, 1.0), RULE_SHAPE).astype(np.float32).copy()
    return tsdf, np.ones(RULE_SHAPE, np.float32)


def rule_lift(centre, forward=(0, 0, 1), f=16.0, hw=(5, 5)):
    return fusion.ray_lift(camera(centre, forward, f, hw[0], hw[1]), np.zeros(3), 1.0)


def rays_of(lift, hw):
    """fp32 ray directions (H, W, 3) as the rule forms them."""
    L = np.asarray(lift, np.float32)
    yy, xx = (v.astype(np.float32) for v in np.mgrid[:hw[0], :hw[1]])
    return np.stack([(L[3 * a] * xx + L[3 * a + 1] * yy) + L[3 * a + 2] for a in range(3)], axis=-1)


def test_plane_from_the_front():
    tsdf, weight = plane_field()
    d, n, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, -5.0)), (5, 5))
    assert (d > 0).all() and np.abs(d - 8.4).max() < 1e-5 and np.abs(n - np.array([0, 0, -1.0])).max() < 1e-6


def test_one_unobserved_corner_hides_the_surface():
    tsdf, weight = plane_field()
    weight[2, 2, 3] = 0.0                                   # a corner of the cells i, j in {1, 2}, k in {2, 3}
    lift = rule_lift((2.3, 2.1, -5.0))
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (5, 5))
    # where the ray meets k = 3.4: inside those cells the surface is hidden, and nothing behind it is a hit
    p = np.asarray(lift[9:], np.float64) + 8.4 * rays_of(lift, (5, 5)).astype(np.float64)
    hidden = (p[..., 0] > 1.01) & (p[..., 0] < 2.99) & (p[..., 1] > 1.01) & (p[..., 1] < 2.99)
    clear = (p[..., 0] < 0.99) | (p[..., 0] > 3.01) | (p[..., 1] < 0.99) | (p[..., 1] > 3.01)
    assert hidden.sum() >= 4 and clear.sum() >= 4 and (d[hidden] == 0).all() and (d[clear] > 0).all()


def test_a_back_face_is_no_hit():
    tsdf, weight = plane_field()
    d, n, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, 12.0), (0, 0, -1)), (5, 5))
    assert (d == 0).all() and (n == 0).all()


def test_entering_the_negative_band_from_unobserved_space_is_no_hit():
    tsdf, weight = plane_field()
    weight[:, :, 5:] = 0.0                                  # seen from behind: unobserved, then tsdf < 0, then the back face
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, 12.0), (0, 0, -1)), (5, 5))
    assert (d == 0).all()
    # and from the front with the free space unobserved up to inside the band: the first counted cell starts at f <= 0
    tsdf, weight = plane_field()
    weight[:, :, :4] = 0.0
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, -5.0)), (5, 5))
    assert (d == 0).all()


def test_camera_inside_the_lattice_and_a_hit_in_the_first_cell():
    tsdf, weight = plane_field()
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, 0.6)), (5, 5))
    assert (d > 0).all() and np.abs(d - 2.8).max() < 1e-5
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, 3.1)), (5, 5))      # the surface is in the camera's own cell
    assert (d > 0).all() and np.abs(d - 0.3).max() < 1e-5


def test_rays_missing_the_box():
    tsdf, weight = plane_field()
    d, n, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((20.0, 2.0, -5.0)), (5, 5))
    assert (d == 0).all() and (n == 0).all()
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 2.1, -5.0), f=3.0, hw=(9, 11)), (9, 11))   # some miss, some hit
    assert (d == 0).any() and (d > 0).any()
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.3, 9.0, 3.0), (1, 0, 0), hw=(3, 3)), (3, 3))   # r_y == 0 beside the box
    assert (d == 0).all()


def test_rays_with_zero_components_and_on_lattice_edges():
    tsdf, weight = plane_field()
    lift = rule_lift((2.25, 2.5, -5.0))                     # f = 16 and an integer principal point: exact zeros in fp32
    r = rays_of(lift, (5, 5))
    assert (r[2, 2, :2] == 0).all() and ((r[..., 0] == 0) ^ (r[..., 1] == 0)).sum() == 8 and (r[..., 2] != 0).all()
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (5, 5))
    assert (d > 0).all()
    # the central ray ON a lattice edge line (x = 2, y = 2), its neighbours in lattice planes
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((2.0, 2.0, -5.0)), (5, 5))
    assert (d > 0).all() and np.abs(d - 8.4).max() < 1e-5
    # along the upper faces of the box (x = 5, y = 4: the last cells are entered, not a cell past them)
    d, _, _ = assert_matches_restatement(tsdf, weight, None, rule_lift((5.0, 4.0, -5.0), hw=(1, 1)), (1, 1))
    assert d[0, 0] > 0


def test_tied_crossings_through_lattice_edges():
    """r = (1, 1, 1/4) from (0.5, 0.5, 0.3): the x and y planes are crossed at the same parameter every time (ties go to x: a cell is
    entered and left at one point), against a surface x + y = 5.2."""
    i, j = np.arange(RULE_SHAPE[0])[:, None, None], np.arange(RULE_SHAPE[1])[None, :, None]
    tsdf = np.broadcast_to(np.clip((5.2 - i - j) / 3.0, -1.0, 1.0), RULE_SHAPE).astype(np.float32).copy()
    weight = np.ones(RULE_SHAPE, np.float32)
    lift = np.array([0, 0, 1, 0, 0, 1, 0, 0, 0.25, 0.5, 0.5, 0.3], np.float32)
    d, n, _ = assert_matches_restatement(tsdf, weight, None, lift, (1, 1))
    assert abs(d[0, 0] - 2.1) < 1e-5 and np.abs(n[0, 0] - np.array([-1, -1, 0]) / np.sqrt(2)).max() < 1e-6
    # exactly through lattice POINTS: all three planes tie
    lift = np.array([0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0], np.float32)
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (1, 1))
    assert abs(d[0, 0] - 2.6) < 1e-5


def test_one_pixel_zmin_and_isovalues():
    tsdf, weight = plane_field()
    lift = rule_lift((2.3, 2.1, -5.0), hw=(1, 1))
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (1, 1))
    assert d.shape == (1, 1) and abs(d[0, 0] - 8.4) < 1e-5
    lift = rule_lift((2.3, 2.1, -5.0))
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (5, 5), z_min=8.0)        # in front of the surface: still hit
    assert (d > 0).all()
    d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (5, 5), z_min=9.0)        # beyond it
    assert (d == 0).all()
    for isovalue, z in ((0.5, 9.4), (-0.5, 7.4)):                                             # u = -tsdf = isovalue
        d, _, _ = assert_matches_restatement(tsdf, weight, None, lift, (5, 5), level=-isovalue)
        assert (d > 0).all() and np.abs(d - z).max() < 1e-5
    vol = FusionVolume((np.zeros(3), np.array(RULE_SHAPE) - 1.0, 1.0), trunc=2.0, backend="host")
    vol.tsdf[...], vol.weight[...] = tsdf, weight
    P = camera((2.3, 2.1, -5.0), (0, 0, 1), 16.0, 5, 5)
    for isovalue, z in ((0.5, 9.4), (-0.5, 7.4), (0.0, 8.4)):
        assert np.abs(vol.ray_cast(P, (5, 5), isovalue=isovalue)["depth"] - z).max() < 1e-5
    assert (vol.ray_cast(P, (5, 5), z_min=9.0)["depth"] == 0).all()


# ---- dense versus brick-sparse on a fused scene --------------------------------------------------------------------------

FUSED_CAMERAS = {"view0": None, "inside": ((0.05, -0.33, -0.39), (0.0, 0.3, 0.4), 30.0, (40, 56))}


@pytest.fixture(scope="module")
def fused():
    """(dense host volume, sparse host volume, views) of the sphere scene of the brick-sparse fusion tests, fused once."""
    axes, views, trunc = sphere_scene()
    dense = dense_host(axes, views, trunc)
    sparse = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
    sparse.integrate(views)
    return dense, sparse, views


def fused_camera(which, views):
    if FUSED_CAMERAS[which] is None:
        return views[0].P, tuple(views[0].depth.shape)
    centre, forward, f, hw = FUSED_CAMERAS[which]
    return camera(centre, forward, f, hw[0], hw[1]), hw


@pytest.mark.parametrize("which", ["view0", "inside"])
def test_dense_and_brick_sparse_return_equal_arrays(fused, which):
    dense, sparse, views = fused
    n_box = lattice_bricks(dense.shape)
    print(f"{sparse.n_bricks} of {n_box} bricks allocated")
    assert 27 <= sparse.n_bricks < n_box                    # some brick inside the lattice box is not allocated: rays cross it
    P, hw = fused_camera(which, views)
    a, b = dense.ray_cast(P, hw), sparse.ray_cast(P, hw)
    for k in ("depth", "normal", "color"):
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
    hits = int((a["depth"] > 0).sum())
    print(f"{which}: {hits} of {hw[0] * hw[1]} rays hit")
    assert hits >= 150 and (a["depth"] == 0).sum() >= 150
    for iso in (0.5, -0.5):
        a, b = dense.ray_cast(P, hw, isovalue=iso), sparse.ray_cast(P, hw, isovalue=iso)
        assert all(np.array_equal(a[k], b[k]) for k in ("depth", "normal", "color")) and (a["depth"] > 0).sum() >= 100


def test_the_model_reproduces_the_view_it_was_fused_from(fused):
    """The ray cast of an input view's camera is that view's depth map again, to a fraction of a lattice step (view_residual)."""
    dense, _, views = fused
    res = fusion.view_residual(views[0], dense.ray_cast(views[0].P, views[0].depth.shape))
    print({k: v for k, v in res.items() if k != "residuals"})
    assert res["measured"] == int((views[0].depth > 0).sum()) and res["hit_share"] > 0.9
    # four projective TSDFs are averaged, so the model is not this view's surface exactly: within a lattice step in the median and
    # inside the truncation band (4 steps) at the 90th percentile
    assert res["median_voxels"] < 1.0 and res["p90_voxels"] < 4.0 and abs(res["median"] / res["median_voxels"] - 1.0 / 128) < 1e-9


# ---- errors, view_residual ---------------------------------------------------------------------------------------------

def test_value_errors():
    vol = FusionVolume(ragged_axes(), trunc=0.25, backend="host")
    P = camera((0.0, 0.0, -3.0), (0, 0, 1), 30.0, 11, 17)
    with pytest.raises(ValueError, match="uniform lattice"):
        vol.ray_cast(P, (11, 17))
    sparse = FusionVolume(ragged_axes(), trunc=0.25, backend="host", sparse=True)
    with pytest.raises(ValueError, match="uniform lattice"):
        sparse.ray_cast(P, (11, 17))
    ok = FusionVolume((np.zeros(3), np.ones(3), 0.25), backend="host")
    assert (ok.ray_cast(P, (11, 17))["depth"] == 0).all() and ok.ray_cast(P, (11, 17))["color"] is None       # nothing fused: no hit
    for iso in (-1.0, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="isovalue"):
            ok.ray_cast(P, (11, 17), isovalue=iso)
    for hw in ((0, 4), (4,), (4, 4, 4), (-1, 4), (2.5, 4), None):
        with pytest.raises(ValueError, match="hw"):
            ok.ray_cast(P, hw)
    for bad in (np.zeros((4, 4)), np.zeros((3, 4)), np.full((3, 4), np.nan), np.zeros(5)):
        with pytest.raises(ValueError, match="P"):
            ok.ray_cast(bad, (4, 4))
    with pytest.raises(ValueError, match="z_min"):
        ok.ray_cast(P, (4, 4), z_min=-1.0)
    flat = FusionVolume((np.zeros(3), np.array([1.0, 1.0, 0.0]), 0.25), trunc=1.0, backend="host")         # one layer: no cells
    with pytest.raises(ValueError, match="two lattice points"):
        flat.ray_cast(P, (4, 4))
    sparse_empty = FusionVolume((np.zeros(3), np.ones(3), 0.25), backend="host", sparse=True, colors=True)
    out = sparse_empty.ray_cast(P, (4, 6))
    assert (out["depth"] == 0).all() and out["color"].shape == (4, 6, 3) and out["normal"].shape == (4, 6, 3)


def test_view_residual_on_a_hand_made_pair():
    depth = np.array([[1.0, 2.0, 0.0, 4.0], [np.nan, 2.0, 3.0, -1.0]], np.float32)          # 5 measured (dscale 2: 2, 4, 8, 4, 6)
    model = np.array([[2.5, 0.0, 3.0, 7.0], [1.0, 4.25, 6.0, 1.0]], np.float32)             # hits 4 of them: residuals .5, 1, .25, 0
    view = DepthView(np.eye(3, 4, dtype=np.float32), depth, 2.0)
    res = fusion.view_residual(view, {"depth": model, "normal": None, "color": None, "voxel": 0.5})
    assert res["measured"] == 5 and res["hit"] == 4 and res["hit_share"] == 0.8
    assert sorted(res["residuals"].tolist()) == [0.0, 0.25, 0.5, 1.0]
    assert res["median"] == 0.375 and abs(res["p90"] - 0.85) < 1e-12
    assert res["median_voxels"] == 0.75 and abs(res["p90_voxels"] - 1.7) < 1e-12
    bare = fusion.view_residual(view, model)
    assert bare["median"] == 0.375 and bare["median_voxels"] is None
    none = fusion.view_residual(view, np.zeros_like(model), voxel=0.5)
    assert none["hit"] == 0 and none["hit_share"] == 0.0 and none["median"] is None and none["p90_voxels"] is None
    pooled = fusion.pooled_residual(np.concatenate([res["residuals"], res["residuals"]]), 0.5)
    assert pooled["median"] == 0.375
    with pytest.raises(ValueError, match="size"):
        fusion.view_residual(view, model[:, :2])
