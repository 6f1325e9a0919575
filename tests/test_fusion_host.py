"""CPU: the host (numpy fp32) path of surf_amd.fusion - the update sequence written out in csrc/fuse.hip's header comment - on an
analytic plane scene, view_from_val's projection against the item's own rays, and incremental integration.  The mesh of a host
lattice is built here from oracle/mcubes_oracle.py, cell by cell over the cells whose eight corners were observed (the rule of
surf_mc_classify_observed); tests/test_fusion_gpu.py compares the device path with these."""
import numpy as np
import pytest
import torch

from oracle import mcubes_oracle
from surf_amd import fusion
from surf_amd.fusion import DepthView, FusionVolume


def look_at(centre, f, H, W):
    """(K (3,3), w2c (4,4)) of a pinhole camera at `centre` looking at the origin, principal point at the image centre."""
    c = np.asarray(centre, dtype=np.float64)
    z = -c / np.linalg.norm(c)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = np.stack([x, y, z], axis=1), c
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return K, np.linalg.inv(c2w)


def plane_depth(K, w2c, H, W):
    """z-depth (H, W) fp32 of the plane z = 0 seen from the camera (0 where a ray does not meet it in front of the camera)."""
    c2w = np.linalg.inv(w2c)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    d_cam = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ np.linalg.inv(K).T         # z component 1: the ray parameter is z-depth
    d_w = d_cam @ c2w[:3, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -c2w[2, 3] / d_w[..., 2]
    return np.where(np.isfinite(t) & (t > 0), t, 0.0).astype(np.float32)


def neighbour_delta(depth):
    """Largest depth difference between 8-neighbouring pixels."""
    d = depth.astype(np.float64)
    return max(float(np.abs(d[1:] - d[:-1]).max()), float(np.abs(d[:, 1:] - d[:, :-1]).max()),
               float(np.abs(d[1:, 1:] - d[:-1, :-1]).max()), float(np.abs(d[1:, :-1] - d[:-1, 1:]).max()))


PLANE_H = 1.0 / 32
PLANE_CAMERAS = ((-0.6, 0.2, -2.0), (0.7, -0.3, -1.8), (0.1, 0.8, -2.2))


def plane_scene(colors=False):
    """The lattice 33 x 33 x 17 over [-0.5, 0.5]^2 x [-0.25, 0.25] (h = 1/32), three 48 x 64 pinhole cameras (f = 60) looking at
    the origin, each with the analytic z-depth map of the plane z = 0; trunc = 4 h.  Returns (axes, views, trunc)."""
    axes = [np.linspace(-0.5, 0.5, 33, dtype=np.float32), np.linspace(-0.5, 0.5, 33, dtype=np.float32),
            np.linspace(-0.25, 0.25, 17, dtype=np.float32)]
    views = []
    for i, c in enumerate(PLANE_CAMERAS):
        K, w2c = look_at(c, 60.0, 48, 64)
        image = None
        if colors:
            yy, xx = np.mgrid[:48, :64]
            image = np.stack([0.5 + 0.4 * np.sin(0.3 * xx + i), 0.5 + 0.4 * np.cos(0.2 * yy - i), 0.1 + 0.8 * xx / 63.0],
                             axis=-1).astype(np.float32)
        views.append(DepthView((K @ w2c[:3, :4]).astype(np.float32), plane_depth(K, w2c, 48, 64), 1.0, image))
    return axes, views, 4 * PLANE_H


def lattice_of(tsdf, weight):
    """surf_fuse_lattice on the host: u = -tsdf where weight > 0, NaN elsewhere."""
    return np.where(weight > 0, -tsdf, np.float32(np.nan)).astype(np.float32)


def observed_triangles(u, isovalue=0.0):
    """The triangle set of the observed-corner rule from the oracle: the union, over the cells whose eight corners are finite, of
    mcubes_oracle.marching_cubes on the cell's 2 x 2 x 2 block, offset by the cell.  Returns a sorted (F, 9) float64 array: per
    triangle its three vertex coordinates in table order (lattice-index units)."""
    u = np.asarray(u, dtype=np.float32)
    fin = np.isfinite(u)
    inside = u <= isovalue
    nx, ny, nz = u.shape
    allfin = np.ones((nx - 1, ny - 1, nz - 1), bool)
    n_in = np.zeros((nx - 1, ny - 1, nz - 1), int)
    for dx, dy, dz in mcubes_oracle.CORNERS:
        allfin &= fin[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
        n_in += inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    rows = []
    for x, y, z in np.argwhere(allfin & (n_in > 0) & (n_in < 8)):                    # the other cells have no triangles
        v, t = mcubes_oracle.marching_cubes(u[x:x + 2, y:y + 2, z:z + 2], isovalue)
        rows.append((v + np.array([x, y, z], dtype=np.float64))[t].reshape(-1, 9))
    return sort_rows(np.concatenate(rows) if rows else np.zeros((0, 9)))


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def index_to_world(tri9, axes):
    """(F, 9) lattice-index coordinates -> world, for uniform axes."""
    out = tri9.reshape(-1, 3).copy()
    for a in range(3):
        ax = axes[a].astype(np.float64)
        out[:, a] = ax[0] + out[:, a] * (ax[-1] - ax[0]) / (len(ax) - 1)
    return out.reshape(-1, 9)


@pytest.fixture(scope="module")
def plane_host():
    axes, views, trunc = plane_scene()
    vol = FusionVolume(axes, trunc=trunc, backend="host")
    vol.integrate(views)
    u = lattice_of(vol.tsdf, vol.weight)
    return axes, views, trunc, vol, u, observed_triangles(u)


def test_plane_scene_host(plane_host):
    axes, views, trunc, vol, u, tris = plane_host
    h = PLANE_H
    bound = h + max(neighbour_delta(v.depth) for v in views)
    assert trunc == 4 * h and 0.03 < bound < 0.1, bound
    assert float(vol.weight.max()) == 3.0
    share = vol.observed_share()
    world = index_to_world(tris, axes).reshape(-1, 3)
    dist = float(np.abs(world[:, 2]).max())
    print(f"plane scene: observed share {share:.3f}, {len(tris)} triangles, max distance {dist:.4f}, bound {bound:.4f}")
    assert abs(share - 0.74) < 0.01 and len(tris) == 3290          # what a prototype of the rule gave on this scene
    # a vertex lies on an edge of length <= h whose end points have opposite fused signs; a lattice point's sign can be wrong only
    # within delta (the depth step between neighbouring pixels) of the surface; the distance to the plane is 1-Lipschitz
    assert dist <= bound, (dist, bound)
    assert world[:, 0].min() <= -0.5 + h and world[:, 0].max() >= 0.5 - h


def test_unmasked_corners_close_the_observed_region_with_a_sheet():
    """Why the observed-corner rule exists.  A NaN reads as "outside" (u <= isovalue is false), and so does a point behind the
    surface (u = -tsdf > 0): past the truncation nothing spurious appears.  Observed FREE SPACE is "inside", though, so wherever
    it borders unobserved points - the side of a frustum, a masked pixel - plain marching cubes closes it with a sheet that runs
    from the surface towards the camera (and whose vertices, interpolated towards a NaN, have no position).
    Here: the plane scene's first view with the right half of its depth map dropped."""
    axes, views, trunc = plane_scene()
    depth = views[0].depth.copy()
    depth[:, 32:] = 0.0
    vol = FusionVolume(axes, trunc=trunc, backend="host")
    vol.integrate([views[0]._replace(depth=depth)])
    assert 0.2 < vol.observed_share() < 0.6 and float(vol.weight.max()) == 1.0
    u = lattice_of(vol.tsdf, vol.weight)
    bound = PLANE_H + neighbour_delta(views[0].depth)
    z0 = float(axes[2][0])
    masked = index_to_world(observed_triangles(u), axes).reshape(-1, 3)
    assert len(masked) > 1000 and float(np.abs(masked[:, 2]).max()) <= bound
    v_all, t_all = mcubes_oracle.marching_cubes(u, 0.0)
    used = v_all[t_all.reshape(-1)]
    z_all = np.abs(z0 + used[:, 2] * PLANE_H)
    # the same assertion fails: the sheet's vertices lie on edges that end in a NaN, their interpolated coordinate is a NaN itself
    assert len(t_all) > len(masked) // 3 and not np.all(z_all <= bound) and np.isnan(used).any()


def test_incremental_integration_equals_one_call_host():
    axes, views, trunc = plane_scene(colors=True)
    a = FusionVolume(axes, trunc=trunc, colors=True, backend="host")
    a.integrate(views)
    b = FusionVolume(axes, trunc=trunc, colors=True, backend="host")
    b.integrate(views[:1])
    b.integrate(views[1:])
    assert a.n_views == b.n_views == 3
    for k in ("tsdf", "weight", "color"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert float(a.weight.max()) == 3.0 and float(a.color.max()) > 0.5


def test_default_trunc_and_lattice_from_bounds():
    vol = FusionVolume(([0.0, 0.0, 0.0], [1.0, 0.5, 0.26], 0.125), backend="host")
    assert vol.shape == (9, 5, 4) and vol.trunc == 0.5
    assert np.array_equal(vol.axes[0], np.arange(9, dtype=np.float32) * 0.125) and vol.axes[2][-1] >= 0.26
    with pytest.raises(ValueError):
        FusionVolume(vol.axes, trunc=0.0, backend="host")
    with pytest.raises(ValueError):
        FusionVolume(vol.axes, backend="octree")
    with pytest.raises(ValueError, match="no image"):
        FusionVolume(vol.axes, colors=True, backend="host").integrate([DepthView(np.zeros((3, 4)), np.ones((2, 2)), 1.0)])


def test_extract_mesh_has_no_cpu_fallback():
    axes, views, trunc = plane_scene()
    vol = FusionVolume(axes, trunc=trunc, backend="host")
    vol.integrate(views)
    if torch.cuda.is_available():            # the host backend's mesh step runs there (tests/test_fusion_gpu.py checks the mesh)
        assert len(vol.extract_mesh()[1]) > 2000
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.extract_mesh()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusionVolume(axes, trunc=trunc, backend="device")


def test_bounds_from_scale_mats():
    a = np.diag([2.0, 2.0, 2.0, 1.0])
    a[:3, 3] = [10.0, 0.0, -5.0]
    c, s = np.cos(0.3), np.sin(0.3)
    b = np.eye(4)
    b[:3, :3] = 3.0 * np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    lo, hi = fusion.bounds_from_scale_mats([a, torch.from_numpy(b)])
    assert np.allclose(lo, [-3 * (c + s), -3 * (c + s), -7.0]) and np.allclose(hi, [12.0, 3 * (c + s), 3.0])


def synthetic_val_item(H=40, W=56, level=2):
    """A `val` item as the readers build it (datasets.dtu.ray_block / scene_block) with val_res_level 2 and a scale_mat that is
    a rotation times a scale != 1 plus a translation, and a forward's outputs with a smooth positive depth map."""
    from surf_amd.datasets.dtu import pixel_rays, choose_pixels
    g = np.random.default_rng(5)
    K = np.eye(4, dtype=np.float32)
    K[:3, :3] = [[70.0, 0.0, 27.3], [0.0, 68.0, 19.1], [0.0, 0.0, 1.0]]
    q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, :3], c2w[:3, 3] = q, [0.2, -0.1, -2.5]
    r, _ = np.linalg.qr(g.standard_normal((3, 3)))
    r *= np.sign(np.linalg.det(r))
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 37.5 * r, [120.0, -40.0, 610.0]
    px, py = choose_pixels("val", (H, W), 0, None, level)
    rays_o, rays_d = pixel_rays(px, py, torch.from_numpy(K), torch.from_numpy(c2w))
    Hl, Wl = H // level, W // level
    yy, xx = np.mgrid[:Hl, :Wl]
    depth = (2.0 + 0.3 * np.sin(0.4 * xx) + 0.2 * np.cos(0.3 * yy)).astype(np.float32)
    inputs = {"imgs": torch.zeros(3, 3, H, W), "intrs": torch.from_numpy(np.stack([K] * 3)), "c2ws": torch.from_numpy(np.stack([c2w] * 3)),
              "scale_mat": torch.from_numpy(S), "rays_o": rays_o, "rays_d": rays_d, "hw": torch.tensor([Hl, Wl]).int(),
              "pixels_x": px, "pixels_y": py}
    outputs = {"sdf_depth": depth, "render_depth": depth + np.float32(0.01),
               "color_fine": torch.from_numpy(g.random((Hl * Wl, 3)).astype(np.float32))}
    return inputs, outputs


def test_view_from_val_projects_the_items_own_rays():
    inputs, outputs = synthetic_val_item()
    view = fusion.view_from_val(inputs, outputs)
    Hl, Wl = outputs["sdf_depth"].shape
    assert view.P.dtype == np.float32 and view.P.shape == (3, 4) and abs(view.dscale - 37.5) < 1e-9
    assert view.image.shape == (Hl, Wl, 3) and np.array_equal(view.image.reshape(-1, 3), outputs["color_fine"].numpy())
    # the item's own surface points: rays_o + rays_d (z-depth / cos), cos = the ray's angle to the optical axis; to world by scale_mat
    o, d = inputs["rays_o"].double().numpy(), inputs["rays_d"].double().numpy()
    axis = inputs["c2ws"][0, :3, 2].double().numpy()
    depth = outputs["sdf_depth"].reshape(-1).astype(np.float64)
    S = inputs["scale_mat"].numpy()
    pts_w = (o + d * (depth / (d @ axis))[:, None]) @ S[:3, :3].T + S[:3, 3]
    proj = pts_w @ view.P[:, :3].astype(np.float64).T + view.P[:, 3].astype(np.float64)
    jj, ii = np.meshgrid(np.arange(Wl), np.arange(Hl))
    ex, ey = np.abs(proj[:, 0] / proj[:, 2] - jj.reshape(-1)).max(), np.abs(proj[:, 1] / proj[:, 2] - ii.reshape(-1)).max()
    ez = np.abs(proj[:, 2] / (depth * view.dscale) - 1.0).max()
    print(f"view_from_val: pixel error {ex:.2e} / {ey:.2e} px, relative depth error {ez:.2e}")
    assert ex < 1e-3 and ey < 1e-3 and ez < 1e-5
    # the other depth, an array, and a mask
    assert np.array_equal(fusion.view_from_val(inputs, outputs, depth="render_depth").depth, outputs["render_depth"])
    mask = np.zeros((Hl, Wl), bool)
    mask[2:5] = True
    masked = fusion.view_from_val(inputs, outputs, depth=outputs["sdf_depth"], mask=mask)
    assert np.array_equal(masked.depth[2:5], outputs["sdf_depth"][2:5]) and not masked.depth[:2].any() and not masked.depth[5:].any()
    with pytest.raises(ValueError):
        fusion.view_from_val(inputs, outputs, mask=mask.astype(np.uint8))


def test_fusion_entry_points_are_declared_bound_and_exported():
    import os
    from surf_amd import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "surf_hip.h")).read()
    L = _lib.lib()
    for name in ("surf_fuse_integrate", "surf_fuse_lattice", "surf_fuse_vertex_colors", "surf_mc_classify_observed"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES and hasattr(L, name), name
        assert getattr(L, name).errcheck is not None
    assert _lib.ABI_VERSION == 41 and L.surf_abi_version() == 41
    assert "#define SURF_FUSE_MAX_VIEWS 16" in hdr
    from surf_amd import ops
    assert ops.FUSE_MAX_VIEWS == 16
    sig = _lib.SIGNATURES["surf_fuse_integrate"][1]
    assert len(sig) == 17 and sig[15] is _lib.ctypes.c_float and sig[6:9] == [_lib.ctypes.c_int] * 3      # trunc: a float by value
    assert _lib.SIGNATURES["surf_mc_classify_observed"] == _lib.SIGNATURES["surf_mc_classify"]
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_fuse_integrate(None, None, None, None, None, None, 0, 0, 0, None, None, None, None, None, 0, 1.0, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_fuse_lattice(None, None, 0, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_fuse_vertex_colors(None, 0, None, 0, 0, 0, None, None)
    with pytest.raises(_lib.SurfHipError, match="invalid"):
        L.surf_mc_classify_observed(None, 0, 0, 0, 0.0, None, None)
