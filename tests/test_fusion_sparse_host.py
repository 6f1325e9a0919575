"""CPU: the brick-sparse FusionVolume (sparse=True) on the host backend - the numpy-fp32 mirror of csrc/fuse_sparse.hip's mark rule
and of the brick-major integration - against the dense host volume: the allocation is a superset of the bricks the mesh can read,
and the state of every allocated point equals the dense state.  Equality, not tolerances.  tests/test_fusion_sparse_gpu.py
compares the device path with these and the sparse mesh with the dense one."""
import numpy as np
import pytest

from surf_amd import fusion
from surf_amd.fusion import DepthView, FusionVolume
from tests.test_fusion_gpu import camera, ragged_axes, ragged_views
from tests.test_fusion_host import PLANE_CAMERAS, look_at, plane_depth

SPHERE_CAMERAS = ((-0.6, 0.2, -2.0), (0.7, -0.3, -1.8), (0.1, 0.8, -2.2), (1.9, 0.1, 0.3))
SPHERE_MEASURED = (240, 276, 188, 276)


def uniform_axes(lo, h, shape):
    return [(lo[a] + h * np.arange(shape[a])).astype(np.float32) for a in range(3)]


def view_image(i, H=48, W=64):
    yy, xx = np.mgrid[:H, :W]
    return np.stack([0.5 + 0.4 * np.sin(0.3 * xx + i), 0.5 + 0.4 * np.cos(0.2 * yy - i), 0.1 + 0.8 * xx / (W - 1.0)], axis=-1).astype(np.float32)


def slab_scene():
    """(axes, views, trunc): 65 x 48 x 150 lattice points (8k + 1, 8k, neither), h = 1/64, the plane z = 0 seen by the three
    plane cameras; trunc = 4 h."""
    h = 1.0 / 64
    axes = uniform_axes((-0.5, -0.36, -1.0), h, (65, 48, 150))
    views = []
    for i, c in enumerate(PLANE_CAMERAS):
        K, w2c = look_at(c, 60.0, 48, 64)
        views.append(DepthView((K @ w2c[:3, :4]).astype(np.float32), plane_depth(K, w2c, 48, 64), 1.0, view_image(i)))
    return axes, views, 4 * h


def sphere_depth(K, w2c, H, W, radius=0.3):
    """z-depth (H, W) fp32 of the nearer intersection of the pixel's ray (direction K^-1 (x, y, 1): z component 1) with the sphere
    |p| = radius, 0 where the ray misses it."""
    c2w = np.linalg.inv(w2c)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    d = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ np.linalg.inv(K).T @ c2w[:3, :3].T
    o = c2w[:3, 3]
    a, b, c = (d * d).sum(-1), d @ o, o @ o - radius * radius
    disc = b * b - a * c
    t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)
    return np.where(t > 0, t, 0.0).astype(np.float32)


def sphere_views():
    views = []
    for i, c in enumerate(SPHERE_CAMERAS):
        K, w2c = look_at(c, 60.0, 48, 64)
        views.append(DepthView((K @ w2c[:3, :4]).astype(np.float32), sphere_depth(K, w2c, 48, 64), 1.0, view_image(i)))
    return views


def sphere_scene():
    """(axes, views, trunc): 97 x 89 x 104 lattice points, h = 1/128, a sphere of radius 0.3 seen by four cameras whose maps are
    mostly "no measurement"; trunc = 4 h."""
    h = 1.0 / 128
    return uniform_axes((-0.375, -0.34, -0.40), h, (97, 89, 104)), sphere_views(), 4 * h


def ragged_scene():
    return ragged_axes(), ragged_views(), 0.25


def seventeen_views():
    """The views of tests/test_fusion_gpu.py::test_seventeen_views_take_two_launches (on the ragged lattice, trunc 0.3)."""
    g = np.random.default_rng(4)
    views = []
    for i in range(17):
        a = 2 * np.pi * i / 17
        c = np.array([2.5 * np.sin(a), 0.4 * np.cos(3 * a), -2.5 * np.cos(a)])
        views.append(DepthView(camera(c, -c, 4.0, 4, 5), (2.5 + 0.4 * g.standard_normal((4, 5))).astype(np.float32), 1.0,
                               (0.05 + 0.9 * g.random((4, 5, 3))).astype(np.float32)))
    return views


SCENES = {"slab": slab_scene, "sphere": sphere_scene, "ragged": ragged_scene}


def dense_host(axes, views, trunc, colors=True):
    vol = FusionVolume(axes, trunc=trunc, colors=colors, backend="host")
    vol.integrate(views)
    return vol


def near_set(axes, views, trunc):
    """(N (bool lattice): the points some view updates with t < 1, per view the size of its share) from the dense host path."""
    N, sizes = np.zeros(tuple(len(a) for a in axes), bool), []
    for v in views:
        one = dense_host(axes, [v], trunc, colors=False)
        n_v = (one.weight > 0) & (one.tsdf < 1)                  # after one view tsdf is that view's t
        sizes.append(int(n_v.sum()))
        N |= n_v
    return N, sizes


def needed_bricks(N):
    """Ascending brick ids (cube table of side ceil(max(shape) / 8)) that hold a point of N dilated by one lattice step."""
    need = np.zeros_like(N)
    nx, ny, nz = N.shape
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                src = N[max(-dx, 0):nx - max(dx, 0), max(-dy, 0):ny - max(dy, 0), max(-dz, 0):nz - max(dz, 0)]
                need[max(dx, 0):nx - max(-dx, 0), max(dy, 0):ny - max(-dy, 0), max(dz, 0):nz - max(-dz, 0)] |= src
    nbp = (max(N.shape) + 7) // 8
    x, y, z = np.nonzero(need)
    return np.unique(((x >> 3) * nbp + (y >> 3)) * nbp + (z >> 3)).astype(np.int32)


def lattice_bricks(shape):
    return int(np.prod([(n + 7) // 8 for n in shape]))


def brick_points(bricks, shape):
    """Per axis the (m, 8) lattice indices of the bricks' points, and the (m, 8, 8, 8) mask of those inside the lattice."""
    nbp = (max(shape) + 7) // 8
    b = np.asarray(bricks, np.int64)
    idx = [o[:, None] * 8 + np.arange(8) for o in (b // (nbp * nbp), (b // nbp) % nbp, b % nbp)]
    ins = [idx[a] < shape[a] for a in range(3)]
    return idx, ins[0][:, :, None, None] & ins[1][:, None, :, None] & ins[2][:, None, None, :]


def assert_equals_dense(sparse, dense):
    """Every lattice point of every allocated brick holds the dense volume's state; the points past the upper faces weight 0."""
    shape = dense.shape
    m = sparse.n_bricks
    idx, valid = brick_points(np.asarray(sparse.bricks), shape)
    ix, iy, iz = (np.minimum(idx[a], shape[a] - 1) for a in range(3))
    pick = (ix[:, :, None, None], iy[:, None, :, None], iz[:, None, None, :])
    for k in ("tsdf", "weight", "color"):
        d = getattr(dense, k)
        if d is None:
            assert getattr(sparse, k) is None
            continue
        s = np.asarray(getattr(sparse, k)).reshape((m, 8, 8, 8) + d.shape[3:])
        assert np.array_equal(s[valid], d[pick][valid]), (k, int((s[valid] != d[pick][valid]).sum()))
    assert not np.asarray(sparse.weight).reshape(m, 8, 8, 8)[~valid].any()
    table = np.asarray(sparse.table)
    assert np.array_equal(np.flatnonzero(table >= 0), np.asarray(sparse.bricks)) and np.array_equal(table[table >= 0], np.arange(m))
    assert abs(sparse.observed_share() - float(((np.asarray(sparse.weight) > 0).sum()) / np.prod(shape))) == 0


@pytest.fixture(scope="module")
def host(request):
    """name -> (axes, views, trunc, dense host volume, N, per-view sizes of N, needed brick ids, sparse host volume), built once."""
    cache = {}

    def get(name):
        if name not in cache:
            axes, views, trunc = SCENES[name]()
            dense = dense_host(axes, views, trunc)
            N, sizes = near_set(axes, views, trunc)
            sparse = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
            sparse.integrate(views)
            cache[name] = (axes, views, trunc, dense, N, sizes, needed_bricks(N), sparse)
        return cache[name]
    return get


@pytest.mark.parametrize("name,share,n_needed,n_table,most", [("slab", 0.457, 108, 1026, 0.15), ("sphere", 0.285, 532, 2028, 0.30)])
def test_conditions_on_the_scenes(host, name, share, n_needed, n_table, most):
    """From the dense host path alone: the scenes are sparse, every view has points within trunc of its surface, and every observed
    point outside N ends with tsdf == 1 exactly - what the superset argument rests on."""
    axes, views, trunc, dense, N, sizes, needed, _ = host(name)
    print(f"{name}: observed share {dense.observed_share():.3f}, N {N.mean():.3f} of the points, needed bricks {len(needed)} of "
          f"{lattice_bricks(dense.shape)}, measured pixels {[int((v.depth > 0).sum()) for v in views]}")
    assert abs(dense.observed_share() - share) < 0.001
    assert lattice_bricks(dense.shape) == n_table and len(needed) == n_needed and len(needed) <= most * n_table
    assert all(s > 0 for s in sizes)
    seen = dense.weight > 0
    assert (N <= seen).all() and (dense.tsdf[seen & ~N] == 1.0).all() and (seen & ~N).sum() > 0
    if name == "sphere":
        assert tuple(int((v.depth > 0).sum()) for v in views) == SPHERE_MEASURED


def test_ragged_scene_conditions(host):
    axes, views, trunc, dense, N, sizes, needed, _ = host("ragged")
    seen = dense.weight > 0
    assert all(s > 0 for s in sizes) and (dense.tsdf[seen & ~N] == 1.0).all()
    assert any(not np.allclose(np.diff(a), np.diff(a)[0]) for a in axes) and views[1].dscale != 1


@pytest.mark.parametrize("name,most", [("slab", 0.25), ("sphere", 0.50), ("ragged", 1.0)])
def test_allocation_is_a_sparse_superset_of_the_needed_bricks(host, name, most):
    axes, views, trunc, dense, N, sizes, needed, sparse = host(name)
    bricks = np.asarray(sparse.bricks)
    print(f"{name}: {len(bricks)} bricks allocated, {len(needed)} needed, allocated share {sparse.allocated_share():.3f}")
    assert bricks.dtype == np.int32 and (np.diff(bricks) > 0).all() and sparse.n_bricks == len(bricks)
    assert np.isin(needed, bricks).all(), np.setdiff1d(needed, bricks)
    assert sparse.allocated_share() == len(bricks) / lattice_bricks(dense.shape) <= most
    assert np.array_equal(bricks, fusion.mark_bricks_host(axes, views, trunc))
    if name == "slab":
        assert len(bricks) == 108                                   # here the pixel rule allocates exactly the needed bricks


@pytest.mark.parametrize("name", ["slab", "sphere", "ragged"])
def test_state_equals_the_dense_state(host, name):
    axes, views, trunc, dense, N, sizes, needed, sparse = host(name)
    assert_equals_dense(sparse, dense)
    assert sparse.n_views == len(views) and float(np.asarray(sparse.weight).max()) == float(dense.weight.max())
    # without colours
    plain = FusionVolume(axes, trunc=trunc, backend="host", sparse=True)
    plain.integrate([v._replace(image=None) for v in views])
    assert plain.color is None and np.array_equal(plain.tsdf, sparse.tsdf) and np.array_equal(plain.weight, sparse.weight)


def test_order_and_batching(host):
    axes, views, trunc, dense, _, _, _, sparse = host("sphere")
    split = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
    split.integrate(views[:1])
    split.integrate(views[1:])
    for k in ("bricks", "table", "tsdf", "weight", "color"):
        assert np.array_equal(getattr(split, k), getattr(sparse, k)), k
    # integrate after finalize(): the state is rebuilt from all views
    late = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
    late.integrate(views[:2])
    assert late.finalize() is late and 0 < late.n_bricks < sparse.n_bricks and late.n_views == 2
    assert_equals_dense(late, dense_host(axes, views[:2], trunc))
    late.integrate(views[2:])
    assert late.n_views == 4
    assert_equals_dense(late, dense)
    assert np.array_equal(late.bricks, sparse.bricks)


def test_seventeen_views_equal_the_dense_host():
    axes, views, trunc = ragged_axes(), seventeen_views(), 0.3
    assert len(views) > fusion.ops.FUSE_MAX_VIEWS
    dense = dense_host(axes, views, trunc)
    assert float(dense.weight.max()) >= 8.0
    sparse = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
    sparse.integrate(views)
    assert np.isin(needed_bricks(near_set(axes, views, trunc)[0]), sparse.bricks).all()
    assert_equals_dense(sparse, dense)


def test_errors_and_the_dense_volume_is_unchanged():
    axes, views, trunc = ragged_scene()
    for bad in ([axes[0][::-1].copy(), axes[1], axes[2]], [axes[0], np.array([0.0, 0.5, 0.5, 1.0], np.float32), axes[2]]):
        with pytest.raises(ValueError, match="increasing"):
            FusionVolume(bad, trunc=trunc, backend="host", sparse=True)
        FusionVolume(bad, trunc=trunc, backend="host")                      # the dense volume takes any spacing, as before
    empty = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=True)
    for iso in (-1.0, 1.0, float("nan"), 2.0):
        with pytest.raises(ValueError, match="isovalue"):
            empty.extract_mesh(iso)
    v, t, c = empty.extract_mesh()
    assert v.shape == (0, 3) and t.shape == (0, 3) and c.shape == (0, 3) and (v.dtype, t.dtype, c.dtype) == (np.float64, np.int64, np.uint8)
    assert empty.n_bricks == 0 and len(empty.bricks) == 0 and empty.allocated_share() == 0.0 and empty.observed_share() == 0.0
    assert (np.asarray(empty.table) == -1).all() and len(empty.table) == ((max(empty.shape) + 7) // 8) ** 3
    with pytest.raises(ValueError, match="no image"):
        empty.integrate([views[0]._replace(image=None)])
    # sparse=False: the class as it was - none of the new attributes, the same arrays
    dense = FusionVolume(axes, trunc=trunc, colors=True, backend="host", sparse=False)
    assert type(dense) is FusionVolume and type(empty) is not FusionVolume and isinstance(empty, FusionVolume)
    for name in ("bricks", "table", "n_bricks", "allocated_share", "finalize", "state_bytes"):
        assert not hasattr(dense, name) and hasattr(empty, name), name
    dense.integrate(views)
    plain = FusionVolume(axes, trunc=trunc, colors=True, backend="host")
    plain.integrate(views)
    ref = {k: np.zeros(dense.shape + ((3,) if k == "color" else ()), np.float32) for k in ("tsdf", "weight", "color")}
    fusion.integrate_host(ref["tsdf"], ref["weight"], ref["color"], axes, views, np.float32(trunc))
    for k in ("tsdf", "weight", "color"):
        assert getattr(dense, k).tobytes() == getattr(plain, k).tobytes() == ref[k].tobytes(), k
    assert dense.shape == (13, 9, 70) and dense.tsdf.shape == dense.shape
