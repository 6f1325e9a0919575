"""Scenes for tests/test_points_host.py and tests/test_points_gpu.py, built the way tests/test_depth_filter_host.py builds its own:
ring cameras around an analytic sphere, depth maps rendered from it.  Map sizes are no multiples of 4, 8 or 64."""
import numpy as np

from surf_amd.fusion import DepthView

HOLES = (0.0, -1.5, np.nan, np.inf)


def look_at(centre, f, H, W):
    """(K (3,3), w2c (4,4)) of a pinhole camera at `centre` looking at the origin, principal point at the image centre."""
    c = np.asarray(centre, dtype=np.float64)
    z = -c / np.linalg.norm(c)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = np.stack([x, np.cross(z, x), z], axis=1), c
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    return K, np.linalg.inv(c2w)


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
    """n camera centres on a ring about the y axis, 2.5 from the origin and 37 degrees off the axis."""
    return [(radius * np.sin(2 * np.pi * i / n), height, -radius * np.cos(2 * np.pi * i / n)) for i in range(n)]


def with_images(views, seed):
    """The views with random images; a few values outside [0, 1) so that the quantisation's clamp has work."""
    g = np.random.default_rng(seed)
    return [v._replace(image=(g.random(v.depth.shape + (3,)) * 1.2 - 0.1).astype(np.float32)) for v in views]


def ring_views(n=5, H=37, W=53, f=75.0):
    """n ring cameras that all see the upper half of the sphere (about 31 pixels across): 37 x 53 = 7.66 blocks of 256."""
    return [sphere_view(c, f, H, W) for c in ring_centres(n)]


def mixed_views():
    """Four views of two sizes (37 x 53, 24 x 31), focal lengths 44 to 85, one with dscale 2.5, with images, each with holes of the
    four kinds sprinkled over 5 % of its pixels."""
    g = np.random.default_rng(31)
    spec = (((0.0, 2.0, -1.5), 75.0, 37, 53, 1.0), ((1.2, 1.9, -1.0), 44.0, 24, 31, 1.0), ((-1.0, 2.1, -0.9), 85.0, 37, 53, 2.5),
            ((0.6, 2.2, -1.2), 46.0, 24, 31, 1.0))
    views = []
    for centre, f, H, W, dscale in spec:
        v = sphere_view(centre, f, H, W, dscale=dscale)
        depth = v.depth.copy()
        holes = g.random(depth.shape) < 0.05
        depth[holes] = g.choice(np.array(HOLES, dtype=np.float32), size=int(holes.sum()))
        views.append(v._replace(depth=depth))
    return with_images(views, 32)


def many_views():
    """18 views of 9 x 13: a view has 17 sources, one more than a launch takes."""
    return [sphere_view(c, 17.0, 9, 13) for c in ring_centres(18)]


SCENES = {"ring": ring_views, "ring_colors": lambda: with_images(ring_views(3), 7), "mixed": mixed_views, "many": many_views}
