"""The synthetic DTU scene of tests/golden/dtu_scene.py plus the two folders only the fine-tuning reader reads
(datasets/dtu_finetune.py:116-121): PseudoMVSScore/dtu_exp/<scene>/filtered_avg_depth/<vid:08d>.pfm and
PseudoMVSDepth/mvsnet<scan:03d>_l3.ply.  The fixture directory of tests/golden/make_golden_finetune.py (which runs the
REFERENCE's reader on it) and of tests/test_dtu_finetune.py / tests/test_finetune_gpu.py.  numpy / PIL only, but for
write_sphere_pseudo_data, which asks surf_amd's reader for the scene's normalisation."""
import os

import numpy as np

from tests.golden.dtu_scene import SEEDS, write_dtu_scene, write_pfm  # noqa: F401  (SEEDS: re-exported for the tests)

FINETUNE_CONF = {"dataset_name": "DTUDatasetFinetune", "scene": "scan24", "ref_view": 2, "n_rays": 96, "val_res_level": 4,
                 "factor": 1.0, "interval_scale": 1, "num_interval": 192, "img_hw": [48, 64]}
# (total_steps, warmup, alpha) and the steps at which the reference scheduler's multiplier is recorded
SCHEDULES = {"plain": (5000, 0, 0.02), "warm": (100, 10, 0.1)}
SCHEDULE_STEPS = {"plain": [0, 1, 2, 10, 100, 1000, 1250, 2500, 3750, 4000, 4998, 4999],
                  "warm": [0, 1, 2, 5, 9, 10, 11, 25, 50, 75, 98, 99]}


def add_finetune_folders(root, scene="scan24", n_views=5, hw=(60, 80), seed=7, n_points=3000, depth=(500.0, 100.0), spread=50.0):
    """The fine-tuning reader's pseudo depths (one PFM per view) and pseudo point cloud under an existing DTU-format tree."""
    g = np.random.default_rng(seed)
    H, W = hw
    ddir = os.path.join(root, "PseudoMVSScore", "dtu_exp", scene, "filtered_avg_depth")
    os.makedirs(ddir)
    os.makedirs(os.path.join(root, "PseudoMVSDepth"))
    for v in range(n_views):
        write_pfm(os.path.join(ddir, f"{v:08d}.pfm"), (depth[0] + depth[1] * g.random((H, W))).astype(np.float32))
    with open(os.path.join(root, "PseudoMVSDepth", "mvsnet{:0>3}_l3.ply".format(int(scene[4:]))), "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {n_points}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for p in g.standard_normal((n_points, 3)) * spread:
            f.write(" ".join(f"{v:.5f}" for v in p) + "\n")


def write_finetune_scene(root, seed=5, n_views=5, hw=(60, 80)):
    """write_dtu_scene + add_finetune_folders: returns (K, w2c list)."""
    out = write_dtu_scene(root, seed=seed, n_views=n_views, hw=hw)
    add_finetune_folders(root, n_views=n_views, hw=hw)
    return out


def write_sphere_pseudo_data(dataset_conf, radius=0.5, n_points=2500):
    """Overwrites the pseudo depths and points of the scene `dataset_conf` (a finetune_dataset block) names, in place, by pseudo
    supervision that agrees with a closed surface: the sphere of `radius` about the origin of the normalised frame (the
    SDF network's geometric initialisation is such a sphere, sdf_network.py:62-86).  The point cloud lies on it (written in world
    coordinates through the reader's own scale_mat), and every view's pseudo depth is the distance along the pixel's unit ray to
    it, 0 = "no depth" off its silhouette (the loss masks target > 0).  Random depths and points, which add_finetune_folders
    writes, ask the surface to pass through 2048 scattered points a step instead."""
    import torch
    from surf_amd import conf
    from surf_amd.datasets import get_loader, mvs_io
    from surf_amd.datasets.dtu import pixel_rays
    ds = get_loader(conf.from_dict(dataset_conf), "finetune", False)                 # reads the placeholder files
    S = ds.scale_mat.double().numpy()                                                 # normalised frame -> world
    u = np.random.default_rng(3).standard_normal((n_points, 3))
    pts = (radius * u / np.linalg.norm(u, axis=1, keepdims=True)) @ S[:3, :3].T + S[:3, 3]
    with open(ds.files.pseudo_points(ds.scene), "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {n_points}\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for q in pts:
            f.write(" ".join(f"{v:.5f}" for v in q) + "\n")
    H, W = ds.img_hw
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    for j, vid in enumerate(ds.all_views):
        o, d = pixel_rays(gx.reshape(-1), gy.reshape(-1), ds.intrs[j], ds.c2ws[j])
        o, d = o.double(), d.double()
        b, c = (o * d).sum(1), (o * o).sum(1) - radius * radius
        disc = b * b - c
        t = torch.where(disc > 0, -b - disc.clamp(min=0).sqrt(), torch.zeros_like(b))
        mvs_io.write_pfm(ds.files.pseudo_depth(ds.scene, vid), (t / ds.scale_factor).reshape(H, W).float().numpy())
