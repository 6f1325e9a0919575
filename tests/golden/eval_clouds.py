"""One point cloud per synthetic scan of tests/golden/eval_scene.py, under <out>/mvsnet{scan:03}_l3.ply (the file name the reference's
evaluator reads in `--mode pcd`), written deterministically: the extra input of tests/golden/make_golden_eval_pcd.py and of the test
that compares surf_amd.evaluation.dtu_eval's point-cloud mode with the numbers the reference printed."""
import os

import numpy as np

from tests.golden.eval_scene import SCANS

PCD_NAME = "mvsnet{scan:03}_l3.ply"
N_POINTS = 5000


def cloud_points(scan):
    """(N_POINTS, 3) fp32: noisy points on the scan's ellipsoid (eval_scene.write_eval_scene's radius, centre and squash), denser than
    the thinning distance in places so that the greedy suppression has work to do, a cap of them missing (a cloud has holes)."""
    k = SCANS.index(scan)
    g = np.random.default_rng(2000 + scan)
    radius, centre, squash = 40.0 + 3.0 * k, np.array([5.0 * k, -3.0 * k, 10.0 + k]), 0.8 + 0.02 * k
    d = g.standard_normal((2 * N_POINTS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[d[:, 0] < 0.9][:N_POINTS]                        # the cap x > 0.9 r is never seen
    assert len(d) == N_POINTS
    return (centre[None] + radius * d * np.array([1.0, squash, 1.0]) + g.normal(0, 0.4, (N_POINTS, 3))).astype(np.float32)


def write_eval_clouds(out_dir):
    from surf_amd import mesh_io
    os.makedirs(out_dir, exist_ok=True)
    for scan in SCANS:
        mesh_io.write_ply_points(os.path.join(out_dir, PCD_NAME.format(scan=scan)), cloud_points(scan))
