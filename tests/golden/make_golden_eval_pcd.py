#!/usr/bin/env python3
"""Golden Chamfer numbers of the REFERENCE's DTU evaluator in its point-cloud mode: its evaluation/dtu_eval.py is run as
the script it is with `--mode pcd` on the synthetic evaluation directory of tests/golden/eval_scene.py plus the clouds of
tests/golden/eval_clouds.py (<out_dir>/mvsnet{scan:03}_l3.ply, the name the script reads); the results.json it writes is committed as
tests/golden/dtu_eval_pcd_results.json.

The stand-ins (open3d's file readers, tqdm, numpy 1's `mgrid` and `from numpy import *`) and the seeded shuffle are those of
tests/golden/make_golden_eval.py, imported from it.  Everything numerical is the reference's code."""
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.golden import eval_clouds, eval_scene  # noqa: E402
from tests.golden.make_golden_eval import REF, _MGridOfNumpy1, _o3d_stub, _tqdm_stub  # noqa: E402


def main():
    o3d, io = _o3d_stub()
    sys.modules["open3d"], sys.modules["open3d.io"] = o3d, io
    sys.modules["tqdm"] = _tqdm_stub()
    real_rng = np.random.default_rng
    with tempfile.TemporaryDirectory() as tmp:
        out_dir, data_dir = os.path.join(tmp, "exp"), os.path.join(tmp, "eval")
        eval_scene.write_eval_scene(out_dir, data_dir)
        eval_clouds.write_eval_clouds(out_dir)
        argv = sys.argv
        sys.argv = ["dtu_eval.py", "--mode", "pcd", "--out_dir", out_dir, "--dataset_dir", data_dir, "--downsample_density",
                    str(eval_scene.ARGS["downsample_density"]), "--patch_size", str(eval_scene.ARGS["patch_size"]), "--max_dist",
                    str(eval_scene.ARGS["max_dist"])]
        np.random.default_rng = lambda *a: real_rng(eval_scene.SHUFFLE_SEED) if not a else real_rng(*a)
        real_mgrid, np.mgrid = np.mgrid, _MGridOfNumpy1()
        real_all = list(np.__all__)
        np.__all__ = [n for n in real_all if n not in ("min", "max", "round")]
        try:
            runpy.run_path(os.path.join(REF, "evaluation", "dtu_eval.py"), run_name="__main__")
        finally:
            np.random.default_rng = real_rng
            np.mgrid = real_mgrid
            np.__all__ = real_all
            sys.argv = argv
        with open(os.path.join(out_dir, "results.json")) as f:
            res = json.load(f)
    with open(os.path.join(HERE, "dtu_eval_pcd_results.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("wrote dtu_eval_pcd_results.json:", {k: round(v["all"], 4) for k, v in res.items()})


if __name__ == "__main__":
    main()
