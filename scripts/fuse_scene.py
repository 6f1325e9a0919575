#!/usr/bin/env python3
"""One scene mesh from MANY reference views, as ONE command:

    python scripts/fuse_scene.py --conf confs/surf.conf --ckpt ckpt.pth --data_dir <DTU> --scan 24 --ref_views 23 43 12 ... \
        --voxel_mm 1.0 --colors [--min_consistent 2] [--point_cloud] [--clean_mesh --dtu_test_dir <DTU_TEST>] \
        [--eval_dir <DTU eval data>]

A `val` forward sees one group of views and returns that group's partial mesh in its own normalised frame.  Here one model is
loaded once and every reference view gets a `val` forward WITHOUT geometry (ipts["extract_geometry"] = False: no per-group SDF
lattice), whose rendered depth map (--depth sdf_depth | render_depth) becomes a surf_amd.fusion.DepthView and is integrated into
one world-frame TSDF lattice (csrc/fuse.hip, 16 views per launch); the forward's outputs are dropped after each view.  With
--min_consistent K > 0 the views are collected first and only the depth pixels that K other views agree with are integrated
(the cross-view geometric consistency check of fusion.filter_views, csrc/depth_filter.hip: needs no object masks).  Then
FusionVolume.extract_mesh -> mesh_io.write_ply (<out>/meshes/fused/scan<N>.ply, world frame) -> optionally the DTU evaluation
protocol's cleaner (evaluation/clean_dtu.py) and evaluation.dtu_eval.evaluate_scan -> one JSON line.
With --point_cloud the same depth maps are ALSO merged into one point cloud, one point per surface sample (fusion.fuse_points,
csrc/point_cloud.hip, with the --min_consistent / --consistency_* flags) -> <out>/meshes/fused/scan<N>_points.ply, scored with
the evaluator's point-cloud mode when --eval_dir is given; the mesh and its fields of the record are what they are without it.
With --cloud_outliers K STD_RATIO (or --cloud_radius_outliers MIN_NEIGHBOURS) and --cloud_normals K the cloud is then cleaned
(surf_amd/point_filter.py, csrc/point_knn.hip: k nearest neighbours within --cloud_max_dist): statistical (or radius) outlier
removal first, then normals on what is left, turned towards the camera that saw each point; the filtered cloud is what goes to
<N>_points.ply (with nx ny nz) and to the scores, and the record gains `cloud_filter` and `cloud_normals`.
With --cloud_mesh [--cloud_mesh_radius VOXELS] [--cloud_mesh_min_points N] (needs --point_cloud and --cloud_normals) the oriented
cloud is then meshed itself: a point-set surface on the same lattice (surf_amd/point_surface.py, csrc/point_surface.hip), simplified
by --simplify_mm -> <N>_cloud_mesh.ply; the record gains `cloud_mesh` {radius, min_points, points, bricks, allocated_share, vertices,
faces, file, ms} and, with --eval_dir / --tnt_dir, that mesh's scores inside it.
With --smooth_iters N [--smooth_lambda L --smooth_mu M | --smooth_laplacian] [--smooth_max_move_mm X] [--smooth_free_boundary] the
mesh is smoothed (surf_amd/mesh_smooth.py, csrc/mesh_smooth.hip: N Taubin lambda|mu pairs, or N Laplacian steps) after --clean_mesh
and before --simplify_mm; positions move, faces and colours stay; the record gains `smooth` {iterations, lam, mu, pin_boundary,
max_move, vertices, boundary_vertices, isolated_vertices, moved_max, moved_rms, capped, ms}.  --cloud_mesh is smoothed the same way.
With --denoise_iters N [--denoise_vertex_iters N --denoise_sigma_r X --denoise_sigma_s_mm X --denoise_max_move_mm X
--denoise_free_boundary --denoise_backend device] the mesh is denoised with its edges kept (surf_amd/mesh_denoise.py,
csrc/mesh_denoise.hip: N bilateral passes over the face normals, then vertex passes that fit them) after --clean_mesh and before
--smooth_iters and --simplify_mm; the record gains `denoise` {normal_iterations, vertex_iterations, sigma_r, sigma_s, pin_boundary,
max_move, vertices, faces, degenerate_faces, boundary_vertices, moved_max, moved_rms, capped, ms}.  --cloud_mesh is denoised the
same way.
With --deviation [--deviation_backend device] [--deviation_max_mm X] (needs --denoise_iters, --smooth_iters or --simplify_mm) the record gains
`deviation` {forward, backward, hausdorff, max_dist, ms}: the vertex-sampled deviation (surf_amd/mesh_distance.py, exact
point-to-triangle distances) between the mesh after --clean_mesh and the mesh that is written; with --cloud_mesh the `cloud_mesh`
block gains the same `deviation` for the cloud mesh (its surface is extracted a second time without the mesh steps).

The lattice covers the union of the groups' normalised [-1, 1]^3 boxes (fusion.bounds_from_scale_mats; a first pass over the items
reads their scale_mats) at --voxel_mm world units per step, or --resolution points along the longest side.
With --sparse the lattice is brick-sparse (fusion.FusionVolume(sparse=True), csrc/fuse_sparse.hip): the same mesh from state kept
only near the measured surfaces, for lattices of 2^31 points and more (a dense lattice of that size exits at once); the record
gains `sparse`, `bricks`, `allocated_share` and `state_bytes`, and ms.finalize (allocation + integration of the recorded views).
With --scene NAME instead of --scan N the conf's own dataset (e.g. TanksDataset) is read for that scene and the outputs are named
after it (<NAME>.ply, <NAME>_points.ply, fused_<NAME>.json; the record carries `scene`); --tnt_dir D [--tau X] [--no_refine] then
scores the mesh (and the cloud) with the Tanks and Temples protocol (evaluation.fscore.evaluate_scene): precision, recall, fscore
(pcd_* for the cloud) and ms.evaluate_fscore.  --clean_mesh and --eval_dir are DTU's protocol and stay with --scan.
With --render_views [DIR] the fused model is then ray-cast (FusionVolume.ray_cast, csrc/ray_cast.hip: no mesh involved) from every
fused reference view's camera at its depth map's size: DIR (default <out>/renders/<name>) gets <view>_depth.pfm (z-depth in world
units, 0 = no hit), <view>_normal.png and, with --colors, <view>_color.png; the record gains `model_residual` - per view and pooled
over them, the share of the view's measured pixels the model also hits and the median / 90th percentile of |view depth - model
depth| over those, in world units and in lattice steps (fusion.view_residual: a quality number that needs no ground truth) - and
`render_views_ms`.  Without the switch the record and the files are what they were.
With --texture [--texture_texels T --texture_depth_tol_mm X --texture_min_cos C --texture_power N --texture_two_sided
--texture_backend host] the mesh that is written - after --clean_mesh, --denoise_iters, --smooth_iters and --simplify_mm - also gets
a texture atlas baked from the reference photographs of the fused views at their full resolution (surf_amd/mesh_texture.py,
csrc/mesh_texture.hip: every texel is projected into every photograph and tested against the mesh's own z-buffer there) ->
<name>_textured.obj, .mtl and .png beside the unchanged PLY; with --colors the vertex colours fill what no photograph sees.  The
record gains `texture` {texels_per_edge, atlas, faces, texels_owned, texels_seen, seen_share, faces_unseen, views,
views_per_seen_texel, depth_tol, min_cos, power, files, ms}.  Without the switch the record and the files are what they were.
Measurement harness like scripts/dtu_chamfer.py: one scan per call, no logging framework, no resume logic."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--conf", required=True, help="HOCON conf with `model` and `val_dataset` blocks (the reference's confs/*.conf)")
    ap.add_argument("--ckpt", default=None, help="checkpoint saved by runner.py (`model` key) - omitted: seeded random weights")
    ap.add_argument("--data_dir", default=None, help="overrides val_dataset.data_dir")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--scan", type=int, default=24)
    which.add_argument("--scene", default=None,
                       help="a scene by name (Tanks and Temples: Barn, Family, ...) of the conf's own dataset_name, instead of DTU's "
                            "scan<N>; the outputs are named after it")
    ap.add_argument("--ref_views", type=int, nargs="+", default=None, help="reference views to fuse (default: val_dataset.ref_view)")
    size = ap.add_mutually_exclusive_group()
    size.add_argument("--voxel_mm", type=float, default=None, help="lattice step in world units (DTU: millimetres)")
    size.add_argument("--resolution", type=int, default=None, help="lattice points along the longest side of the box (default 256)")
    ap.add_argument("--trunc_voxels", type=float, default=4.0, help="truncation distance in lattice steps")
    ap.add_argument("--sparse", action="store_true",
                    help="brick-sparse lattice (fusion.FusionVolume(sparse=True), csrc/fuse_sparse.hip): state only near the measured "
                         "surfaces, the same mesh; needed from 2^31 lattice points on.  The views' depth maps (and images) stay on "
                         "the device until the mesh is taken")
    ap.add_argument("--depth", default="sdf_depth", choices=["sdf_depth", "render_depth"], help="which rendered depth map is fused")
    ap.add_argument("--colors", action="store_true", help="also fuse color_fine and write red green blue into the PLY")
    ap.add_argument("--min_consistent", type=int, default=0,
                    help="fuse only the depth pixels that at least this many other views agree with (fusion.filter_views, "
                         "csrc/depth_filter.hip; 0: every pixel is fused)")
    ap.add_argument("--consistency_px", type=float, default=1.0, help="largest round-trip reprojection error of an agreeing view, pixels")
    ap.add_argument("--consistency_rel", type=float, default=0.01, help="largest relative depth error of an agreeing view")
    ap.add_argument("--consistency_sources", type=int, default=None,
                    help="test a view against its N nearest views by optical axis (default: all fused views)")
    ap.add_argument("--consistency_average", action="store_true", help="a kept depth becomes the mean over its agreeing views")
    ap.add_argument("--point_cloud", action="store_true",
                    help="also merge the depth maps into one point cloud (fusion.fuse_points: a pixel that --min_consistent other "
                         "views agree with is emitted once) and write meshes/fused/scan<N>_points.ply")
    ap.add_argument("--cloud_outliers", nargs=2, default=None, metavar=("K", "STD_RATIO"),
                    help="with --point_cloud: drop the points whose mean distance to their K nearest neighbours exceeds the cloud's "
                         "mean + STD_RATIO standard deviations, and the points with fewer than K neighbours within --cloud_max_dist "
                         "(surf_amd/point_filter.py, csrc/point_knn.hip)")
    ap.add_argument("--cloud_radius_outliers", type=int, default=None, metavar="MIN_NEIGHBOURS",
                    help="with --point_cloud: drop the points with fewer than MIN_NEIGHBOURS neighbours within --cloud_max_dist")
    ap.add_argument("--cloud_normals", type=int, default=None, metavar="K",
                    help="with --point_cloud: normals from the K nearest neighbours, turned towards the camera that saw the point; the "
                         "PLY gains nx ny nz.  Runs after the outlier step, on what is left")
    ap.add_argument("--cloud_max_dist", type=float, default=None,
                    help="search radius of the three cloud steps in world units (default: 10 lattice steps; a guess - the record's "
                         "`starved` count says when it is too small)")
    ap.add_argument("--cloud_mesh", action="store_true",
                    help="with --point_cloud and --cloud_normals: also mesh the oriented cloud itself, a point-set surface on the "
                         "--voxel_mm lattice (surf_amd/point_surface.py, csrc/point_surface.hip) -> <name>_cloud_mesh.ply, simplified "
                         "by --simplify_mm and scored like the mesh")
    ap.add_argument("--cloud_mesh_radius", type=float, default=3.0, metavar="VOXELS", help="support radius of --cloud_mesh in lattice steps")
    ap.add_argument("--cloud_mesh_min_points", type=int, default=4, metavar="N",
                    help="--cloud_mesh: a lattice point is observed with at least N points inside the radius")
    ap.add_argument("--clean_mesh", action="store_true",
                    help="the DTU evaluation protocol's cleaner on the world-frame mesh (evaluation/clean_dtu.py; needs --dtu_test_dir)")
    ap.add_argument("--dtu_test_dir", default=None, help="DTU_TEST tree (cameras/, scan<N>/mask/) of --clean_mesh")
    ap.add_argument("--clean_set", type=int, default=1, choices=[0, 1], help="view set of --clean_mesh")
    ap.add_argument("--clean_backend", default="host", choices=["host", "device"])
    ap.add_argument("--denoise_iters", type=int, default=None, metavar="N",
                    help="denoise the mesh and keep its edges: N bilateral filter passes over the face normals, then vertex passes "
                         "that fit them (surf_amd/mesh_denoise.py): after --clean_mesh, before --smooth_iters and --simplify_mm; "
                         "also applied to --cloud_mesh")
    ap.add_argument("--denoise_vertex_iters", type=int, default=10, metavar="N", help="vertex passes after the normal passes")
    ap.add_argument("--denoise_sigma_r", type=float, default=0.35,
                    help="normals further apart than 3 of these (as a chord of the unit sphere) do not average each other")
    ap.add_argument("--denoise_sigma_s_mm", type=float, default=None,
                    help="the same for the distance of two face centroids (world units; DTU: millimetres); default: the mean side length")
    ap.add_argument("--denoise_max_move_mm", type=float, default=None,
                    help="no vertex ends further than this from where it started (world units; DTU: millimetres)")
    ap.add_argument("--denoise_free_boundary", action="store_true", help="let the vertices on open edges move too (default: pinned)")
    ap.add_argument("--denoise_backend", default="host", choices=["host", "device"])
    ap.add_argument("--smooth_iters", type=int, default=None, metavar="N",
                    help="smooth the mesh with N Taubin lambda|mu pairs (surf_amd/mesh_smooth.py): after --clean_mesh, before "
                         "--simplify_mm; also applied to --cloud_mesh")
    ap.add_argument("--smooth_lambda", type=float, default=0.5, help="0 < lambda <= 1: the shrinking step's factor")
    ap.add_argument("--smooth_mu", type=float, default=-0.53, help="mu < -lambda: the inflating step's factor")
    ap.add_argument("--smooth_laplacian", action="store_true", help="N plain Laplacian steps with --smooth_lambda, no mu step (shrinks)")
    ap.add_argument("--smooth_max_move_mm", type=float, default=None,
                    help="no vertex ends further than this from where it started (world units; DTU: millimetres)")
    ap.add_argument("--smooth_free_boundary", action="store_true", help="let the vertices on open edges move too (default: pinned)")
    ap.add_argument("--smooth_backend", default="host", choices=["host", "device"])
    ap.add_argument("--simplify_mm", type=float, default=None,
                    help="simplify the mesh to one vertex per cell of this size (world units; DTU: millimetres) by quadric vertex "
                         "clustering (surf_amd/mesh_simplify.py): the last mesh step, after --clean_mesh, before the PLY and the scores")
    ap.add_argument("--simplify_backend", default="host", choices=["host", "device"])
    ap.add_argument("--deviation", action="store_true",
                    help="report how far --smooth_iters / --simplify_mm moved the surface: the vertex-sampled deviation between the "
                         "mesh before them and the mesh that is written (surf_amd/mesh_distance.py)")
    ap.add_argument("--deviation_backend", default="host", choices=["host", "device"])
    ap.add_argument("--deviation_max_mm", type=float, default=None,
                    help="vertices without a face of the other mesh nearer than this count as `beyond` (world units; default: "
                         "the diagonal of the two meshes' joint bounding box)")
    ap.add_argument("--texture", action="store_true",
                    help="also bake the fused views' reference photographs into a texture atlas of the mesh that is written "
                         "(surf_amd/mesh_texture.py) -> <name>_textured.obj, .mtl and .png beside the PLY")
    ap.add_argument("--texture_texels", type=int, default=8, metavar="T", help="texels along a face's edge, 4..64: T (T+1) / 2 a face")
    ap.add_argument("--texture_depth_tol_mm", type=float, default=None,
                    help="a texel further than this behind the mesh's own depth map is hidden from that photograph (world units; "
                         "DTU: millimetres; default: 2 lattice steps)")
    ap.add_argument("--texture_min_cos", type=float, default=0.2, help="photographs that see a face more obliquely are not used for it")
    ap.add_argument("--texture_power", type=int, default=4, metavar="N", help="a photograph's weight is cos^N, 1..16")
    ap.add_argument("--texture_two_sided", action="store_true", help="photographs of a face's back side count too")
    ap.add_argument("--texture_backend", default="device", choices=["host", "device"])
    ap.add_argument("--eval_dir", default=None, help="DTU evaluation data (ObsMask/, Points/stl/): also report the Chamfer distance")
    ap.add_argument("--eval_device", default="cpu", choices=["cpu", "gpu"])
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--shuffle_seed", type=int, default=0)
    ap.add_argument("--tnt_dir", default=None,
                    help="Tanks and Temples ground truth (<scene>/<scene>.ply, .json, _trans.txt): also report precision, recall and "
                         "F-score of the mesh (and of the cloud with --point_cloud), evaluation/fscore.py; needs --scene")
    ap.add_argument("--tau", type=float, default=None, help="F-score distance threshold (default: the benchmark's value for the scene)")
    ap.add_argument("--no_refine", action="store_true", help="F-score: use <scene>_trans.txt as it is, no ICP")
    ap.add_argument("--render_views", nargs="?", const="", default=None, metavar="DIR",
                    help="after fusing, ray-cast the model from every fused reference view's camera (FusionVolume.ray_cast): depth "
                         "(.pfm), normal and colour (.png) maps into DIR (default <out_dir>/renders/<name>), and `model_residual` in "
                         "the record")
    ap.add_argument("--out_dir", default="./outputs")
    ap.add_argument("--sdf_precision", default=None, choices=["f32", "bf16x3", "f16x2"])
    ap.add_argument("--logit_override", default=None, choices=["sphere"],
                    help="(tests) replace the U-Nets' matching logits by a sphere-concentrated field, as an untrained model needs")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def denoise_params(args):
    """The --denoise_* flags as mesh_denoise's argument dict, or None without --denoise_iters (a Namespace built by hand may lack
    them)."""
    iters = getattr(args, "denoise_iters", None)
    if iters is None:
        return None
    from surf_amd.mesh_denoise import check_params
    try:
        return check_params({"normal_iterations": iters, "vertex_iterations": getattr(args, "denoise_vertex_iters", 10),
                             "sigma_r": getattr(args, "denoise_sigma_r", 0.35), "sigma_s": getattr(args, "denoise_sigma_s_mm", None),
                             "pin_boundary": not getattr(args, "denoise_free_boundary", False),
                             "max_move": getattr(args, "denoise_max_move_mm", None)})
    except ValueError as e:
        raise SystemExit(f"fuse_scene: {e}")


def texture_params(args, voxel):
    """The --texture_* flags as mesh_texture's argument dict, or None without --texture (a Namespace built by hand may lack them).
    voxel: the lattice step, of which the default depth tolerance is two."""
    if not getattr(args, "texture", False):
        return None
    from surf_amd.mesh_texture import check_params
    tol = getattr(args, "texture_depth_tol_mm", None)
    try:
        return check_params({"texels_per_edge": getattr(args, "texture_texels", 8), "depth_tol": 2.0 * voxel if tol is None else tol,
                             "min_cos": getattr(args, "texture_min_cos", 0.2), "power": getattr(args, "texture_power", 4),
                             "two_sided": getattr(args, "texture_two_sided", False)})
    except ValueError as e:
        raise SystemExit(f"fuse_scene: {e}")


def texture_mesh(v, t, colors, views, params, path, backend, dev):
    """--texture: bake `views` into an atlas of the mesh (v, t) and write <path>.obj / .mtl / .png: (the `texture` block of the
    record, uv, atlas)."""
    from surf_amd import mesh_io
    from surf_amd.mesh_texture import texture_step
    try:
        uv, atlas, rec = texture_step(v, t, views, params, backend=backend, device=dev, vertex_colors=colors)
    except ValueError as e:
        raise SystemExit(f"fuse_scene: {e}")
    rec["files"] = list(mesh_io.write_obj(path, v, t, uv, atlas))
    return rec, uv, atlas


def smooth_params(args):
    """The --smooth_* flags as mesh_smooth's argument dict, or None without --smooth_iters (a Namespace built by hand may lack them)."""
    iters = getattr(args, "smooth_iters", None)
    if iters is None:
        return None
    from surf_amd.mesh_smooth import check_params
    try:
        return check_params({"iterations": iters, "lam": getattr(args, "smooth_lambda", 0.5),
                             "mu": None if getattr(args, "smooth_laplacian", False) else getattr(args, "smooth_mu", -0.53),
                             "pin_boundary": not getattr(args, "smooth_free_boundary", False),
                             "max_move": getattr(args, "smooth_max_move_mm", None)})
    except ValueError as e:
        raise SystemExit(f"fuse_scene: {e}")


def mesh_steps(v, t, colors, args, denoise, smooth, dev):
    """The mesh steps after the cleaner, in their order - denoise, smooth, simplify - each only if asked for: (vertices, triangles,
    colors, denoise record, smooth record, simplify record), a record None for a step that did not run."""
    denoised = None
    if denoise is not None:                             # after the cleaner, before the filter that rounds what this one keeps
        from surf_amd.mesh_denoise import denoise_step
        try:
            v, _, denoised = denoise_step(v, t, denoise, backend=getattr(args, "denoise_backend", "host"), device=dev)
        except ValueError as e:
            raise SystemExit(f"fuse_scene: {e}")
    smoothed = None
    if smooth is not None:                              # after the cleaner, whose masks are about the measured surface
        from surf_amd.mesh_smooth import smooth_step
        v, _, smoothed = smooth_step(v, t, smooth, backend=getattr(args, "smooth_backend", "host"), device=dev)
    simplified = None
    if args.simplify_mm is not None:                    # the last mesh step: the cleaner's component threshold is about the full mesh
        from surf_amd.mesh_simplify import simplify_step
        v, t, _, colors, simplified = simplify_step(v, t, args.simplify_mm, colors=colors, backend=args.simplify_backend, device=dev)
        if len(t) == 0:
            raise SystemExit(f"fuse_scene: --simplify_mm {args.simplify_mm} leaves no face (the cell swallows the mesh)")
    return v, t, colors, denoised, smoothed, simplified


def run(args, state=None):
    """Returns the JSON record.  state (dict, tests): receives the live `model`, the FusionVolume `volume` and the final world-frame
    `vertices` / `triangles` (/ `colors`)."""
    from surf_amd import conf as C
    from surf_amd import fusion, mesh_io, synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.evaluation import clean_dtu, dtu_eval
    from surf_amd.surf import SuRF

    dev = torch.device(args.device)
    # a caller may build the Namespace by hand without the scene / F-score attributes
    scene, tnt_dir = getattr(args, "scene", None), getattr(args, "tnt_dir", None)
    render_dir = getattr(args, "render_views", None)
    name = scene if scene is not None else f"scan{args.scan}"
    if scene is not None and (args.clean_mesh or args.eval_dir is not None):
        raise SystemExit("fuse_scene: --clean_mesh and --eval_dir are DTU's protocol and need --scan, not --scene")
    if tnt_dir is not None and scene is None:
        raise SystemExit("fuse_scene: --tnt_dir needs --scene")
    if args.clean_mesh and args.dtu_test_dir is None:
        raise SystemExit("fuse_scene: --clean_mesh needs --dtu_test_dir")
    # a caller may build the Namespace by hand without the cloud steps' attributes
    cloud_outliers, cloud_radius = getattr(args, "cloud_outliers", None), getattr(args, "cloud_radius_outliers", None)
    cloud_normals, cloud_max_dist = getattr(args, "cloud_normals", None), getattr(args, "cloud_max_dist", None)
    cloud_steps = cloud_outliers is not None or cloud_radius is not None or cloud_normals is not None
    cloud_records = {}
    if cloud_steps and not args.point_cloud:
        raise SystemExit("fuse_scene: --cloud_outliers, --cloud_radius_outliers and --cloud_normals need --point_cloud")
    if cloud_outliers is not None and cloud_radius is not None:
        raise SystemExit("fuse_scene: one of --cloud_outliers and --cloud_radius_outliers")
    cloud_mesh = bool(getattr(args, "cloud_mesh", False))
    cloud_mesh_record = None
    if cloud_mesh and not (args.point_cloud and cloud_normals is not None):
        raise SystemExit("fuse_scene: --cloud_mesh needs --point_cloud and --cloud_normals (the surface is taken from oriented points)")
    smooth = smooth_params(args)
    denoise = denoise_params(args)
    deviation = bool(getattr(args, "deviation", False))
    if deviation and smooth is None and denoise is None and args.simplify_mm is None:
        raise SystemExit("fuse_scene: --deviation compares the mesh before and after --denoise_iters / --smooth_iters / --simplify_mm: "
                         "give one of them")
    cfg = C.parse_file(args.conf)
    dconf = cfg["val_dataset"]
    if args.data_dir is not None:
        dconf["data_dir"] = args.data_dir
    dconf["scene"] = [name]
    if args.ref_views is not None:
        dconf["ref_view"] = list(args.ref_views)
    mconf = cfg["model"]
    if args.sdf_precision is not None:
        mconf["implicit_surface"]["render"]["sdf_precision"] = args.sdf_precision

    t0 = time.perf_counter()
    loader, _, dataset = get_loader(dconf, "val", False, num_workers=0)
    if len(dataset) < 1:
        raise SystemExit(f"fuse_scene: no validation item for {name} under {dconf['data_dir']}")
    torch.manual_seed(0)
    model = SuRF(mconf)
    if args.ckpt is not None:
        ckpt = torch.load(args.ckpt, map_location="cpu")
        model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt, strict=True)
    model = model.to(dev).eval()
    if args.logit_override == "sphere":
        model.logit_override = synthetic.sphere_logit
    ms = {"load": 1e3 * (time.perf_counter() - t0)}

    # ---- the lattice: the union of the groups' unit boxes in the world frame ----
    t0 = time.perf_counter()
    lo, hi = fusion.bounds_from_scale_mats([dataset[i]["scale_mat"] for i in range(len(dataset))])
    voxel = args.voxel_mm if args.voxel_mm is not None else float((hi - lo).max()) / ((args.resolution or 256) - 1)
    shape = [len(a) for a in fusion.lattice_axes(lo, hi, voxel)]
    if not args.sparse and int(np.prod(shape, dtype=np.int64)) >= 2 ** 31:
        raise SystemExit(f"fuse_scene: a dense lattice of {shape[0]} x {shape[1]} x {shape[2]} points is past the mesh step's limit "
                         "of 2^31 points (and takes 8 to 20 B per point): use --sparse")
    volume = fusion.FusionVolume((lo, hi, voxel), trunc=args.trunc_voxels * voxel, colors=args.colors, device=dev, sparse=args.sparse)
    ms["lattice"] = 1e3 * (time.perf_counter() - t0)
    texture = texture_params(args, voxel)
    texture_views = []                                  # --texture: the reference photograph of every fused view, world frame

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    # ---- one forward per reference view; views are integrated 16 per launch ----
    ms.update(forward=0.0, integrate=0.0)
    pending, cloud_views = [], []
    render_views, render_names = [], []                # --render_views: the views as they are fused, and what their files are called

    def flush():
        t0 = time.perf_counter()
        volume.integrate(pending)
        sync()
        ms["integrate"] += 1e3 * (time.perf_counter() - t0)
        pending.clear()

    for item in loader:
        t0 = time.perf_counter()
        inputs = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in item.items()}
        inputs["extract_geometry"] = False
        with torch.no_grad():
            out = model("val", inputs, cos_anneal_ratio=1.0)
        sync()
        pending.append(fusion.view_from_val(item, out, depth=args.depth))
        if texture is not None:
            from surf_amd.mesh_texture import view_from_item
            texture_views.append(view_from_item(item, 0))
        if args.point_cloud:
            cloud_views.append(pending[-1])
        if render_dir is not None:
            render_views.append(pending[-1])
            ids = item.get("view_ids")
            render_names.append(f"{name}_{len(render_names):03d}" if ids is None else f"{name}_view{int(ids.reshape(-1)[0]):03d}")
        del out, inputs
        ms["forward"] += 1e3 * (time.perf_counter() - t0)
        if len(pending) == 16 and args.min_consistent == 0:
            flush()
    cloud = None
    if args.point_cloud:
        # ---- every view is there: the consistent depths as one cloud, each surface sample once (the unfiltered maps go in) ----
        t0 = time.perf_counter()
        near = None if args.consistency_sources is None else fusion.nearest_sources(cloud_views, args.consistency_sources)
        cloud = fusion.fuse_points(cloud_views, args.min_consistent, args.consistency_px, args.consistency_rel, sources=near,
                                   device=dev)
        ms["points"] = 1e3 * (time.perf_counter() - t0)
        points_path = os.path.join(args.out_dir, "meshes", "fused", f"{name}_points.ply")
        if cloud_steps:
            # ---- outliers first, normals on what is left: the filtered cloud is what is written and scored ----
            from surf_amd import point_filter
            max_dist = cloud_max_dist if cloud_max_dist is not None else 10.0 * voxel
            ratio = None if cloud_outliers is None else (int(cloud_outliers[0]), float(cloud_outliers[1]))
            cloud, cloud_nrm, cloud_records = point_filter.clean_step(cloud, cloud_views, outliers=ratio, radius_outliers=cloud_radius,
                                                                      normals_k=cloud_normals, max_dist=max_dist, device=dev)
            mesh_io.write_ply_points(points_path, cloud.points, cloud.colors, normals=cloud_nrm)
            if cloud_mesh:
                # ---- the oriented cloud as a surface of its own: a point-set surface on the fusion lattice ----
                from surf_amd import point_surface
                t0 = time.perf_counter()
                st = {}
                radius = float(getattr(args, "cloud_mesh_radius", 3.0)) * voxel
                min_points = int(getattr(args, "cloud_mesh_min_points", 4))
                cm = point_surface.reconstruct(cloud, cloud_nrm, voxel, radius=radius, min_points=min_points, bounds=(lo, hi),
                                               simplify_cell=args.simplify_mm, device=dev, stats=st, smooth=smooth, denoise=denoise)
                if len(cm[1]) == 0:
                    raise SystemExit("fuse_scene: --cloud_mesh found no zero crossing between observed lattice points (empty mesh)")
                cloud_deviated = None
                if deviation:                           # mesh A: the same surface extracted again without the mesh steps
                    from surf_amd.mesh_distance import deviation_step
                    ca = point_surface.reconstruct(cloud, cloud_nrm, voxel, radius=radius, min_points=min_points, bounds=(lo, hi),
                                                   device=dev)
                    try:
                        cloud_deviated = deviation_step(ca[0], ca[1], cm[0], cm[1], getattr(args, "deviation_max_mm", None),
                                                        backend=getattr(args, "deviation_backend", "host"), device=dev)
                    except ValueError as e:
                        raise SystemExit(f"fuse_scene: {e}")
                cloud_mesh_path = os.path.join(args.out_dir, "meshes", "fused", f"{name}_cloud_mesh.ply")
                mesh_io.write_ply(cloud_mesh_path, cm[0], cm[1], colors=cm[2] if len(cm) > 2 else None)
                cloud_mesh_record = {"radius": radius, "min_points": min_points, "points": st["points"], "bricks": st["bricks"],
                                     "allocated_share": st["allocated_share"], "vertices": st["vertices"], "faces": st["faces"],
                                     "file": cloud_mesh_path, "ms": 1e3 * (time.perf_counter() - t0)}
                if cloud_deviated is not None:          # without the flag the block is what it was
                    cloud_mesh_record["deviation"] = cloud_deviated
        else:
            mesh_io.write_ply_points(points_path, cloud.points, cloud.colors)
        cloud_views.clear()
    filtered = None
    if args.min_consistent > 0:
        # ---- every view is there: drop the depths too few other views agree with, then integrate 16 per launch ----
        t0 = time.perf_counter()
        filtered = {}
        near = None if args.consistency_sources is None else fusion.nearest_sources(pending, args.consistency_sources)
        views = fusion.filter_views(pending, args.min_consistent, args.consistency_px, args.consistency_rel, sources=near,
                                    average=args.consistency_average, device=dev, stats=filtered)
        sync()
        ms["filter"] = 1e3 * (time.perf_counter() - t0)
        pending.clear()
        if render_dir is not None:
            render_views = list(views)                 # the residual is taken against the depths that were fused
        for s in range(0, len(views), 16):
            pending.extend(views[s:s + 16])
            flush()
    if pending:
        flush()

    if args.sparse:
        # ---- integrate() only recorded the views: allocate bricks over all of them, then integrate all of them ----
        t0 = time.perf_counter()
        volume.finalize()
        sync()
        ms["finalize"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    mesh = volume.extract_mesh()
    v, t, colors = mesh[0], mesh[1], (mesh[2] if args.colors else None)
    ms["extract"] = 1e3 * (time.perf_counter() - t0)
    if len(t) == 0:
        raise SystemExit("fuse_scene: the fused lattice has no zero crossing between observed points (empty mesh)")
    if args.clean_mesh:
        t0 = time.perf_counter()
        v, t, kept = clean_dtu.clean_dtu_scan(v, t, args.dtu_test_dir, args.scan, view_set=args.clean_set, backend=args.clean_backend,
                                              device=dev.type, return_index=True)
        colors = None if colors is None else colors[kept]
        ms["clean"] = 1e3 * (time.perf_counter() - t0)
    before = (v, t) if deviation else None              # mesh A of --deviation: after the cleaner, before the steps it measures
    v, t, colors, denoised, smoothed, simplified = mesh_steps(v, t, colors, args, denoise, smooth, dev)
    deviated = None
    if before is not None:                              # mesh B is the mesh that is written
        from surf_amd.mesh_distance import deviation_step
        try:
            deviated = deviation_step(before[0], before[1], v, t, getattr(args, "deviation_max_mm", None),
                                      backend=getattr(args, "deviation_backend", "host"), device=dev)
        except ValueError as e:
            raise SystemExit(f"fuse_scene: {e}")
    t0 = time.perf_counter()
    mesh_path = os.path.join(args.out_dir, "meshes", "fused", f"{name}.ply")
    mesh_io.write_ply(mesh_path, v, t, colors=colors)
    ms["write"] = 1e3 * (time.perf_counter() - t0)
    textured = None
    if texture is not None:                             # on the mesh that is written; the PLY stays what it is
        textured, uv, atlas = texture_mesh(v, t, colors, texture_views, texture,
                                           os.path.join(args.out_dir, "meshes", "fused", f"{name}_textured.obj"),
                                           getattr(args, "texture_backend", "device"), dev)
    if state is not None:
        state.update(model=model, volume=volume, vertices=v, triangles=t, colors=colors)
        if textured is not None:
            state.update(texture_views=texture_views, uv=uv, atlas=atlas)
        if cloud is not None:
            state.update(cloud=cloud)
        if cloud_mesh_record is not None:
            state.update(cloud_mesh=cm)
            if cloud_mesh_record.get("deviation") is not None:
                state.update(cloud_mesh_before=ca)
    model_residual = None
    if render_dir is not None:
        # ---- the fused model seen from every fused view's camera: no mesh involved, one kernel launch and one copy per view ----
        from PIL import Image
        from surf_amd.datasets import mvs_io
        t0 = time.perf_counter()
        render_dir = render_dir or os.path.join(args.out_dir, "renders", name)
        os.makedirs(render_dir, exist_ok=True)
        per_view, residuals = [], []
        for vname, view in zip(render_names, render_views):
            cast = volume.ray_cast(view.P, tuple(view.depth.shape))
            mvs_io.write_pfm(os.path.join(render_dir, f"{vname}_depth.pfm"), cast["depth"])
            Image.fromarray(fusion.quantise_colors_host(0.5 * cast["normal"] + 0.5 * (cast["depth"] > 0)[..., None])).save(
                os.path.join(render_dir, f"{vname}_normal.png"))
            if cast["color"] is not None:
                Image.fromarray(fusion.quantise_colors_host(cast["color"])).save(os.path.join(render_dir, f"{vname}_color.png"))
            res = fusion.view_residual(view, cast)
            residuals.append(res.pop("residuals"))
            per_view.append({"view": vname, **res})
        measured, hit = sum(r["measured"] for r in per_view), sum(r["hit"] for r in per_view)
        pooled = {"measured": measured, "hit": hit, "hit_share": hit / max(measured, 1)}
        pooled.update(fusion.pooled_residual(np.concatenate(residuals) if residuals else np.zeros(0), volume.lattice()[1]))
        model_residual = {"views": per_view, "pooled": pooled, "dir": render_dir}
        render_ms = 1e3 * (time.perf_counter() - t0)
    rec = {("scan" if scene is None else "scene"): (args.scan if scene is None else scene), "views_fused": volume.n_views, "lattice": list(volume.shape), "voxel": voxel, "trunc": volume.trunc,
           "observed_share": volume.observed_share(), "vertices": int(len(v)), "triangles": int(len(t)), "depth": args.depth,
           "colors": bool(args.colors), "cleaned": bool(args.clean_mesh), "mesh": mesh_path, "ms": ms}
    if args.sparse:                                     # without the flag the record is what it was
        rec.update(sparse=True, bricks=volume.n_bricks, allocated_share=volume.allocated_share(), state_bytes=volume.state_bytes())
    if denoised is not None:                            # without the flag the record is what it was
        rec.update(denoise=denoised)
    if smoothed is not None:                            # without the flag the record is what it was
        rec.update(smooth=smoothed)
    if simplified is not None:                          # without the flag the record is what it was
        rec.update(simplify=simplified)
    if deviated is not None:                            # without the flag the record is what it was
        rec.update(deviation=deviated)
    if textured is not None:                            # without the flag the record is what it was
        rec.update(texture=textured)
    if model_residual is not None:                      # without the switch the record is what it was
        rec.update(model_residual=model_residual, render_views_ms=render_ms)
    if filtered is not None:
        rec.update(min_consistent=args.min_consistent, kept_share=sum(filtered["kept"]) / max(sum(filtered["measured"]), 1))
    if cloud is not None:
        rec.update(points=int(len(cloud.points)), points_file=points_path)
        rec.update(cloud_records)                       # cloud_filter / cloud_normals: without the flags the record is what it was
    if cloud_mesh_record is not None:                   # without the flag the record is what it was
        rec.update(cloud_mesh=cloud_mesh_record)
    if args.eval_dir is not None:
        t0 = time.perf_counter()
        d2s, s2d, overall = dtu_eval.evaluate_scan(mesh_path, args.eval_dir, args.scan, patch_size=args.patch_size,
                                                   max_dist=args.max_dist, downsample_density=args.downsample_density,
                                                   rng=np.random.default_rng(args.shuffle_seed), device=args.eval_device)
        ms["evaluate"] = 1e3 * (time.perf_counter() - t0)
        rec.update(d2s=d2s, s2d=s2d, chamfer=overall)
        if cloud is not None:
            t0 = time.perf_counter()
            d2s, s2d, overall = dtu_eval.evaluate_scan(points_path, args.eval_dir, args.scan, mode="pcd", patch_size=args.patch_size,
                                                       max_dist=args.max_dist, downsample_density=args.downsample_density,
                                                       rng=np.random.default_rng(args.shuffle_seed), device=args.eval_device)
            ms["evaluate_points"] = 1e3 * (time.perf_counter() - t0)
            rec.update(pcd_d2s=d2s, pcd_s2d=s2d, pcd_chamfer=overall)
        if cloud_mesh_record is not None:
            t0 = time.perf_counter()
            d2s, s2d, overall = dtu_eval.evaluate_scan(cloud_mesh_record["file"], args.eval_dir, args.scan, patch_size=args.patch_size,
                                                       max_dist=args.max_dist, downsample_density=args.downsample_density,
                                                       rng=np.random.default_rng(args.shuffle_seed), device=args.eval_device)
            ms["evaluate_cloud_mesh"] = 1e3 * (time.perf_counter() - t0)
            cloud_mesh_record.update(d2s=d2s, s2d=s2d, chamfer=overall)
    if tnt_dir is not None:
        from surf_amd.evaluation import fscore
        t0 = time.perf_counter()
        kw = dict(tau=getattr(args, "tau", None), refine=not getattr(args, "no_refine", False), device=args.eval_device)
        res = fscore.evaluate_scene(mesh_path, tnt_dir, scene, mode="mesh", **kw)
        rec.update(precision=res["precision"], recall=res["recall"], fscore=res["fscore"], tau=res["tau"])
        if cloud is not None:
            res = fscore.evaluate_scene(points_path, tnt_dir, scene, mode="pcd", **kw)
            rec.update(pcd_precision=res["precision"], pcd_recall=res["recall"], pcd_fscore=res["fscore"])
        if cloud_mesh_record is not None:
            res = fscore.evaluate_scene(cloud_mesh_record["file"], tnt_dir, scene, mode="mesh", **kw)
            cloud_mesh_record.update(precision=res["precision"], recall=res["recall"], fscore=res["fscore"])
        ms["evaluate_fscore"] = 1e3 * (time.perf_counter() - t0)
    with open(os.path.join(args.out_dir, f"fused_{name}.json"), "w") as f:
        json.dump(rec, f)
    return rec


def main(argv=None):
    print(json.dumps(run(parse_args(argv))))


if __name__ == "__main__":
    main()
