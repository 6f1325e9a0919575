#!/usr/bin/env python3
"""The second half of BASELINE.json's metric - "DTU scan24 Chamfer vs ref" - as ONE command:

    python scripts/dtu_chamfer.py --conf confs/surf.conf --ckpt ckpt.pth --data_dir <DTU> --eval_dir <DTU eval data> --scan 24

loader (surf_amd.datasets, the val_dataset block of the HOCON conf)  ->  SuRF(conf.model).load_state_dict(ckpt["model"])
-> model("val", inputs)                                     (runner.py:213-229: FPN, 4-stage volumes, render, SDF lattice, marching cubes)
-> [clean_mesh with the item's masks, --clean_mesh]         (runner.py:233-234, utils/clean_mesh.py:110-130;
                                                             --clean_backend device: the same cleaned mesh from mesh_clean.hip)
   or, with --clean_protocol dtu_test, AFTER scale_mat:      (evaluation/clean_mesh.py, the cleaner of the published numbers:
   clean_dtu.clean_dtu_scan with --dtu_test_dir's masks       world millimetres, DTU_TEST object masks, view set --clean_set)
-> [per-vertex normals + blended colours, --vertex_colors]  (ImplicitSurface.vertex_attributes on the final vertex set)
-> mesh_io.export_mesh(<out>/meshes/final/scan<N>.ply, scale_mat)   (runner.py:236-240; the file name evaluation/dtu_eval.py reads)
-> evaluation.dtu_eval.evaluate_scan                        (evaluation/dtu_eval.py:31-190)
-> one JSON line: {"scan", "d2s", "s2d", "chamfer", "reference_chamfer", "delta", ...}.

Needs external data (a DTU tree, the DTU evaluation files ObsMask/ + Points/stl/, a checkpoint): nothing in the test-suite's
default path calls it with real data; tests/test_end_to_end_dtu.py runs it on a synthetic scene written in DTU's file formats.
Measurement harness, not a training / serving control plane: no logging framework, no resume logic, one scan per call.

--down_rule {dilate,floor,pad0}: which stride-2 site rule of torchsparse the checkpoint's sparse U-Net was trained under
(row a5 is parity-unpinned: torchsparse is not available to the build; with three rules behind one switch the authors'
checkpoint picks its own - the right rule is the one that reproduces the published Chamfer, README.md:87-106).
--kernel_order {xfast,zfast} / --transposed_pairing {same,mirrored}: the two other torchsparse conventions a loaded checkpoint
depends on (surf_amd.reg_network.slice_permutation): the enumeration of the 27 kernel slices and which slice a transposed layer
pairs with which offset.  --sweep runs all 3 x 2 x 2 = 12 combinations on ONE loaded model (set_conventions between runs, one mesh
and one evaluation each), prints one line per combination and a final line naming the combination whose Chamfer is closest to
--reference_chamfer: twelve candidates and a one-command discriminator instead of one guess that may scramble the checkpoint.
--reference_chamfer X: the reference's own number for this scan (or the published mean 1.05); "delta" = ours - X is then the
quantity north_star bounds by 0.01.
--texture [--texture_texels T --texture_depth_tol X --texture_min_cos C --texture_power N --texture_two_sided --texture_backend host]:
the world-frame mesh that is written also gets a texture atlas baked from ALL photographs of the item at their full resolution
(surf_amd/mesh_texture.py) -> scan<N>_textured.obj, .mtl and .png beside the PLY, and a `texture` block in the record; the PLY and
the scores are what they are without it.  The tolerance is in the written mesh's own units, the world frame."""
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
    ap.add_argument("--eval_dir", required=True, help="DTU evaluation data: ObsMask/ObsMask<N>_10.mat, ObsMask/Plane<N>.mat, Points/stl/stl<NNN>_total.ply")
    ap.add_argument("--scan", type=int, default=24)
    ap.add_argument("--ref_view", type=int, default=None, help="overrides val_dataset.ref_view")
    ap.add_argument("--out_dir", default="./outputs")
    ap.add_argument("--down_rule", default=None, choices=["dilate", "floor", "pad0"], help="model.reg_network.down_rule")
    ap.add_argument("--kernel_order", default=None, choices=["xfast", "zfast"], help="model.reg_network.kernel_order")
    ap.add_argument("--transposed_pairing", default=None, choices=["same", "mirrored"], help="model.reg_network.transposed_pairing")
    ap.add_argument("--sweep", action="store_true",
                    help="evaluate every (down_rule, kernel_order, transposed_pairing) combination and report the one closest to "
                         "--reference_chamfer")
    ap.add_argument("--sdf_precision", default=None, choices=["f32", "bf16x3", "f16x2"])
    ap.add_argument("--mesh_resolution", type=int, default=512, help="lattice points per axis of the mesh (band: up to 8192)")
    ap.add_argument("--mesh_extraction", default=None, choices=["dense", "band"],
                    help="model.implicit_surface.render.mesh_extraction: whole lattice or bricks near the surface (same mesh)")
    ap.add_argument("--clean_mesh", action="store_true", help="runner.py --clean_mesh: drop faces outside the dilated masks / frusta")
    ap.add_argument("--clean_backend", default="host", choices=["host", "device"],
                    help="where --clean_mesh runs (device: the HIP kernels of mesh_clean.hip, same cleaned mesh)")
    ap.add_argument("--clean_protocol", default="runner", choices=["runner", "dtu_test"],
                    help="which cleaner --clean_mesh runs: runner.py's (the loader's masks, normalised frame) or the DTU evaluation "
                         "protocol's (evaluation/clean_mesh.py: --dtu_test_dir's object masks, world frame, after scale_mat)")
    ap.add_argument("--dtu_test_dir", default=None, help="DTU_TEST tree (cameras/, scan<N>/mask/) of --clean_protocol dtu_test")
    ap.add_argument("--clean_set", type=int, default=1, choices=[0, 1], help="view set of --clean_protocol dtu_test")
    ap.add_argument("--vertex_colors", action="store_true",
                    help="also write per-vertex normals (nx ny nz) and blended colours (red green blue) into the PLY "
                         "(ImplicitSurface.vertex_attributes on the final vertex set; geometry and Chamfer unchanged)")
    ap.add_argument("--denoise_iters", type=int, default=None, metavar="N",
                    help="denoise the mesh and keep its edges: N bilateral filter passes over the face normals, then vertex passes "
                         "that fit them (surf_amd/mesh_denoise.py) after --clean_mesh and before --smooth_iters and "
                         "--simplify_cell; with --vertex_colors the normals are recomputed, on the side of the ones they replace")
    ap.add_argument("--denoise_vertex_iters", type=int, default=10, metavar="N", help="vertex passes after the normal passes")
    ap.add_argument("--denoise_sigma_r", type=float, default=0.35,
                    help="normals further apart than 3 of these (as a chord of the unit sphere) do not average each other")
    ap.add_argument("--denoise_sigma_s", type=float, default=None,
                    help="the same for the distance of two face centroids, in the mesh's own units; default: the mean side length")
    ap.add_argument("--denoise_max_move", type=float, default=None,
                    help="no vertex ends further than this from where it started, in the mesh's own units (the normalised frame)")
    ap.add_argument("--denoise_free_boundary", action="store_true", help="let the vertices on open edges move too (default: pinned)")
    ap.add_argument("--denoise_backend", default="host", choices=["host", "device"])
    ap.add_argument("--smooth_iters", type=int, default=None, metavar="N",
                    help="smooth the mesh with N Taubin lambda|mu pairs (surf_amd/mesh_smooth.py) after --clean_mesh and before "
                         "--simplify_cell; with --vertex_colors the normals are recomputed from the smoothed mesh, on the side of "
                         "the ones they replace")
    ap.add_argument("--smooth_lambda", type=float, default=0.5, help="0 < lambda <= 1: the shrinking step's factor")
    ap.add_argument("--smooth_mu", type=float, default=-0.53, help="mu < -lambda: the inflating step's factor")
    ap.add_argument("--smooth_laplacian", action="store_true", help="N plain Laplacian steps with --smooth_lambda, no mu step (shrinks)")
    ap.add_argument("--smooth_max_move", type=float, default=None,
                    help="no vertex ends further than this from where it started, in the mesh's own units (the normalised frame)")
    ap.add_argument("--smooth_free_boundary", action="store_true", help="let the vertices on open edges move too (default: pinned)")
    ap.add_argument("--smooth_backend", default="host", choices=["host", "device"])
    ap.add_argument("--simplify_cell", type=float, default=None,
                    help="simplify the mesh to one vertex per cell of this size, in the mesh's own units (the normalised frame the "
                         "val forward extracts it in), by quadric vertex clustering: the last mesh step, after --clean_mesh")
    ap.add_argument("--simplify_backend", default="host", choices=["host", "device"])
    ap.add_argument("--deviation", action="store_true",
                    help="report how far --smooth_iters / --simplify_cell moved the surface: the vertex-sampled deviation between "
                         "the mesh before them and the mesh that is written, in the mesh's own units (surf_amd/mesh_distance.py)")
    ap.add_argument("--deviation_backend", default="host", choices=["host", "device"])
    ap.add_argument("--deviation_max_dist", type=float, default=None,
                    help="vertices without a face of the other mesh nearer than this count as `beyond` (default: the diagonal of "
                         "the two meshes' joint bounding box)")
    ap.add_argument("--texture", action="store_true",
                    help="also bake all photographs of the item into a texture atlas of the mesh that is written "
                         "(surf_amd/mesh_texture.py) -> scan<N>_textured.obj, .mtl and .png beside the PLY")
    ap.add_argument("--texture_texels", type=int, default=8, metavar="T", help="texels along a face's edge, 4..64: T (T+1) / 2 a face")
    ap.add_argument("--texture_depth_tol", type=float, default=None,
                    help="a texel further than this behind the mesh's own depth map is hidden from that photograph, in the written "
                         "mesh's own units (the world frame; default: 2 steps of the --mesh_resolution lattice)")
    ap.add_argument("--texture_min_cos", type=float, default=0.2, help="photographs that see a face more obliquely are not used for it")
    ap.add_argument("--texture_power", type=int, default=4, metavar="N", help="a photograph's weight is cos^N, 1..16")
    ap.add_argument("--texture_two_sided", action="store_true", help="photographs of a face's back side count too")
    ap.add_argument("--texture_backend", default="device", choices=["host", "device"])
    ap.add_argument("--downsample_density", type=float, default=0.2)
    ap.add_argument("--patch_size", type=float, default=60)
    ap.add_argument("--max_dist", type=float, default=20)
    ap.add_argument("--shuffle_seed", type=int, default=0, help="seed of the thinning shuffle of the evaluator (the reference's is unseeded)")
    ap.add_argument("--eval_device", default="cpu", choices=["cpu", "gpu"],
                    help="where the DTU evaluator samples, thins and measures (gpu: the HIP kernels, same numbers)")
    ap.add_argument("--reference_chamfer", type=float, default=None)
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
                             "sigma_r": getattr(args, "denoise_sigma_r", 0.35), "sigma_s": getattr(args, "denoise_sigma_s", None),
                             "pin_boundary": not getattr(args, "denoise_free_boundary", False),
                             "max_move": getattr(args, "denoise_max_move", None)})
    except ValueError as e:
        raise SystemExit(f"dtu_chamfer: {e}")


def texture_params(args, voxel):
    """The --texture_* flags as mesh_texture's argument dict, or None without --texture (a Namespace built by hand may lack them).
    voxel: the world-frame step of the extraction lattice, of which the default depth tolerance is two."""
    if not getattr(args, "texture", False):
        return None
    from surf_amd.mesh_texture import check_params
    tol = getattr(args, "texture_depth_tol", None)
    try:
        return check_params({"texels_per_edge": getattr(args, "texture_texels", 8), "depth_tol": 2.0 * voxel if tol is None else tol,
                             "min_cos": getattr(args, "texture_min_cos", 0.2), "power": getattr(args, "texture_power", 4),
                             "two_sided": getattr(args, "texture_two_sided", False)})
    except ValueError as e:
        raise SystemExit(f"dtu_chamfer: {e}")


def run(args, state=None):
    """Returns the JSON record.  state (dict, tests): receives the live `model`, the loader's `item` and the final normalised-frame
    `vertices` / `triangles` of the (last) evaluation; with --texture also the world-frame `world_vertices`, `texture_views`, `uv`
    and `atlas`."""
    from surf_amd import conf as C
    from surf_amd import mesh_io, synthetic
    from surf_amd.datasets import get_loader
    from surf_amd.evaluation import clean_dtu
    from surf_amd.evaluation import clean_mesh as CM
    from surf_amd.mesh_simplify import simplify_step
    from surf_amd.mesh_smooth import check_params, smooth_step
    from surf_amd.evaluation import dtu_eval
    from surf_amd.surf import SuRF

    dev = torch.device(args.device)
    protocol = args.clean_protocol if args.clean_mesh else None
    if protocol == "dtu_test" and args.dtu_test_dir is None:
        raise SystemExit("dtu_chamfer: --clean_protocol dtu_test needs --dtu_test_dir")
    smooth = None
    if getattr(args, "smooth_iters", None) is not None:      # a Namespace built by hand may lack the flags
        try:
            smooth = check_params({"iterations": args.smooth_iters, "lam": args.smooth_lambda,
                                   "mu": None if args.smooth_laplacian else args.smooth_mu,
                                   "pin_boundary": not args.smooth_free_boundary, "max_move": args.smooth_max_move})
        except ValueError as e:
            raise SystemExit(f"dtu_chamfer: {e}")
    denoise = denoise_params(args)
    texture_on = bool(getattr(args, "texture", False))
    if texture_on:
        texture_params(args, 1.0)                        # a refused flag ends the run before the model is loaded
    deviation = bool(getattr(args, "deviation", False))
    if deviation and smooth is None and denoise is None and args.simplify_cell is None:
        raise SystemExit("dtu_chamfer: --deviation compares the mesh before and after --denoise_iters / --smooth_iters / "
                         "--simplify_cell: give one of them")
    cfg = C.parse_file(args.conf)
    dconf = cfg["val_dataset"]
    if args.data_dir is not None:
        dconf["data_dir"] = args.data_dir
    dconf["scene"] = [f"scan{args.scan}"]
    if args.ref_view is not None:
        dconf["ref_view"] = [args.ref_view]
    mconf = cfg["model"]
    for key in ("down_rule", "kernel_order", "transposed_pairing"):
        if getattr(args, key) is not None:
            mconf["reg_network"][key] = getattr(args, key)
    if args.sdf_precision is not None:
        mconf["implicit_surface"]["render"]["sdf_precision"] = args.sdf_precision
    if args.mesh_extraction:
        mconf["implicit_surface"]["render"]["mesh_extraction"] = args.mesh_extraction

    t0 = time.perf_counter()
    loader, _, dataset = get_loader(dconf, "val", False, num_workers=0)
    if len(dataset) < 1:
        raise SystemExit(f"dtu_chamfer: no validation item for scan{args.scan} under {dconf['data_dir']}")
    item = next(iter(loader))
    inputs = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in item.items()}              # runner.py's tocuda
    inputs["mesh_resolution"] = args.mesh_resolution
    if args.vertex_colors:
        inputs["keep_scene"] = True              # the val forward's scene, for the attributes of the (cleaned) vertex set

    torch.manual_seed(0)
    model = SuRF(mconf)
    missing = unexpected = None
    if args.ckpt is not None:
        ckpt = torch.load(args.ckpt, map_location="cpu")
        res = model.load_state_dict(ckpt["model"] if "model" in ckpt else ckpt, strict=True)        # runner.py:79
        missing, unexpected = list(res.missing_keys), list(res.unexpected_keys)
    model = model.to(dev).eval()
    if args.logit_override == "sphere":
        model.logit_override = synthetic.sphere_logit
    t_load = time.perf_counter() - t0

    def evaluate(tag=""):
        """One val forward + mesh + DTU evaluation of `model` under its current torchsparse conventions."""
        t0 = time.perf_counter()
        with torch.no_grad():
            out = model("val", inputs, cos_anneal_ratio=1.0)                                      # runner.py:216
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t_val = time.perf_counter() - t0
        conv = model.reg_network.conventions()
        v, t = np.asarray(out["vertices"]), np.asarray(out["triangles"])
        if len(t) == 0:
            if tag:                      # a sweep candidate that scrambles the checkpoint may well produce no surface at all
                return {"scan": args.scan, "chamfer": None, "error": "empty mesh", **conv}
            raise SystemExit("dtu_chamfer: the SDF lattice has no zero crossing inside the bounding box (empty mesh)")
        t0 = time.perf_counter()
        if protocol == "runner":
            v, t = CM.clean_mesh(v, t, item["masks"], item["intrs"], item["c2ws"], device=dev.type, backend=args.clean_backend)
        t_clean = time.perf_counter() - t0
        mesh_path = os.path.join(args.out_dir, "meshes", "final" + tag, f"scan{args.scan}.ply")
        os.makedirs(os.path.dirname(mesh_path), exist_ok=True)
        if state is not None:
            state.update(model=model, item=item, vertices=v, triangles=t)
        attrs, t_attr, simplified, smoothed, denoised = {}, None, None, None, None

        def denoise_now(v, normals):                 # in the normalised frame, before the smoothing and the simplification
            from surf_amd.mesh_denoise import denoise_step
            try:
                return denoise_step(v, t, denoise, normals=normals, backend=getattr(args, "denoise_backend", "host"), device=dev)
            except ValueError as e:
                raise SystemExit(f"dtu_chamfer: {e}")

        if args.vertex_colors:                   # on the final vertex set: after clean_mesh, before scale_mat
            t0 = time.perf_counter()
            attrs = model.vertex_attributes(v)
            t_attr = time.perf_counter() - t0
        if protocol == "dtu_test":               # the protocol's order: world-frame mesh first, then its cleaner, then the file
            scale_mat = item["scale_mat"].detach().cpu().numpy()
            vw = mesh_io.transform_vertices(v, scale_mat)
            t0 = time.perf_counter()
            vw, t, kept = clean_dtu.clean_dtu_scan(vw, t, args.dtu_test_dir, args.scan, view_set=args.clean_set,
                                                   backend=args.clean_backend, device=dev.type, return_index=True)
            t_clean = time.perf_counter() - t0
            v = np.asarray(v)[kept]
            normals, colors = attrs.get("normals"), attrs.get("colors")
            normals, colors = (None if normals is None else normals[kept]), (None if colors is None else colors[kept])
            before = (v, t)                      # mesh A of --deviation: after the cleaner, before the steps it measures
            if denoise is not None:
                v, normals, denoised = denoise_now(v, normals)
                vw = mesh_io.transform_vertices(v, scale_mat)
            if smooth is not None:               # in the normalised frame, like the simplification; the world-frame vertices follow
                v, normals, smoothed = smooth_step(v, t, smooth, normals=normals, backend=args.smooth_backend, device=dev)
                vw = mesh_io.transform_vertices(v, scale_mat)
            if args.simplify_cell is not None:   # the last mesh step, in the normalised frame; the world-frame vertices follow it
                v, t, normals, colors, simplified = simplify_step(v, t, args.simplify_cell, normals, colors, args.simplify_backend, dev)
                vw = mesh_io.transform_vertices(v, scale_mat)
            if state is not None:
                state.update(vertices=v, triangles=t)
            if normals is not None:
                normals = mesh_io.transform_normals(normals, scale_mat)
            mesh_io.write_ply(mesh_path, vw, t, normals=normals, colors=colors)
            written = vw
        else:
            normals, colors = attrs.get("normals"), attrs.get("colors")
            before = (v, t)
            if denoise is not None:
                v, normals, denoised = denoise_now(v, normals)
                if state is not None:
                    state.update(vertices=v, triangles=t)
            if smooth is not None:
                v, normals, smoothed = smooth_step(v, t, smooth, normals=normals, backend=args.smooth_backend, device=dev)
                if state is not None:
                    state.update(vertices=v, triangles=t)
            if args.simplify_cell is not None:
                v, t, normals, colors, simplified = simplify_step(v, t, args.simplify_cell, normals, colors, args.simplify_backend, dev)
                if state is not None:
                    state.update(vertices=v, triangles=t)
            written = mesh_io.export_mesh(mesh_path, v, t, item["scale_mat"], normals=normals, colors=colors)   # runner.py:236-240
        if len(t) == 0:
            raise SystemExit(f"dtu_chamfer: --simplify_cell {args.simplify_cell} leaves no face (the cell swallows the mesh)")
        textured = None
        if texture_on:                           # on the world-frame mesh that was written, from every photograph of the item
            from surf_amd.fusion import similarity_scale
            from surf_amd.mesh_texture import texture_step, view_from_item
            world_step = similarity_scale(item["scale_mat"].detach().cpu().numpy().reshape(4, 4)) * 2.0 / (args.mesh_resolution - 1)
            tviews = [view_from_item(item, k) for k in range(int(item["intrs"].reshape(-1, 4, 4).shape[0]))]
            try:
                uv, atlas, textured = texture_step(written, t, tviews, texture_params(args, world_step),
                                                   backend=getattr(args, "texture_backend", "device"), device=dev,
                                                   vertex_colors=colors)
            except ValueError as e:
                raise SystemExit(f"dtu_chamfer: {e}")
            textured["files"] = list(mesh_io.write_obj(os.path.splitext(mesh_path)[0] + "_textured.obj", written, t, uv, atlas))
            if state is not None:
                state.update(world_vertices=written, texture_views=tviews, uv=uv, atlas=atlas)
        deviated = None
        if deviation:                            # mesh B is the mesh that is written, both in the normalised frame
            from surf_amd.mesh_distance import deviation_step
            try:
                deviated = deviation_step(before[0], before[1], v, t, getattr(args, "deviation_max_dist", None),
                                          backend=getattr(args, "deviation_backend", "host"), device=dev)
            except ValueError as e:
                raise SystemExit(f"dtu_chamfer: {e}")
        t0 = time.perf_counter()
        d2s, s2d, overall = dtu_eval.evaluate_scan(mesh_path, args.eval_dir, args.scan, patch_size=args.patch_size,
                                                   max_dist=args.max_dist, downsample_density=args.downsample_density,
                                                   rng=np.random.default_rng(args.shuffle_seed), device=args.eval_device)
        t_eval = time.perf_counter() - t0
        return {"scan": args.scan, "d2s": d2s, "s2d": s2d, "chamfer": overall, "reference_chamfer": args.reference_chamfer,
                "delta": None if args.reference_chamfer is None else overall - args.reference_chamfer,
                "mesh": mesh_path, "vertices": int(len(v)), "triangles": int(len(t)), "mesh_resolution": args.mesh_resolution,
                "views": int(item["imgs"].shape[0]), "render_hw": [int(x) for x in out["img_fine"].shape[:2]],
                **conv, "sdf_precision": model.implicit_surface.sdf_precision,
                "checkpoint": args.ckpt, "missing_keys": missing, "unexpected_keys": unexpected, "cleaned": bool(args.clean_mesh),
                "clean_backend": args.clean_backend if args.clean_mesh else None, "clean_protocol": protocol,
                "seconds": {"load": t_load, "val_forward": t_val, "clean": t_clean, "evaluate": t_eval,
                            **({} if t_attr is None else {"vertex_attributes": t_attr})},
                **({} if denoised is None else {"denoise": denoised}), **({} if smoothed is None else {"smooth": smoothed}), **({} if simplified is None else {"simplify": simplified}),
                **({} if deviated is None else {"deviation": deviated}), **({} if textured is None else {"texture": textured})}

    if not args.sweep:
        rec = evaluate()
        with open(os.path.join(args.out_dir, f"chamfer_scan{args.scan}.json"), "w") as f:
            json.dump(rec, f)
        return rec
    # ---- the 3 x 2 x 2 grid of torchsparse conventions on the one loaded model ----
    grid = []
    for rule in ("pad0", "dilate", "floor"):
        for order in ("xfast", "zfast"):
            for pairing in ("same", "mirrored"):
                model.reg_network.set_conventions(rule, order, pairing)
                r = evaluate(f"_{rule}_{order}_{pairing}")
                grid.append(r)
                print(json.dumps({k: r.get(k) for k in ("down_rule", "kernel_order", "transposed_pairing", "chamfer", "d2s", "s2d",
                                                        "delta", "triangles", "error")}), flush=True)
    ok = [r for r in grid if r["chamfer"] is not None]
    if not ok:
        raise SystemExit("dtu_chamfer --sweep: every combination produced an empty mesh")
    target = args.reference_chamfer
    best = min(ok, key=(lambda r: abs(r["chamfer"] - target)) if target is not None else (lambda r: r["chamfer"]))
    rec = {"scan": args.scan, "sweep": [{k: r.get(k) for k in ("down_rule", "kernel_order", "transposed_pairing", "chamfer", "delta",
                                                              "error")} for r in grid],
           "selected_by": "closest to --reference_chamfer" if target is not None else "lowest Chamfer (no --reference_chamfer given)",
           "best": best, "reference_chamfer": target,
           "within_0.01_of_reference": None if target is None else [
               {k: r[k] for k in ("down_rule", "kernel_order", "transposed_pairing", "chamfer")} for r in ok
               if abs(r["chamfer"] - target) <= 0.01]}
    with open(os.path.join(args.out_dir, f"chamfer_sweep_scan{args.scan}.json"), "w") as f:
        json.dump(rec, f)
    return rec


def main(argv=None):
    print(json.dumps(run(parse_args(argv))))


if __name__ == "__main__":
    main()
