#!/usr/bin/env python3
"""Times the mesh deviation (surf_amd/mesh_distance.py; csrc/mesh_distance.hip) on the GPU and writes profiles/mesh_distance.txt:

    python scripts/time_mesh_distance.py [--res 512] [--iters 3] [--host_queries 20000] [--out profiles/mesh_distance.txt] [--no_host]

Mesh A is the marching-cubes mesh of scripts/time_simplify.py's fused sphere at --res^3.  Two workloads, both directions each:
A against its simplification at 4 lattice steps (mesh_simplify, device), and A against its smoothing by 10 Taubin pairs
(mesh_smooth, device).  A direction queries the vertices that the one mesh's faces name against the other mesh.  Per direction:
  * ops.point_to_mesh stage by stage (pairs: the reads, the pair count and emit; sort: the sort by cell, the cell starts, the
    record gather and the query sort; query: the query kernel): device events around each stage over --iters repetitions after 2
    warm-up ones, meshes resident on the device; total = wall clock of a repetition with its host reads;
  * pairs per face of the table, and the query kernel's compulsory bytes (per query 12 + 8 in and 8 + 8 + 24 out, per pair one
    48-byte record) with the time those bytes take at the 6.29 TB/s this GPU copies at; `bound/measured` is that ratio against
    the query stage, reported, not a pass mark (the kernel is arithmetic, not a copy);
  * the point-to-point floor: ops.nearest_capped_index of the same queries against the vertices the other mesh's faces name
    (fp64), table build and query, device events over the same repetitions;
  * the numpy mirror (point_to_mesh_host) on the first --host_queries queries against the whole mesh, one repetition, and from
    the same run the faces evaluated per query (the pairs the walk visits; the device walk visits the same shells).
Measurements, not thresholds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_TBS = 6.29
STAGES = ("pairs", "sort", "query")


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--host_queries", type=int, default=20000)
    ap.add_argument("--no_host", action="store_true", help="skip the numpy mirror")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mesh_distance.txt"))
    args = ap.parse_args(argv)
    from surf_amd import ops
    from surf_amd.mesh_distance import joint_diagonal, point_to_mesh_host
    from surf_amd.mesh_simplify import simplify_mesh
    from surf_amd.mesh_smooth import smooth_mesh
    from time_simplify import fused_mesh
    assert torch.cuda.is_available(), "time_mesh_distance.py measures on the GPU"
    dev = torch.device("cuda:0")
    va, fa = fused_mesh(args.res, dev)[:2]
    va, fa = np.ascontiguousarray(va, np.float32), np.ascontiguousarray(fa, np.int32)
    cell = 4 * 2.0 / (args.res - 1)
    sv, sf = simplify_mesh(va, fa, cell, backend="device", device=dev)[:2]
    tv = smooth_mesh(va, fa, iterations=10, backend="device", device=dev)[0]
    workloads = [(f"simplified at 4 lattice steps ({cell:.5f})", np.ascontiguousarray(sv, np.float32), np.ascontiguousarray(sf, np.int32)),
                 ("smoothed by 10 Taubin pairs", np.ascontiguousarray(tv, np.float32), fa)]
    lines = [f"# scripts/time_mesh_distance.py: {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})",
             f"# mesh A: fused sphere {args.res}^3, {len(va)} vertices, {len(fa)} faces",
             f"# device ms: events per stage ({' | '.join(STAGES)}) of ops.point_to_mesh over {args.iters} repetitions after 2 warm-up "
             "ones; total = wall clock with the host reads, meshes resident on the device",
             f"# bytes = k (12 + 8 + 8 + 8 + 24) + 48 pairs of the query kernel; bound = bytes at {COPY_TBS} TB/s (the measured copy "
             "rate); bound/measured against the query stage.  Reported, not a pass mark.",
             "# floor ms: ops.nearest_capped_index of the same queries against the other mesh's named vertices (table build + query)",
             f"# host ms: point_to_mesh_host of the first {args.host_queries} queries against the whole mesh, one repetition (numpy, "
             "one thread); evaluated = (cell, face) pairs its walk visits per query"]

    def timed(fn):
        """Mean device ms (events) and mean wall ms of fn over the repetitions after two warm-up ones."""
        ev_ms, wall = 0.0, []
        for it in range(2 + args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                wall.append(1e3 * (time.perf_counter() - t0))
                ev_ms += e0.elapsed_time(e1) / args.iters
        return ev_ms, float(np.mean(wall))

    for name, vb, fb in workloads:
        max_dist = joint_diagonal(va, vb)
        lines.append(f"A against A {name}: {len(vb)} vertices, {len(fb)} faces, max_dist {max_dist:.4f}")
        for direction, (qv, qf), (mv, mf) in (("forward  (A's vertices -> B)", (va, fa), (vb, fb)),
                                              ("backward (B's vertices -> A)", (vb, fb), (va, fa))):
            q32 = qv[np.unique(qf)]
            k, m = len(q32), len(mf)
            dq, dv, df = torch.from_numpy(q32).to(dev), torch.from_numpy(mv).to(dev), torch.from_numpy(mf).to(dev)
            sums, totals, stats = dict.fromkeys(STAGES, 0.0), [], {}
            for it in range(2 + args.iters):
                st = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = ops.point_to_mesh(dq, dv, df, max_dist, stages=st, stats=stats)
                torch.cuda.synchronize()
                if it >= 2:
                    totals.append(1e3 * (time.perf_counter() - t0))
                    for sname, a, b in st:
                        sums[sname] += a.elapsed_time(b) / args.iters
            dist = out[0]
            found = torch.isfinite(dist)
            d_max, d_mean = float(dist[found].max()), float(dist[found].mean())
            del out
            nbytes = k * (12 + 8 + 8 + 8 + 24) + 48 * stats["pairs"]
            bound_ms = nbytes / (COPY_TBS * 1e12) * 1e3
            ref = torch.from_numpy(mv[np.unique(mf)].astype(np.float64)).to(dev)
            q64 = dq.double()
            floor_ms, _ = timed(lambda: ops.nearest_capped_index(q64, ref, max_dist))
            table = ops.NearestTable(ref)
            floor_query_ms, _ = timed(lambda: table.query(q64, max_dist))
            del table, ref, q64
            lines += [f"  {direction}: {k} queries, {m} faces, cell {stats['cell']:.5f}, table {stats['dims']}, {stats['pairs']} pairs "
                      f"({stats['pairs'] / m:.2f} per face), max {d_max:.5f}, mean {d_mean:.6f}",
                      f"    device  {' | '.join(f'{sums[x]:8.3f}' for x in STAGES)}   total {np.mean(totals):9.3f}",
                      f"    query   bytes {nbytes / 1e6:9.1f} MB   bound {bound_ms:7.4f} ms   bound/measured {bound_ms / sums['query']:6.3f}   "
                      f"{k / sums['query'] / 1e3:8.2f} M queries/s",
                      f"    floor   nearest_capped_index {floor_ms:8.3f} (query alone {floor_query_ms:8.3f})"]
            rows = 4
            if not args.no_host:
                hk = min(k, args.host_queries)
                hstats = {}
                t0 = time.perf_counter()
                hd = point_to_mesh_host(q32[:hk], mv, mf, max_dist, stats=hstats)[0]
                h_ms = 1e3 * (time.perf_counter() - t0)
                same = bool(np.array_equal(hd.view(np.uint64), dist[:hk].cpu().numpy().view(np.uint64))) if hk == k else \
                    bool(np.array_equal(hd.view(np.uint64), ops.point_to_mesh(dq[:hk].contiguous(), dv, df, max_dist)[0].cpu().numpy().view(np.uint64)))
                lines.append(f"    host    {h_ms:10.1f} ms for {hk} queries ({h_ms / hk * 1e3:8.1f} us per query), evaluated "
                             f"{hstats['evaluated'] / hk:8.1f} pairs per query, {hstats['pairs'] / m:.2f} pairs per face; "
                             f"distance bits equal to the device's: {same}")
                rows = 5
            del dq, dv, df, dist
            for line in lines[-rows:]:
                print(line, flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
