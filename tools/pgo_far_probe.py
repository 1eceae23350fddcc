#!/usr/bin/env python3
"""Dense route against the far-edge route of the pose-graph solver.

Graphs: keyframe chains of tests/pgo_ref.loop_graph (window 3, node 0 fixed) with 1 / 8 / 32 extra long edges, 500 / 1000 /
2000 keyframes.  Per graph and route (switch "pgo_far_edges" off / on at the same commit; off is the yardstick): one
warm-up solve, then --repeats timed solves of the same problem from the same start; median and min / max of the whole
call's wall time and of that time per LM iteration (the pose-graph summary carries no timer of its own), the LM counts, the final cost, and the bytes of the
solve's matrix storage (the two n x n arrays of the dense route; the two band arrays, the right-hand-side blocks, the
inverted diagonal blocks and C of the far-edge route -- computed from the sizes, not read back from the allocator).

    python tools/pgo_far_probe.py [--out profiles/r16_pgo_far_probe.json] [--sizes 500,1000,2000] [--far 1,8,32] [--repeats 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as entry  # noqa: E402
import pgo_far_ref as fr  # noqa: E402
import pgo_ref as pg  # noqa: E402


def storage_bytes(n, info):
    if not info["taken"]:
        return 2 * 8 * n * n
    bw, cols = info["half_bandwidth"], info["columns"]
    band = n * (bw + 33) + 64
    nblk = (cols + 15) // 16
    return 8 * (2 * band + nblk * n * 16 + ((n + 31) // 32) * 1024 + (cols - 1) ** 2 + 3 * n)


def run(ctx, g0, far, iters, repeats):
    ctx.set_diagnostic("pgo_far_edges", int(far))
    try:
        rows = []
        for rep in range(repeats + 1):  # the first solve is the warm-up
            g = g0.copy()
            t0 = time.perf_counter()
            s = ctx.pose_graph_optimize(g, True, 1.0, iters)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                rows.append((wall, wall / max(s.iterations, 1)))
        info = ctx.last_pgo_far()
    finally:
        ctx.set_diagnostic("pgo_far_edges", 0)
    wall, per_it = [r[0] for r in rows], [r[1] for r in rows]
    return dict(route=info, lm_iterations=s.iterations, termination=s.termination, successful_steps=s.successful_steps,
                initial_cost=s.initial_cost, final_cost=s.final_cost, call_ms_median=statistics.median(wall), call_ms_min=min(wall),
                call_ms_max=max(wall), ms_per_lm_iteration_median=statistics.median(per_it), ms_per_lm_iteration_min=min(per_it),
                ms_per_lm_iteration_max=max(per_it), matrix_storage_bytes=storage_bytes(g0.n_unknowns(), info), repeats=repeats), g.poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r16_pgo_far_probe.json"))
    ap.add_argument("--sizes", default="500,1000,2000")
    ap.add_argument("--far", default="1,8,32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    vsl = entry.load_package()
    ctx = vsl.Context(0)
    out = dict(tool="tools/pgo_far_probe.py", device="MI355X (gfx950)", max_lm_iterations=args.iters, window=3, graphs=[])
    for n_kf in map(int, args.sizes.split(",")):
        for k in map(int, args.far.split(",")):
            g = pg.loop_graph(n_kf, window=3, loop=False, fixed=[0], extra=fr._spread_extra(n_kf, k, 100 + k), noise=fr.NOISE,
                              seed=n_kf + k, name="chain%d_w3_far%d" % (n_kf, k))
            row = dict(graph=g.name, keyframes=n_kf, unknowns=g.n_unknowns(), edges=len(g.edge_a), far_edges=k)
            row["off"], p_off = run(ctx, g, False, args.iters, args.repeats)
            row["on"], p_on = run(ctx, g, True, args.iters, args.repeats)
            row["final_cost_rel_gap"] = abs(row["on"]["final_cost"] - row["off"]["final_cost"]) / max(row["off"]["final_cost"], 1e-12)
            row["poses_max_abs_gap"] = float(np.abs(p_on - p_off).max())
            row["on_below_off_beyond_ranges"] = bool(row["on"]["call_ms_max"] < row["off"]["call_ms_min"])
            print(json.dumps(row), flush=True)
            out["graphs"].append(row)
    ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
