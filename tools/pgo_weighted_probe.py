#!/usr/bin/env python3
"""Cost of per-edge information matrices in the pose-graph solve.

The 500-keyframe ring of the bench's pose-graph leg (synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6)).
Per variant one warm-up solve, then --repeats timed solves of the same problem from the same start; median and min / max
of the wall time per Levenberg-Marquardt iteration:
  parent_unweighted   vsl_pose_graph_optimize of the library given by --parent (the parent commit's build), if given
  unweighted          vsl_pose_graph_optimize of this tree
  weighted            vsl_pose_graph_optimize_w with random SPD information matrices (condition number up to 1e6)
  whitening           the one-off set-up cost of the weights: a weighted call with max_num_iterations = 0 minus an
                      unweighted one (upload of Omega, pgo_edge_whiten_kernel, read-back of the verdict)

    python tools/pgo_weighted_probe.py [--out profiles/r14_pgo_weighted_probe.json] [--parent PATH/libvslam_hip.so] [--repeats 3]
"""
import argparse
import ctypes as C
import importlib
import json
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as entry  # noqa: E402


def random_spd(E, seed=1):
    rng = np.random.default_rng(seed)
    out = np.zeros((E, 6, 6))
    for e in range(E):
        c = rng.uniform(0, 6)
        lam = 10.0 ** np.concatenate([[-c / 2, c / 2], rng.uniform(-c / 2, c / 2, 4)])
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        W = (Q * lam) @ Q.T
        out[e] = (W + W.T) / 2
    return out


def timed(solve, repeats):
    rows = []
    for rep in range(repeats + 1):  # the first solve is the warm-up
        t0 = time.perf_counter()
        s = solve()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            rows.append((wall, wall / max(s.iterations, 1)))
    wall, per_it = [r[0] for r in rows], [r[1] for r in rows]
    return dict(lm_iterations=s.iterations, termination=s.termination, final_cost=s.final_cost, repeats=repeats,
                solve_ms_median=statistics.median(wall), solve_ms_min=min(wall), solve_ms_max=max(wall),
                ms_per_lm_iteration_median=statistics.median(per_it), ms_per_lm_iteration_min=min(per_it),
                ms_per_lm_iteration_max=max(per_it))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14_pgo_weighted_probe.json"))
    ap.add_argument("--parent", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    d = synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6)

    def graph():
        return SimpleNamespace(poses=np.ascontiguousarray(d["poses"], np.float64).copy(), node_fixed=np.ascontiguousarray(d["node_fixed"], np.uint8),
                               edge_a=np.ascontiguousarray(d["edge_a"], np.int32), edge_b=np.ascontiguousarray(d["edge_b"], np.int32),
                               edge_meas=np.ascontiguousarray(d["edge_meas"], np.float64))

    E = len(d["edge_a"])
    W = random_spd(E)
    ctx = vsl.Context(0)
    out = dict(tool="tools/pgo_weighted_probe.py", device="MI355X (gfx950)", graph="ring of 500 keyframes, window 6 (the bench's pose_graph leg)",
               nodes=len(d["poses"]), edges=E, max_lm_iterations=args.iters)
    if args.parent:
        # the parent's library beside this one in the same process: only its pose-graph solve is called
        P = C.CDLL(args.parent)
        P.vsl_ctx_create.restype = C.c_int
        h = C.c_void_p()
        assert P.vsl_ctx_create(0, C.byref(h)) == 0

        def parent_solve():
            g = graph()
            st, o, s = ctx._pgo_struct(g), ctx._ba_opts(True, 1.0, args.iters, 0), vsl.BaSummary()
            assert P.vsl_pose_graph_optimize(h, C.byref(st), C.byref(o), C.byref(s)) == 0
            return s

        out["parent_unweighted"] = timed(parent_solve, args.repeats)
        P.vsl_ctx_destroy(h)
    out["unweighted"] = timed(lambda: ctx.pose_graph_optimize(graph(), max_iters=args.iters), args.repeats)
    out["weighted"] = timed(lambda: ctx.pose_graph_optimize(graph(), max_iters=args.iters, edge_info=W), args.repeats)
    setup_u = timed(lambda: ctx.pose_graph_optimize(graph(), max_iters=0), args.repeats)
    setup_w = timed(lambda: ctx.pose_graph_optimize(graph(), max_iters=0, edge_info=W), args.repeats)
    out["whitening_ms"] = dict(median=setup_w["solve_ms_median"] - setup_u["solve_ms_median"], setup_unweighted_ms=setup_u["solve_ms_median"],
                               setup_weighted_ms=setup_w["solve_ms_median"])
    ctx.close()
    print(json.dumps(out), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
