#!/usr/bin/env python3
"""Direct against iterative Schur on maps with and without a narrow band.

Maps: inward-looking circles of 100 / 300 / 600 keyframes (tests/ba_wide_ref.py; every camera pair covisible, the direct
route stores S dense; at most --max-obs observations of a landmark are kept so that every landmark fits a run of the
recompute form) and the 1000-camera loop of BASELINE.json configs[4] (cyclic band on the direct route).
Per map and route (switch "ba_iterative_schur" off / on, forcing term 0.1): one warm-up solve, then --repeats timed solves
of the same problem from the same start; median and min / max of the solve's wall time and of ms per LM iteration, LM
iterations, PCG iterations per LM iteration, final cost, doubles and bytes of S.  The off column on the same commit is the
baseline.

    python tools/ba_pcg_probe.py [--out profiles/r13_ba_pcg_probe.json] [--maps 100,300,600,loop] [--repeats 5]
"""
import argparse
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
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as entry  # noqa: E402
import ba_wide_ref as W  # noqa: E402


def arrays(d):
    a = SimpleNamespace(cam_model=d["cam_model"])
    for k in ("poses", "cam_fixed", "cam_intr", "intr", "points", "obs_cam", "obs_lm", "obs_uv"):
        setattr(a, k, np.ascontiguousarray(d[k]).copy())
    return a


def run(ctx, d, iterative, max_iters, repeats):
    ctx.set_diagnostic("ba_iterative_schur", int(iterative))
    try:
        rows = []
        for rep in range(repeats + 1):  # the first solve is the warm-up
            a = arrays(d)
            t0 = time.perf_counter()
            s = ctx.bundle_adjust(a, max_iters=max_iters)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                rows.append((wall, s.total_ms / max(s.iterations, 1)))
        elems, form, bw = ctx.last_ba_layout()
        solves, total, _, rel = ctx.last_ba_pcg()
    finally:
        ctx.set_diagnostic("ba_iterative_schur", 0)
    wall, per_it = [r[0] for r in rows], [r[1] for r in rows]
    return dict(layout=form, s_doubles=elems, s_bytes=8 * elems, bandwidth=bw, lm_iterations=s.iterations, termination=s.termination,
                successful_steps=s.successful_steps, initial_cost=s.initial_cost, final_cost=s.final_cost,
                solve_ms_median=statistics.median(wall), solve_ms_min=min(wall), solve_ms_max=max(wall),
                ms_per_lm_iteration_median=statistics.median(per_it), ms_per_lm_iteration_min=min(per_it),
                ms_per_lm_iteration_max=max(per_it), pcg_solves=solves, pcg_iterations=total,
                pcg_iterations_per_lm_iteration=(total / solves if solves else 0.0), pcg_rel_residual_last=rel, repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_ba_pcg_probe.json"))
    ap.add_argument("--maps", default="100,300,600,loop")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max-obs", type=int, default=300)
    args = ap.parse_args()
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    ctx = vsl.Context(0)
    out = dict(tool="tools/ba_pcg_probe.py", device="MI355X (gfx950)", max_lm_iterations=args.iters, forcing_term=0.1, maps=[])
    for name in args.maps.split(","):
        if name == "loop":
            d = synth.ba_problem(5, n_kf=500, n_lms=100000, loop_radius=200.0, max_range=15.0)
            label = "loop of 500 keyframes (configs[4])"
        else:
            n_kf = int(name)
            d = W.wide(synth, 100 + n_kf, n_kf, {100: 3000, 300: 4000, 600: 5000}.get(n_kf, 4000), max_obs_per_lm=args.max_obs)
            label = "inward circle of %d keyframes" % n_kf
        row = dict(map=label, cameras=len(d["poses"]), free_cameras=int((d["cam_fixed"] == 0).sum()), landmarks=len(d["points"]),
                   observations=len(d["obs_cam"]))
        row["direct"] = run(ctx, d, False, args.iters, args.repeats)
        row["iterative"] = run(ctx, d, True, args.iters, args.repeats)
        row["final_cost_rel_gap"] = abs(row["iterative"]["final_cost"] - row["direct"]["final_cost"]) / row["direct"]["final_cost"]
        print(json.dumps(row), flush=True)
        out["maps"].append(row)
    ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
