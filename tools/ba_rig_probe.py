"""Rig-constrained local BA against the host-decided free loop on the benchmark's local window (7 stereo keyframes =
14 cameras, ~15k landmarks): ms per LM iteration of Context.bundle_adjust_rig and of Context.bundle_adjust under
"ba_no_fused", median of 20 solves, with the reduced-system sizes and the device stage times of a separate profiled run.
One variant per process (argv[1] = rig | free): run three processes per variant, alternating.  One JSON line."""
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as entry  # noqa: E402

variant = sys.argv[1] if len(sys.argv) > 1 else "rig"
vsl = entry.load_package()
synth = importlib.import_module("visual_slam_amd.synth")
ctx = vsl.Context(0)
d = synth.ba_problem(4, n_kf=7, n_lms=20000)
n_cams = len(d["poses"])
T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], synth.T_0_1])   # the generator's own stereo extrinsic
if variant == "rig":
    # the same observations; the body of keyframe k is its left camera (2 k), the right one at the generator's T_0_1
    bodies = np.asarray(d["poses"]).reshape(-1, 7)[0::2]
    fixed = np.asarray(d["cam_fixed"])[0::2]

    def solve(max_iters):
        arr = vsl.BaArrays.from_dict(d)
        rig = vsl.RigArrays(bodies, fixed, np.arange(n_cams) // 2, T_b_c)
        return ctx.bundle_adjust_rig(arr, rig, max_iters=max_iters)
    n_unknowns = 6 * int((fixed == 0).sum())
else:
    ctx.set_diagnostic("ba_no_fused", 1)

    def solve(max_iters):
        return ctx.bundle_adjust(vsl.BaArrays.from_dict(d), max_iters=max_iters)
    n_unknowns = 6 * int((np.asarray(d["cam_fixed"]) == 0).sum())
solve(2)
per_iter, iters = [], 0
for _ in range(20):
    ctx.synchronize()
    t0 = time.perf_counter()
    s = solve(20)
    per_iter.append(1e3 * (time.perf_counter() - t0) / max(s.iterations, 1))
    iters = s.iterations
ctx.set_profiling(1)
sp = solve(20)
ctx.set_profiling(0)
print(json.dumps({"variant": variant, "reduced_system_unknowns": n_unknowns, "cameras": n_cams, "landmarks": len(d["points"]),
                  "observations": len(d["obs_cam"]), "iterations": iters, "ms_per_iteration_median": statistics.median(per_iter),
                  "ms_per_iteration_min": min(per_iter), "ms_per_iteration_max": max(per_iter),
                  "device_ms_per_iteration": {"linearize": sp.linearize_ms / max(sp.iterations, 1), "schur": sp.schur_ms / max(sp.iterations, 1),
                                              "solve": sp.solve_ms / max(sp.iterations, 1)},
                  "final_cost": s.final_cost}))
ctx.close()
