"""Rig-constrained local BA against the host-decided free loop on the benchmark's local window (7 stereo keyframes =
14 cameras, ~15k landmarks): ms per LM iteration of Context.bundle_adjust_rig and of Context.bundle_adjust under
"ba_no_fused", median of 20 solves, with the reduced-system sizes and the device stage times of a separate profiled run.
One variant per process (argv[1] = rig | free | rig_ext): run three processes per variant, alternating.  One JSON line.
rig_ext: Context.bundle_adjust_rig_ext on the same window with extrinsic block 1 free (one more 6-dof slot and the border).

argv[1] = map_dense | map | map_free: the benchmark's 500-keyframe loop (the scene of bench.py's global-BA leg: 500
bodies, 1000 cameras, ~100 k landmark candidates; argv[2] = keyframes) through (a) Context.bundle_adjust_rig, the dense rig
route, (b) Context.global_bundle_adjust_rig, the pair gather into band storage, (c) the free global solver on the
expanded problem.  ms per LM iteration = the marginal wall time between solves of 3 and 9 iterations (medians of three:
the host set-up cancels), the layout of the reduced system and the device stage times of a profiled solve."""
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
if variant.startswith("map"):
    n_kf = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    d = synth.ba_problem(5, n_kf=n_kf, n_lms=100000 * n_kf // 500, loop_radius=200.0 * n_kf / 500.0, max_range=15.0)
    n_cams = len(d["poses"])
    T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], synth.T_0_1])
    bodies = np.asarray(d["poses"]).reshape(-1, 7)[0::2]
    fixed = np.asarray(d["cam_fixed"])[0::2]
    if variant == "map_free":
        ba_dist = importlib.import_module("visual_slam_amd.ba_dist")

        def solve(max_iters):
            return ba_dist.bundle_adjust_distributed(vsl, ctx, vsl.BaArrays.from_dict(d), max_iters=max_iters)
        n_unknowns = 6 * int((np.asarray(d["cam_fixed"]) == 0).sum())
    else:
        call = ctx.bundle_adjust_rig if variant == "map_dense" else ctx.global_bundle_adjust_rig

        def solve(max_iters):
            return call(vsl.BaArrays.from_dict(d), vsl.RigArrays(bodies, fixed, np.arange(n_cams) // 2, T_b_c), max_iters=max_iters)
        n_unknowns = 6 * int((fixed == 0).sum())
    solve(2)
    layout = ctx.last_ba_layout() if variant != "map_dense" else (n_unknowns * n_unknowns, 0, n_unknowns)
    wall = {3: [], 9: []}
    its = {}
    for _ in range(3):
        for k in (3, 9):
            ctx.synchronize()
            t0 = time.perf_counter()
            s = solve(k)
            ctx.synchronize()
            wall[k].append(1e3 * (time.perf_counter() - t0))
            its[k] = s.iterations
    ctx.set_profiling(1)
    sp = solve(9)
    ctx.set_profiling(0)
    m3, m9 = statistics.median(wall[3]), statistics.median(wall[9])
    print(json.dumps({"variant": variant, "keyframes": n_kf, "reduced_system_unknowns": n_unknowns, "cameras": n_cams,
                      "landmarks": len(d["points"]), "observations": len(d["obs_cam"]), "s_doubles": layout[0], "layout": layout[1],
                      "bandwidth": layout[2], "iterations": [its[3], its[9]], "wall_ms_3_iterations": wall[3], "wall_ms_9_iterations": wall[9],
                      "ms_per_iteration": (m9 - m3) / max(its[9] - its[3], 1),
                      "device_ms_per_iteration": {k: getattr(sp, k + "_ms", 0.0) / max(sp.iterations, 1) for k in ("linearize", "schur", "solve")},
                      "final_cost_9": s.final_cost}))
    ctx.close()
    sys.exit(0)
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
elif variant == "rig_ext":
    bodies = np.asarray(d["poses"]).reshape(-1, 7)[0::2]
    fixed = np.asarray(d["cam_fixed"])[0::2]

    def solve(max_iters):
        arr = vsl.BaArrays.from_dict(d)
        rig = vsl.RigArrays(bodies, fixed, np.arange(n_cams) // 2, T_b_c)
        return ctx.bundle_adjust_rig_ext(arr, rig, T_b_c.copy(), ext_free=(0, 1), max_iters=max_iters)
    n_unknowns = 6 * (int((fixed == 0).sum()) + 1)
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
