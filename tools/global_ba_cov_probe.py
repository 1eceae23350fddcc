"""Timing probe of vsl_global_ba_covariance on the global-BA problem of bench.py (BASELINE
configs[4]: synth.ba_problem(5, n_kf=500, n_lms=100000, loop_radius=200): 1000 cameras, ~97 k landmarks), beside two
yardsticks.  Legs, each in a child process of its own under its own time limit; host wall time of the synchronous call
in ms, a warm-up, then best and median of seven (three for the dense leg):
  a      vsl_global_ba_covariance, all free cameras
  b      the same plus 1000 landmarks
  c      the same plus all landmarks (those with at most 256 observations)
  d      yardstick: vsl_ba_covariance (dense) with the query of (a); also the largest difference between (a) and (d)
         relative to the largest entry
  e      yardstick: one LM iteration of vsl_global_bundle_adjust (the marginal time between a 3- and a 12-iteration solve
         on the solver's own clock, as bench.py measures it)
--kf 250 runs everything on the 250-keyframe loop instead (for when (d) does not finish inside the time limit at 500).
VSL_SO=<path> measures another build of the library (leg e on the parent commit).

  python tools/global_ba_cov_probe.py [--kf 500] [--legs a,b,c,d,e] [--out profiles/global_ba_cov_probe.json] [--timeout 150]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def leg(name, kf):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as entry
    import numpy as np
    vsl = entry.load_package()
    if os.environ.get("VSL_SO"):
        vsl._SO = Path(os.environ["VSL_SO"]).resolve()
    synth = importlib.import_module("visual_slam_amd.synth")
    vsl.load()
    d = synth.ba_problem(5, n_kf=kf, n_lms=100000 * kf // 500, loop_radius=200.0 * kf / 500.0, max_range=15.0)
    arr = vsl.BaArrays.from_dict(d)
    out = {"leg": name, "keyframes": kf, "cameras": len(arr.poses), "free_cameras": arr.n_free, "landmarks": len(arr.points),
           "observations": len(arr.obs_cam)}
    ctx = vsl.Context(0)
    cnt = np.bincount(arr.obs_lm, minlength=len(arr.points))
    ok_lms = np.flatnonzero(cnt <= 256).astype(np.int32)
    if name in ("a", "b", "c"):
        lms = {"a": None, "b": ok_lms[np.linspace(0, len(ok_lms) - 1, 1000).astype(int)], "c": ok_lms}[name]
        (cp, cl, nd, storage), t = timed(lambda: ctx.global_ba_covariance(arr, lms=lms), 7)
        out.update(t, storage=storage, queried_cameras=len(cp), queried_landmarks=len(cl), n_degenerate=nd,
                   half_bandwidth=ctx.last_ba_layout()[2])
    elif name == "d":
        (dp, _, _), t = timed(lambda: ctx.ba_covariance(arr), 3)
        cp, _, _, storage = ctx.global_ba_covariance(arr)
        out.update(t, queried_cameras=len(dp), storage_of_a=storage,
                   max_abs_difference_a_d_over_max=float(np.abs(cp - dp).max() / np.abs(dp).max()))
    else:
        ba_dist = importlib.import_module("visual_slam_amd.ba_dist")
        ba_dist.bundle_adjust_distributed(vsl, ctx, arr.copy(), max_iters=1)
        loops, its = {}, {}
        for iters in (3, 12, 3, 12, 3, 12):
            s = ba_dist.bundle_adjust_distributed(vsl, ctx, arr.copy(), max_iters=iters)
            if iters not in loops or s.total_ms < loops[iters]:
                loops[iters], its[iters] = s.total_ms, s.iterations
        out.update(ms_per_lm_iteration=round((loops[12] - loops[3]) / max(its[12] - its[3], 1), 4), iterations=[its[3], its[12]])
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=500)
    ap.add_argument("--legs", default="a,b,c,d,e")
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--timeout", type=float, default=150.0, help="seconds per leg")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.kf)))
        return 0
    res = {"label": a.label, "library": os.environ.get("VSL_SO", "visual-slam_amd/libvslam_hip.so"),
           "date": time.strftime("%Y-%m-%d"), "legs": []}
    rc = 0
    for name in a.legs.split(","):
        try:
            r = subprocess.run([sys.executable, __file__, "--leg", name, "--kf", str(a.kf)], capture_output=True, text=True,
                               timeout=a.timeout)
        except subprocess.TimeoutExpired:
            res["legs"].append({"leg": name, "keyframes": a.kf, "error": "time limit of %.0f s" % a.timeout})
            rc = 1
            break  # nothing more is started on the device after a leg that hung
        if r.returncode != 0:
            res["legs"].append({"leg": name, "keyframes": a.kf, "error": "exit %d: %s" % (r.returncode, r.stderr[-400:])})
            rc = 1
            break
        res["legs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
