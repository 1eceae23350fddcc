"""Timing probe of vsl_ba_covariance beside its yardstick, one LM iteration of vsl_bundle_adjust on the same problem.

Two problems: BASELINE configs[2] (7 keyframes = 14 cameras, ~15 k landmarks; all 12 free cameras and 1000 landmarks
queried) and the 10-keyframe window (20 cameras, 18 free = 108 unknowns; all free cameras, 1000 landmarks).  Per problem
two legs, each in a child process of its own under its own time limit, host wall time of the synchronous call, best of
five after a warm-up:
  cov    Context.ba_covariance (skipped, and reported as such, when the library has no vsl_ba_covariance: the same script
         then measures the solve leg of an older build)
  solve  Context.bundle_adjust with max_iters = 1 on a fresh copy of the problem
VSL_SO=<path> measures another build of the library with this script (tools/local_ba_probe.py has the same switch).

  python tools/ba_cov_probe.py [--out profiles/ba_cov_probe.json] [--label text] [--timeout 120]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PROBLEMS = {"configs2_7kf": 7, "window_10kf": 10}
N_LMS_QUERIED = 1000


def leg(name, problem):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as entry
    import numpy as np
    vsl = entry.load_package()
    if os.environ.get("VSL_SO"):
        vsl._SO = Path(os.environ["VSL_SO"]).resolve()
    synth = importlib.import_module("visual_slam_amd.synth")
    L = vsl.load()
    d = synth.ba_problem(4, n_kf=PROBLEMS[problem], n_lms=20000)
    arr = vsl.BaArrays.from_dict(d)
    out = {"leg": name, "problem": problem, "cameras": len(arr.poses), "free_cameras": arr.n_free,
           "landmarks": len(arr.points), "observations": len(arr.obs_cam)}
    if name == "cov" and not hasattr(L, "vsl_ba_covariance"):
        out["skipped"] = "the library has no vsl_ba_covariance"
        return out
    ctx = vsl.Context(0)
    lms = np.linspace(0, len(arr.points) - 1, N_LMS_QUERIED).astype(np.int32)
    if name == "cov":
        call = lambda a: ctx.ba_covariance(a, lms=lms)  # noqa: E731
        out["queried_cameras"], out["queried_landmarks"] = arr.n_free, len(lms)
    else:
        call = lambda a: ctx.bundle_adjust(a, max_iters=1)  # noqa: E731
    call(arr.copy())
    times = []
    for _ in range(5):
        a = arr.copy()
        ctx.synchronize()
        t0 = time.perf_counter()
        r = call(a)
        times.append(1e3 * (time.perf_counter() - t0))
    if name == "cov":
        out["n_degenerate"] = int(r[2])
        out["sqrt_trace_translation_last_camera"] = float(np.sqrt(np.trace(r[0][-1][:3, :3])))
    else:
        out["iterations"] = int(r.iterations)
    out["ms_best_of_5"], out["ms_all"] = min(times), times
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per leg")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--problem", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.problem)))
        return 0
    res = {"label": a.label, "library": os.environ.get("VSL_SO", "visual-slam_amd/libvslam_hip.so"),
           "date": time.strftime("%Y-%m-%d"), "legs": []}
    for problem in PROBLEMS:
        for name in ("cov", "solve"):
            try:
                r = subprocess.run([sys.executable, __file__, "--leg", name, "--problem", problem], capture_output=True, text=True,
                                   timeout=a.timeout)
            except subprocess.TimeoutExpired:
                res["legs"].append({"leg": name, "problem": problem, "error": "time limit of %.0f s" % a.timeout})
                print(json.dumps(res))
                return 1  # nothing more is started on the device after a leg that hung
            if r.returncode != 0:
                res["legs"].append({"leg": name, "problem": problem, "error": "exit %d: %s" % (r.returncode, r.stderr[-400:])})
                print(json.dumps(res))
                return 1
            res["legs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
