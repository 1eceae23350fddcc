"""Timing probe of vsl_pgo_covariance on the 500-keyframe ring of the pose_graph bench leg
(synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6): the generator of tools/pgo_probe.py), all free
nodes queried, beside two yardsticks from the same build:
  lm_iter   one Levenberg-Marquardt iteration of vsl_pose_graph_optimize on that graph (a 20-iteration solve / iterations)
  dense     the same covariance call on route 0 (diagnostic ba_force_dense)
Host wall time of the synchronous calls in ms: a warm-up, then best and median of seven.  Prints one JSON line."""
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


class Arrays:
    def __init__(self, d):
        self.poses = np.ascontiguousarray(d["poses"], np.float64).copy()
        self.node_fixed = np.ascontiguousarray(d["node_fixed"], np.uint8)
        self.edge_a = np.ascontiguousarray(d["edge_a"], np.int32)
        self.edge_b = np.ascontiguousarray(d["edge_b"], np.int32)
        self.edge_meas = np.ascontiguousarray(d["edge_meas"], np.float64)


def timed(fn, reps=7):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def main():
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    ctx = vsl.Context(0)
    d = synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6)
    out = {"graph": "500 keyframes, window 6, %d edges, %d fixed" % (len(d["edge_a"]), int(np.sum(d["node_fixed"] != 0)))}
    (cov, storage), t = timed(lambda: ctx.pgo_covariance(Arrays(d)))
    out["covariance"] = dict(t, storage=storage, blocks=len(cov))
    ctx.set_diagnostic("ba_force_dense", 1)
    (cov_d, storage_d), t = timed(lambda: ctx.pgo_covariance(Arrays(d)), reps=3)
    ctx.set_diagnostic("ba_force_dense", 0)
    out["covariance_dense"] = dict(t, storage=storage_d)
    out["max_abs_difference_over_max"] = float(np.abs(cov - cov_d).max() / np.abs(cov_d).max())
    s, t = timed(lambda: ctx.pose_graph_optimize(Arrays(d), True, 1.0, 20))
    out["solve"] = dict(t, iterations=s.iterations, ms_per_iteration=round(t["best_ms"] / max(s.iterations, 1), 3))
    out["covariance_over_lm_iteration"] = round(out["covariance"]["best_ms"] / out["solve"]["ms_per_iteration"], 2)
    out["dense_over_covariance"] = round(out["covariance_dense"]["best_ms"] / out["covariance"]["best_ms"], 2)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
