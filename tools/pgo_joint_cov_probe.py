"""Timing probe of vsl_pgo_joint_covariance and vsl_pgo_edge_consistency on the 500-keyframe ring
of the pose_graph bench leg (synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6): the generator of
tools/pgo_cov_probe.py), for 1, 16 and 256 candidate pairs half a ring apart -- out-of-band pairs, the band unit-column
solve -- on the route the graph takes and on route 0 (diagnostic ba_force_dense), next to vsl_pgo_covariance of the same
nodes on either route.  Host wall time of the synchronous calls in ms: a warm-up, then best and median of seven, all in
one process.  Prints one JSON line."""
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
    g = Arrays(d)
    free = np.flatnonzero(g.node_fixed == 0)
    nf = len(free)
    out = {"graph": "500 keyframes, window 6, %d edges, %d fixed" % (len(g.edge_a), int(np.sum(g.node_fixed != 0))), "cases": []}
    for n_pairs in (1, 16, 256):
        k = np.arange(n_pairs) * (nf // 2) // n_pairs
        pairs = np.stack([free[k], free[(k + nf // 2) % nf]], axis=1)
        nodes = np.unique(pairs)
        meas = np.zeros((n_pairs, 6))
        case = {"pairs": n_pairs, "distinct_nodes": len(nodes)}
        for label, dense in (("route_taken", 0), ("forced_dense", 1)):
            ctx.set_diagnostic("ba_force_dense", dense)
            try:
                (cov, storage), tj = timed(lambda: ctx.pgo_joint_covariance(g, pairs))
                (_, _, chi2, _), te = timed(lambda: ctx.pgo_edge_consistency(g, pairs[:, 0], pairs[:, 1], meas))
                (_, st_m), tm = timed(lambda: ctx.pgo_covariance(g, nodes=nodes))
            finally:
                ctx.set_diagnostic("ba_force_dense", 0)
            case[label] = {"storage": storage, "joint_covariance": tj, "edge_consistency": te,
                           "marginals_of_the_same_nodes": dict(tm, storage=st_m)}
            case[label + "_cov"] = cov
        a, b = case.pop("route_taken_cov"), case.pop("forced_dense_cov")
        case["max_abs_difference_over_max"] = float(np.abs(a - b).max() / np.abs(b).max())
        case["dense_over_band_joint"] = round(case["forced_dense"]["joint_covariance"]["best_ms"] /
                                              case["route_taken"]["joint_covariance"]["best_ms"], 2)
        out["cases"].append(case)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
