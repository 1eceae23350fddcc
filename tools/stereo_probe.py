"""Cost of the device stereo stage (csrc/stereo.hip) next to the pass that feeds it: bench.py's launch of 1024 images
(512 stereo frames, 1500 keypoints) through detect + describe + match, then vsl_frames_stereo_inliers over the 512 pairs
with the reference's V1 ds calibration and E / R / t of its stereo extrinsics, threshold 1e-3, triangulating.

Run it under the kernel tracer and summarise the trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/stereo_probe.py
    python3 tools/stereo_probe.py --stats OUT
The first form also prints the mean inlier count and the host wall time of one stage call + synchronisation.  An optional
threshold argument replaces 1e-3 (`inf`: every match is an inlier and is triangulated -- the stage's largest output; the
synthetic scenes of bench.py are not drawn with the V1 stereo geometry, so at 1e-3 almost every match is rejected)."""
import csv
import glob
import importlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
REPS = 20


def stats(out_dir):
    f = max(glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    st, pass_ns, other = None, 0.0, []
    for r in csv.DictReader(open(f)):
        name, total = r["Name"], float(r["TotalDurationNs"])
        if "stereo_inliers_kernel" in name:
            st = (int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"]))
        else:
            pass_ns += total
            other.append((name.replace("void ", "")[:60], int(r["Calls"]), total))
    calls, avg, mn, mx = st
    # every other kernel belongs to the detect + describe + match pass, which ran as often as the stage
    n_pass = calls
    out = {"stereo_kernel_us_avg": round(avg / 1e3, 2), "stereo_kernel_us_min": round(mn / 1e3, 2),
           "stereo_kernel_us_max": round(mx / 1e3, 2), "stereo_calls": calls,
           "pass_us_per_launch": round(pass_ns / n_pass / 1e3, 1),
           "stereo_share_of_pass": round(avg / (pass_ns / n_pass), 4)}
    print(json.dumps(out))
    for name, c, total in sorted(other, key=lambda x: -x[2])[:12]:
        print("  %-60s calls %5d  %9.1f us/launch" % (name, c, total / n_pass / 1e3))


def workload(threshold):
    import __graft_entry__ as entry
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    Bu = 512
    base = np.concatenate([synth.stereo_pair_variants(10 + s, 4, margin=24) for s in range(16)])  # bench.py's 64 pairs
    imgs = np.concatenate([base] * (Bu // len(base)))[:Bu].reshape(2 * Bu, 480, 752)
    ctx = vsl.Context(0)
    fr = vsl.Frames(ctx, 2 * Bu, 752, 480, 1500, max_pairs=Bu)
    fr.upload(0, imgs)
    pairs = np.array([[2 * k, 2 * k + 1] for k in range(Bu)], np.int32)
    c0, c1 = sq.CALIB["intrinsics"]
    cam = [(vsl.CAM_DS, [c["fx"], c["fy"], c["cx"], c["cy"], c["p1"], c["p2"]]) for c in (c0, c1)]
    T = sq.CALIB["T_i_c"][1]
    q = np.array([T["qx"], T["qy"], T["qz"], T["qw"]])
    q = q / np.linalg.norm(q)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t = np.array([T["px"], T["py"], T["pz"]])
    tn = t / np.linalg.norm(t)
    E = np.array([[0, -tn[2], tn[1]], [tn[2], 0, -tn[0]], [-tn[1], tn[0], 0]]) @ R
    host_ms = []
    for rep in range(REPS + 2):
        fr.detect_describe(0, 2 * Bu, 1500, True)
        fr.resolve_ties()
        fr.match(pairs, 70, 1.2)
        ctx.synchronize()
        t0 = time.perf_counter()
        fr.stereo_inliers(0, Bu, cam[0], cam[1], E, R, t, threshold, True)
        ctx.synchronize()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    _, nm = fr.counts(2 * Bu, Bu)
    ni = fr.inlier_counts(Bu)
    print(json.dumps({"pairs": Bu, "threshold": repr(threshold), "matches_per_pair": round(float(nm.mean()), 1),
                      "inliers_per_pair": round(float(ni.mean()), 1),
                      "stage_call_plus_sync_ms_median": round(float(np.median(host_ms[2:])), 4)}), flush=True)
    fr.close()
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--stats":
        stats(sys.argv[2])
    else:
        workload(float(sys.argv[1]) if len(sys.argv) > 1 else 1e-3)
