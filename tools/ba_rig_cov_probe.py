"""Covariances in rig form on the benchmark's local window in rig form (7 stereo keyframes, ~15k landmarks): host wall
time of the synchronous call, best of five after a warm-up.  Query: all free bodies, all their cameras, 1000 landmarks.
  rig_cov    Context.ba_rig_covariance
  rig_iter   one LM iteration of Context.bundle_adjust_rig on the same problem (the yardstick)
  free_cov   Context.ba_covariance of the expanded free problem (the same cameras and landmarks queried)
One leg per process (argv[1]): run the legs in processes of their own, alternating.  One JSON line."""
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as entry  # noqa: E402

leg = sys.argv[1] if len(sys.argv) > 1 else "rig_cov"
vsl = entry.load_package()
synth = importlib.import_module("visual_slam_amd.synth")
ctx = vsl.Context(0)
d = synth.ba_problem(4, n_kf=7, n_lms=20000)
n_cams = len(d["poses"])
T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], synth.T_0_1])   # the generator's own stereo extrinsic
bodies = np.asarray(d["poses"]).reshape(-1, 7)[0::2]        # the body of keyframe k is its left camera (2 k)
fixed = np.asarray(d["cam_fixed"])[0::2]
cam_body = np.arange(n_cams) // 2
q_bodies = np.flatnonzero(fixed == 0)
q_cams = np.flatnonzero(fixed[cam_body] == 0)
L = len(d["points"])
q_lms = np.arange(0, L, max(L // 1000, 1))[:1000]


def call():
    arr = vsl.BaArrays.from_dict(d)
    if leg == "rig_cov":
        return ctx.ba_rig_covariance(arr, vsl.RigArrays(bodies, fixed, cam_body, T_b_c), q_bodies, q_cams, q_lms)
    if leg == "rig_iter":
        return ctx.bundle_adjust_rig(arr, vsl.RigArrays(bodies, fixed, cam_body, T_b_c), max_iters=1)
    # the free problem of the same cameras: each camera on the calibration of its body
    arr.cam_fixed[:] = fixed[cam_body]
    return ctx.ba_covariance(arr, q_cams, q_lms)


call()
ms = []
for _ in range(5):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = call()
    ms.append(1e3 * (time.perf_counter() - t0))
rec = {"leg": leg, "cameras": n_cams, "landmarks": L, "observations": len(d["obs_cam"]), "free_bodies": len(q_bodies),
       "queried_cameras": len(q_cams), "queried_landmarks": len(q_lms), "ms_best_of_5": min(ms), "ms_all": ms}
if leg != "rig_iter":
    rec["n_degenerate"] = int(out[-1])
    rec["max_abs_pose_block"] = float(np.abs(out[0]).max())
print(json.dumps(rec))
ctx.close()
