"""Cost of the batched fusion search (vsl_fuse_search, csrc/vo.hip) next to the per-view loop it replaces, on the same inputs:
16 views x 1500 keypoints x 4000 landmarks with at most 20 observations each (DESIGN.md "Landmark fusion").

    python3 tools/fuse_probe.py [--views 16] [--kp 1500] [--lms 4000] [--max-obs 20] [--reps 30] [--warmup 5]

Both ways are host calls that end in a stream synchronisation, so a host clock around the call is the call's time.  The
two are timed alternately in one process (warm-up first), the medians and the spread are printed as one JSON line, and
the results of the two ways are compared pair for pair before anything is timed.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/fuse_probe.py` in a run of its own."""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
W, H = 752, 480
INTR = [351.0, 350.0, 365.9, 249.3, -0.2385, 0.5679, 0, 0]  # double sphere


def inputs(ctx, synth, seed, n_views, n_kp, n_lms, max_obs):
    rng = np.random.default_rng(seed)
    base = np.concatenate([synth.axis_angle_q(rng.normal(size=3), 0.3), rng.normal(0, 0.5, 3)])
    pc = np.stack([rng.uniform(-6, 6, n_lms), rng.uniform(-4, 4, n_lms), rng.uniform(1, 12, n_lms)], -1)
    pw = pc @ synth.quat_R(base[:4]).T + base[4:]
    n_obs = rng.integers(1, max_obs + 1, n_lms)
    start = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    obs = synth.random_descriptors(rng, int(start[-1]))
    poses, kp_xy, kp_desc = [], [], []
    for _ in range(n_views):
        pose = synth.se3_mul(base, np.concatenate([synth.axis_angle_q(rng.normal(size=3), 0.05), rng.normal(0, 0.1, 3)]))
        xy = np.stack([rng.integers(19, 733, n_kp), rng.integers(19, 461, n_kp)], -1).astype(np.float64)
        desc = synth.random_descriptors(rng, n_kp)
        uv, idx = ctx.project_landmarks(pose, 0, INTR, W, H, pw, 0.1)
        # six keypoints in ten sit near a projected landmark that carries a noisy copy of their descriptor
        for k in np.flatnonzero(rng.random(n_kp) < 0.6):
            j = int(rng.integers(len(idx)))
            l = int(idx[j])
            xy[k] = np.clip(np.round(uv[j] + rng.uniform(-12, 12, 2)), [0, 0], [W - 1, H - 1])
            o = int(start[l] + rng.integers(n_obs[l]))
            obs[o] = desc[k]
            for b in rng.choice(256, size=int(rng.integers(0, 40)), replace=False):
                obs[o, b // 64] ^= np.uint64(1) << np.uint64(b % 64)
        poses.append(pose)
        kp_xy.append(xy)
        kp_desc.append(desc)
    return np.array(poses), kp_xy, kp_desc, pw, start, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--kp", type=int, default=1500)
    ap.add_argument("--lms", type=int, default=4000)
    ap.add_argument("--max-obs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as entry
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    ctx = vsl.Context(0)
    poses, kp_xy, kp_desc, pw, start, obs = inputs(ctx, synth, 1, a.views, a.kp, a.lms, a.max_obs)

    def batched():
        return ctx.fuse_search(poses, 0, INTR, W, H, kp_xy, kp_desc, pw, start, obs, 0.1, 20.0, 70, 1.2)

    def per_view():
        pairs, n_proj = [], []
        for v in range(a.views):
            uv, idx = ctx.project_landmarks(poses[v], 0, INTR, W, H, pw, 0.1)
            pairs.append(ctx.find_matches_landmarks(kp_xy[v], kp_desc[v], uv, idx, start, obs, 20.0, 70, 1.2))
            n_proj.append(len(idx))
        return pairs, np.array(n_proj, np.int32)

    got, got_np = batched()
    exp, exp_np = per_view()
    assert np.array_equal(got_np, exp_np) and all(np.array_equal(g, e) for g, e in zip(got, exp)), "the two ways differ"
    t = {"batched": [], "per_view": []}
    for rep in range(a.warmup + a.reps):
        for name, fn in (("batched", batched), ("per_view", per_view)):  # alternating: both see the same machine
            t0 = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= a.warmup:
                t[name].append(dt)
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"views": a.views, "keypoints_per_view": a.kp, "landmarks": a.lms, "observations": int(start[-1]),
                      "pairs": int(sum(len(p) for p in got)), "projected_per_view": round(float(got_np.mean()), 1),
                      "reps": a.reps, "batched_ms_median": round(med["batched"], 4),
                      "batched_ms_min_max": [round(min(t["batched"]), 4), round(max(t["batched"]), 4)],
                      "per_view_loop_ms_median": round(med["per_view"], 4),
                      "per_view_loop_ms_min_max": [round(min(t["per_view"]), 4), round(max(t["per_view"]), 4)],
                      "speedup": round(med["per_view"] / med["batched"], 2)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
