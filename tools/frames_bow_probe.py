"""Cost of the batched keyframe BoW on the frame store (vsl_frames_bow_vectors) next to the per-image
loop it replaces -- vsl_compute_bow_vector + vsl_bowdb_append for every image -- on the same 752 x 480 images.

    python3 tools/frames_bow_probe.py [--n 1 16 256] [--features 1500] [--voc-levels 4] [--reps 10] [--warmup 2]

The loop uploads every image from the host, as its callers do; the batched call reads the images where the frame store
already holds them (uploaded before the clock starts: in the odometry loop they are there anyway).  Both ways end in a
stream synchronisation, so a host clock around them is their time.  They are timed alternately in one process after a
warm-up, each into a fresh database created outside the clock, and the vectors and the two databases' answers are
compared before anything is timed.  One JSON line per n.  For the kernels' own times run it under
`rocprofv3 --kernel-trace --stats -- python3 tools/frames_bow_probe.py --n 16` in a run of its own."""
import argparse
import importlib
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def images(synth, n):
    """n distinct 752 x 480 images: a few rendered stereo pairs, shifted."""
    base = []
    for seed in range(4):
        base.extend(synth.stereo_pair(20 + seed))
    return np.stack([np.roll(base[i % len(base)], (3 * (i // len(base)), 5 * (i // len(base))), (0, 1)) for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--features", type=int, default=1500)
    ap.add_argument("--voc-levels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import __graft_entry__ as entry
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    ctx = vsl.Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "voc.txt"
        path.write_text(synth.vocabulary_text(5, 10, a.voc_levels))
        voc = vsl.Vocabulary(ctx, str(path))
    n_words = voc.info()[3]
    for n in a.n:
        imgs = images(synth, n)
        h, w = imgs.shape[1:]
        frames = vsl.Frames(ctx, n, w, h, max_features=64, max_pairs=1)
        frames.upload(0, imgs)
        cap_entries, cap_vecs = (2 * a.features + 512) * n, max(n, 64)

        def loop(db):
            out = []
            for img in imgs:
                v = voc.compute_bow_vector(img, a.features, 4)
                db.append(v[0], v[1])
                out.append(v)
            return out

        def batched(db):
            return frames.bow_vectors(0, n, voc, a.features, 4, db=db)[0]

        def device_only(db):
            return frames.bow_vectors(0, n, voc, a.features, 4, db=db, host_outputs=False)

        ways = (("batched", batched), ("batched_device_only", device_only), ("loop", loop))
        dbs = {name: vsl.BowDatabase(ctx, cap_entries, cap_vecs) for name, _ in ways}
        res = {name: fn(dbs[name]) for name, fn in ways}
        for g, e in zip(res["batched"], res["loop"]):
            assert all(np.array_equal(x, y) for x, y in zip(g, e)) and np.array_equal(g[1].view(np.uint64), e[1].view(np.uint64))
        q = res["loop"][0]
        ans = [(db.info(), db.score(q[0], q[1]).view(np.uint64).tolist(), [x.tolist() for x in db.query(q[0], q[1], n_words)[:2]])
               for db in dbs.values()]
        assert ans[0] == ans[1] == ans[2], "the databases differ"
        for db in dbs.values():
            db.close()
        t = {name: [] for name, _ in ways}
        for rep in range(a.warmup + a.reps):
            for name, fn in ways:  # alternating: all see the same machine
                db = vsl.BowDatabase(ctx, cap_entries, cap_vecs)
                ctx.synchronize()
                t0 = time.perf_counter()
                fn(db)
                dt = 1e3 * (time.perf_counter() - t0)
                db.close()
                if rep >= a.warmup:
                    t[name].append(dt)
        med = {k: float(np.median(v)) for k, v in t.items()}
        out = {"n": n, "image": [w, h], "features": a.features, "vocabulary_nodes": voc.info()[2],
               "features_per_image": round(float(np.mean([len(v[3]) for v in res["loop"]])), 1), "reps": a.reps}
        for name in t:
            out[name + "_ms_median"] = round(med[name], 3)
            out[name + "_ms_min_max"] = [round(min(t[name]), 3), round(max(t[name]), 3)]
            out[name + "_ms_per_image"] = round(med[name] / n, 4)
        out["speedup"] = round(med["loop"] / med["batched"], 2)
        print(json.dumps(out), flush=True)
        frames.close()
    voc.close()
    ctx.close()


if __name__ == "__main__":
    main()
