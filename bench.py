#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X-native visual-SLAM hot path.

Metric (BASELINE.json): stereo frames/sec on synthetic 752x480 stereo, 1500 features per frame
(configs[1]); one rank per GPU, every rank owns independent streams (configs[3]: weak scaling, no
data-path collective).

One PASS = the per-frame hot path over B distinct stereo frames already resident in HBM:
detectKeypointsAndDescriptors on 2B images (K1 response, K2 selection, K3+K4 orientation + rBRIEF-256)
->  exactness guard (vsl_frames_resolve_ties: one stream sync + 4-byte readback)  ->
matchDescriptors(left, right, 70, 1.2) on B pairs (K5); outputs stay in HBM.  The batch is split over S HIP
streams (default 2 x 512 stereo frames): the selection kernel is one latency-bound workgroup per image and leaves
most of each CU's issue slots free, so the other stream's response / describe kernels run underneath it.
One STEP = `--passes` passes (default 18, ~62 ms), so that the driver's 20 timed steps cover > 1 s of sustained
clocks.  `value` = frames of all passes / time, inputs resident in HBM (the contract's definition).

Next to it, at N = 1, the STREAMING mode measures the same hot path fed from the host (`value_incl_upload`):
the B distinct stereo pairs sit in a pinned host ring, an upload context copies the next 512-frame batch into the
idle one of two frame stores while the other one is being processed (vsl_event hand-offs, no host round trip),
and the per-pair match counts are read back per batch.  It reports the PCIe rate achieved and which side bounds.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--passes P] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run does what the headline figure needs and nothing else: set-up, W warm-up steps, the K timed steps, the
outputs (--dump-outputs DIR) and ONE JSON line on rank 0 (`value`, `ms_per_step`, `config`, `per_rank`).  The rest --
the streaming mode above, the per-stage times and rooflines, the CPU baseline and the output check against the oracle,
the BA / pose-graph / BoW / end-to-end legs below and, for N > 1, the multi-rank global BA -- runs with --full only.

--dump-outputs DIR writes what the timed path left in HBM after its last step as DIR/<name>.npy (float32 / float64, a
few MB): keypoint and match counts of every stereo frame, and the keypoints (position, angle, descriptor bytes) and
match lists of a fixed, seeded sample of the frames.  The inputs depend on the arguments only, so two builds can be
compared output for output.

With --full the line carries more.  `roofline` is for the dominant kernel, timed with HIP events on the stream the
kernels run on; `cpu_baseline` is the CPU oracle (a port of the reference's path, the reference itself cannot be
built offline) timed on the host's cores on a bounded sample of the same frames -- and the timed run's outputs
for those frames are compared with the oracle's (`outputs_equal_oracle_sample`).

At N = 1 the line also carries: `local_ba` / `global_ba` (ms per LM iteration, BASELINE configs[2] / [4]); `bow` (DBoW2
transform and L1 score on a k = 10, L = 6 vocabulary, device time, bytes, oracle beside it); the end-to-end legs of the
headless next_step pipeline on a rendered 640-frame lap -- `end_to_end_single_stream` with the reference's default-on
branches (relocalisation, loop closure, per-keyframe BoW) next to `cpu_baseline_end_to_end` (the same application on
the CPU oracle), `end_to_end_loop_closing_stages` (a labelled stage exerciser), `end_to_end_vo_subset` (round 2's
configuration) -- and the single-stream device accounting from the committed rocprofv3 summary.

`--gpus N` without a launcher starts the N ranks itself (torch.distributed.run as a child process); under a launcher
WORLD_SIZE must equal N.
"""
import argparse
import importlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as entry  # noqa: E402

W, H, NUM_FEATURES = 752, 480, 1500
SYNTH_MARGIN = 24  # synth.stereo_pair(margin=24): the 1500 strongest corners are interior, ~1500 keypoints survive the border filter
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8 TB/s (6.3 TB/s achievable)
I8_PEAK_TOPS = 5000.0   # dense int8 MFMA = 2x the 2.5 PFLOP/s bf16 peak (MI355X_MICROARCH.md, MFMA table)
FP4_PEAK_TOPS = 10000.0  # dense block-scaled FP4 MFMA (same table): the instruction the matcher runs on for <= 2048 features


def stage_algorithmic_bytes(stage, n_img, n_pairs, kp_total, cand_total, match_total):
    """Compulsory bytes of one launch of a stage over the whole batch (DESIGN.md 'Kernels'):
    one read of each input and one write of each OUTPUT of the path -- intermediates (provisional candidate keys,
    best / second keys) are not counted."""
    px = W * H
    if stage in ("response", "detect_describe"):
        # 8(d) row "detect+angle+describe": image in, (xy 16 + angle 8 + descriptor 32) B per keypoint out; the
        # response kernel is priced with the figure of the stage it dominates
        return n_img * px + 56 * kp_total
    if stage == "select":        # K2b: candidate keys in, selected corners out
        return 8 * cand_total + 8 * kp_total
    if stage == "describe":      # K3+K4: 709-px disc + position in, moments/angle/descriptor out
        return kp_total * (709 + 8 + 8 + 8 + 32)
    if stage == "match":         # 8(d) row "match": both descriptor sets in, match list out
        return kp_total * 32 + match_total * 8
    if stage == "match_finalize":
        return kp_total * 8 + match_total * 8
    return 0


def _gen_scene(job):
    seed, n_variants = job
    synth = importlib.import_module("visual_slam_amd.synth")
    return synth.stereo_pair_variants(seed, n_variants, margin=SYNTH_MARGIN)


def distinct_stereo_frames(seeds, n_variants, workers):
    """(len(seeds) * n_variants, 2, H, W) uint8: every stereo pair distinct (scene x sensor-noise realisation).
    Called BEFORE anything touches the GPU (worker processes are forked)."""
    jobs = [(int(s), n_variants) for s in seeds]
    if workers > 1 and len(jobs) > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(min(workers, len(jobs))) as pool:
            parts = pool.map(_gen_scene, jobs)
    else:
        parts = [_gen_scene(j) for j in jobs]
    return np.concatenate(parts, axis=0)


DUMP_SAMPLE_FRAMES = 32   # stereo frames whose keypoints and matches --dump-outputs writes (<= 15 MB at 1500 features)
DUMP_SAMPLE_SEED = 2024


def dump_outputs(dirname, units, counts, B, Bu):
    """--dump-outputs: the outputs of the timed path's last step (every pass recomputes the same frames, so the frame
    stores hold them after the timed region), as float arrays.  Counts for all B stereo frames; keypoints and match
    lists for a fixed, seeded sample of them.  Stereo frame f lives in unit f // Bu, images 2k / 2k+1 and pair k for
    k = f % Bu."""
    os.makedirs(dirname, exist_ok=True)
    sample = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(B, min(DUMP_SAMPLE_FRAMES, B), replace=False))
    xy, ang, desc, n_kp, pairs, n_m = [], [], [], [], [], []
    for f in sample:
        fr = units[f // Bu][2]
        k = int(f % Bu)
        for slot in (2 * k, 2 * k + 1):
            p, a, d = fr.keypoints(slot)
            xy.append(p)
            ang.append(a)
            desc.append(d.view(np.uint8).reshape(-1, 32))   # the 256-bit descriptor as its 32 bytes
            n_kp.append(len(p))
        m = fr.matches(k)
        pairs.append(m)
        n_m.append(len(m))
    arrays = {
        "keypoints_per_image": np.concatenate([c[0] for c in counts]).astype(np.float64),   # (2B,) left, right, ...
        "matches_per_pair": np.concatenate([c[1] for c in counts]).astype(np.float64),      # (B,)
        "sample_stereo_frames": sample.astype(np.float64),
        "sample_keypoints_per_image": np.asarray(n_kp, np.float64),
        "sample_keypoints_xy": np.concatenate(xy).astype(np.float64).reshape(-1, 2),
        "sample_keypoints_angle": np.concatenate(ang).astype(np.float64),
        "sample_descriptor_bytes": np.concatenate(desc).astype(np.float32),
        "sample_matches_per_pair": np.asarray(n_m, np.float64),
        "sample_matches": np.concatenate(pairs).astype(np.float64).reshape(-1, 2),         # (left, right) keypoint indices
    }
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def streaming_measurement(vsl, units, ring, Bu, slot_pairs, seconds, device, expect_matches):
    """Upload-inclusive throughput of the same hot path (N = 1).  `ring` = pinned host array (B, 2, H, W) of distinct
    stereo pairs; the two frame stores of `units` are the double buffer: an upload context copies batch k+1 into the
    idle store while batch k is processed (vsl_event hand-offs on the device), and batch k's per-pair match counts are
    read back before batch k+1 is enqueued.  Mirrors the reference's order load -> detect x2 -> match
    (src/slam.cpp:1122-1141)."""
    n_img = 2 * Bu
    chunks = [ring[c * Bu:(c + 1) * Bu].reshape(n_img, H, W) for c in range(len(ring) // Bu)]
    bufs = [units[0], units[1]]
    copy_ctx = vsl.Context(device)  # its own stream
    uploaded = [vsl.Event(copy_ctx) for _ in range(2)]
    computed = [vsl.Event(copy_ctx) for _ in range(2)]
    batch_bytes = n_img * W * H

    def enqueue_upload(k):
        b = k % 2
        copy_ctx.wait_event(computed[b])          # the store's previous batch has been consumed
        bufs[b][2].upload_async(0, chunks[k % len(chunks)], ctx=copy_ctx)
        uploaded[b].record(copy_ctx)

    def compute(k):
        b = k % 2
        _, c, fr = bufs[b]
        c.wait_event(uploaded[b])
        fr.detect_describe(0, n_img, NUM_FEATURES, True)
        fr.resolve_ties()
        fr.match(slot_pairs, 70, 1.2)
        computed[b].record(c)
        return fr.counts(0, Bu)[1]                 # per-batch readback (host sync on this batch)

    def run(min_seconds, check):
        ok = True
        for _, c, _ in bufs:
            c.synchronize()
        copy_ctx.synchronize()
        t0 = time.perf_counter()
        enqueue_upload(0)
        k = 0
        while True:
            more = (time.perf_counter() - t0) < min_seconds
            if more:
                enqueue_upload(k + 1)
            nm = compute(k)
            if check:
                ok = ok and np.array_equal(nm, expect_matches[k % len(chunks)])
            k += 1
            if not more:
                break
        copy_ctx.synchronize()
        return k, time.perf_counter() - t0, ok

    run(0.15, False)                                # warm-up (first-touch of the pinned pages by the DMA engine)
    n_batches, dt, ok = run(seconds, True)
    # copy alone (the PCIe ceiling as this process sees it) for the same batch size
    copy_ctx.synchronize()
    t0 = time.perf_counter()
    n_copy = 0
    while time.perf_counter() - t0 < 0.3:
        for _ in range(4):
            bufs[n_copy % 2][2].upload_async(0, chunks[n_copy % len(chunks)], ctx=copy_ctx)
            n_copy += 1
        copy_ctx.synchronize()
    dt_copy = time.perf_counter() - t0
    for e in uploaded + computed:
        e.close()
    copy_ctx.close()
    fps = n_batches * Bu / dt
    copy_only_fps = n_copy * Bu / dt_copy
    return {"value_incl_upload": round(fps, 2),
            "h2d_gbps": round(n_batches * batch_bytes / dt / 1e9, 2),
            "streaming": {"what": "pinned host ring of %d distinct stereo pairs -> upload context (async H2D of %d-frame "
                                  "batches into the idle one of two frame stores) -> detect+describe x2 + match -> per-pair "
                                  "match counts read back per batch" % (len(ring), Bu),
                          "stereo_frames": n_batches * Bu, "timed_region_s": round(dt, 3),
                          "h2d_gbps_copy_alone": round(n_copy * batch_bytes / dt_copy / 1e9, 2),
                          "frames_per_s_copy_alone": round(copy_only_fps, 1),
                          "bound": "pcie (host->device copy)" if fps > 0.85 * copy_only_fps else "kernels",
                          "outputs_equal_resident_run": bool(ok)}}


def ba_algorithmic_bytes(d, s_doubles):
    """SURVEY.md 8(d), one LM iteration: n_obs * (16 uv + 8 idx) + n_lm * 24 + n_cam * 56 + 128 intrinsics in; the reduced
    system as the solver stores it (s_doubles) + its right-hand side + (P^-1, b) per landmark (96 B) out."""
    n_obs, n_lms, n_cams = len(d["obs_cam"]), len(d["points"]), len(d["poses"])
    n = 6 * int((d["cam_fixed"] == 0).sum())
    return n_obs * 24 + n_lms * 24 + n_cams * 56 + 128 + 8 * s_doubles + 8 * n + 96 * n_lms


def ba_traffic(workload, kernels):
    """(bytes per LM iteration over `kernels`, per-kernel bytes, source) from the newest committed
    profiles/r*_ba_pmc_traffic.json (tools/ba_pmc.sh: FETCH_SIZE x 2 + WRITE_SIZE, separate --pmc passes)."""
    try:
        newest = sorted((ROOT / "profiles").glob("r*_ba_pmc_traffic.json"))[-1]
        w = json.loads(newest.read_text())["workloads"][workload]
        per = {}
        for k, v in w["kernels"].items():
            base = k.split("<")[0]
            if base in kernels and "<true" not in k:   # (<true, .> is the once-per-solve scaling pass of the Schur kernel)
                per[base] = per.get(base, 0) + v["bytes_per_dispatch"]
        src = ("profiles/%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same problem, committed with the "
               "tree -- NOT collected in this run" % newest.name)
        return w.get("bytes_per_iteration_measured"), per, src
    except Exception:
        return None, {}, None


def global_ba_multi_rank(args, vsl, ctx, synth, vdist, rank, world, backend):
    """BASELINE configs[4] over `world` ranks: the one place the path has a real exchange step.  Every
    rank linearises and Schur-reduces its landmark range, ONE packed SUM all-reduce per LM iteration carries the band of
    the reduced camera system (RCCL over xGMI with backend nccl; gloo through host memory in rehearsals), every rank
    solves it redundantly.  Replaces the single ceres::Solve of global_bundle_adjustment
    (include/visnav/loop_closure_utils.h:672-748).  Called by ALL ranks; returns the dict on every rank."""
    import torch
    ba_dist = importlib.import_module("visual_slam_amd.ba_dist")
    ddev = "cuda" if backend == "nccl" else "cpu"
    dg = synth.ba_problem(5, n_kf=args.gba_kf, n_lms=args.gba_lms, loop_radius=200.0 * args.gba_kf / 500.0, max_range=15.0)

    def mk_g():
        return vsl.BaArrays.from_dict(dg)

    ba_dist.bundle_adjust_distributed(vsl, ctx, mk_g(), max_iters=1)   # warm-up: allocations, code objects, communicator
    times = {}
    own = {}
    last = None
    for iters in (3, 12, 3, 12):  # best of two per length (the one-off set-up jitters by a few ms)
        a = mk_g()
        vdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sg = ba_dist.bundle_adjust_distributed(vsl, ctx, a, max_iters=iters)
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0
        vdist.barrier()
        dt = vdist.max_over_ranks(time.perf_counter() - t0, device=ddev)   # MAX over ranks
        if iters not in times or dt < times[iters][0]:
            times[iters] = (dt, sg.iterations)
            own[iters] = mine
        last = (sg, a)
    (t3, i3), (t12, i12) = times[3], times[12]
    per_rank = vdist.gather_over_ranks((own[12] - own[3]) / max(i12 - i3, 1), device=ddev)
    s_elems, banded, bw = ctx.last_ba_layout()
    n_red = 6 * int((dg["cam_fixed"] == 0).sum())
    # the world-1 reference: every rank solves the whole problem alone (no collective) -- same LM trajectory expected
    a1 = mk_g()
    s1 = ba_dist.bundle_adjust_distributed(vsl, ctx, a1, max_iters=12, solo=True)
    sg, a = last
    return {"workload": "%d cameras (%d fixed), %d landmarks, %d observations; reduced system %d x %d, %s"
                        % (len(dg["poses"]), int(dg["cam_fixed"].sum()), len(dg["points"]), len(dg["obs_cam"]), n_red, n_red,
                           ("%sband form, half bandwidth %d" % ("cyclic " if banded == 2 else "", bw)) if banded else "dense"),
            "world": world, "backend": backend + (" (RCCL over xGMI)" if backend == "nccl" else " (host memory: a rehearsal, not xGMI)"),
            "partition": "landmarks in contiguous ranges balanced by observation count, poses replicated; every rank factorises "
                         "the all-reduced system redundantly",
            "ms_per_lm_iteration_marginal": round(1e3 * (t12 - t3) / max(i12 - i3, 1), 3),
            "per_rank_ms_per_iteration": [round(1e3 * t, 3) for t in per_rank],
            "ms_total_12_iterations_incl_setup": round(1e3 * t12, 1), "iterations": i12,
            "allreduce_bytes_per_iteration": int(8 * (s_elems + 3 * n_red + 2)),
            "collectives_per_iteration": "1 SUM of [S band | rhs | diag H | g_c | cost] + 1 SUM of 8 scalars (+ 1 scalar MAX after an accepted step)",
            "final_cost": sg.final_cost, "final_cost_world1": s1.final_cost,
            "final_cost_rel_diff_vs_world1": abs(sg.final_cost - s1.final_cost) / s1.final_cost,
            "iterations_world1": s1.iterations,
            "max_pose_diff_vs_world1": float(np.abs(a.poses - a1.poses).max())}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def write_orb_shaped_vocabulary(synth, path):
    """k = 10, L = 6 (1,111,111 nodes, 1,000,000 words): the SHAPE of ORBvoc.txt, which the reference loads
    (TemplatedVocabulary.h:1338-1424) and which is a missing blob in its tree; the tree itself is synthetic."""
    if not os.path.exists(path):
        tmp = "%s.%d.tmp" % (path, os.getpid())
        synth.write_vocabulary_text(tmp, 10, 6, *synth.vocabulary_arrays(7, 10, 6))
        os.replace(tmp, path)   # atomically: a half-written file is never picked up by a later run
    return path


def bow_measurement(vsl, ctx, synth, ring, voc_path, orc=None):
    """K8 / K9 at the reference's vocabulary shape: `transform` of the ORB descriptors of one image
    (TemplatedVocabulary.h:1127-1259) and the L1 `score` (ScoringObject.cpp:23-68) of one query against M keyframe vectors
    held in the device-resident database, M = 100 / 1,000 / 10,000.  Device times from HIP events on the context's
    stream; bytes are SURVEY 8(d)'s: transform = 32 n in + visited nodes n L k 32 B + 12 nnz out; score = 12 (q + sum c)
    in + 8 M out."""
    t0 = time.perf_counter()
    voc = ctx.load_vocabulary(voc_path)
    load_s = time.perf_counter() - t0
    k, L, n_nodes, n_words = voc.info()
    descs, vecs = [], []
    for i in range(16):
        d = ctx.orb_detect_describe(ring[(37 * i) % len(ring)][0], NUM_FEATURES)[-1]
        descs.append(d)
        vecs.append(voc.transform(d, 4)[:2])
    n_desc = len(descs[0])
    ctx.synchronize()
    ctx.set_profiling(True)
    for _ in range(5):
        voc.transform(descs[0], 4)
    ctx.reset_profiling()
    t0 = time.perf_counter()
    reps = 50
    for _ in range(reps):
        voc.transform(descs[0], 4)
    wall_ms = 1e3 * (time.perf_counter() - t0) / reps
    st = ctx.stage_ms()["bow_transform"]
    t_ms = st[0] / st[1]
    t_bytes = 32 * n_desc + n_desc * L * k * 32 + 12 * len(vecs[0][0])
    out = {"vocabulary": {"k": k, "L": L, "nodes": n_nodes, "words": n_words, "source": "synthetic tree of the ORBvoc.txt shape "
                          "(the file is a missing blob of the reference)", "text_load_s": round(load_s, 3)},
           "transform": {"descriptors": n_desc, "nnz": len(vecs[0][0]), "levelsup": 4, "device_ms": round(t_ms, 5),
                         "host_call_ms": round(wall_ms, 4), "algorithmic_bytes": t_bytes,
                         "achieved_gbs": round(t_bytes / (t_ms * 1e-3) / 1e9, 2),
                         "frac_of_hbm_peak": round(t_bytes / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                         "bound": "latency (7 dependent round trips of the descent + a single-workgroup sort and the ordered "
                                  "L1 norm: 1500 dependent fp64 additions)"},
           "score_batch": []}
    db = vsl.BowDatabase(ctx, cap_entries=16 * 1600 * 700, cap_vectors=10240)
    pool = vecs[1:]
    for i in range(10000):
        ids, vals = pool[i % len(pool)]
        db.append(ids, vals)
    q = vecs[0]
    for M in (100, 1000, 10000):
        db.score(q[0], q[1], m=M)
        ctx.reset_profiling()
        t0 = time.perf_counter()
        for _ in range(10):
            sc = db.score(q[0], q[1], m=M)
        wall = 1e3 * (time.perf_counter() - t0) / 10
        st = ctx.stage_ms()["bow_score"]
        ms = st[0] / st[1]
        total = sum(len(pool[i % len(pool)][0]) for i in range(M))
        nbytes = 12 * (len(q[0]) + total) + 8 * M
        row = {"M": M, "candidate_words": total, "device_ms": round(ms, 5), "host_call_ms": round(wall, 4),
               "algorithmic_bytes": nbytes, "achieved_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1),
               "frac_of_hbm_peak": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)}
        if orc is not None:   # the oracle beside it: pairwise L1 scores, one core, on a bounded sample of the candidates
            n_cpu = min(M, 300)
            t0 = time.perf_counter()
            exp = [orc.bow_score_l1(q[0], q[1], *pool[i % len(pool)]) for i in range(n_cpu)]
            row["cpu_oracle_ms_extrapolated"] = round(1e3 * (time.perf_counter() - t0) / n_cpu * M, 2)
            row["scores_equal_oracle"] = bool(np.array_equal(np.asarray(exp), sc[:n_cpu]))
        out["score_batch"].append(row)
    ctx.set_profiling(False)
    # HBM traffic of these kernels from the newest committed PMC passes (tools/bow_pmc.sh: FETCH_SIZE x 2 + WRITE_SIZE,
    # the calibration of profiles/rNN_pmc_traffic.json), taken on the same vocabulary and descriptor counts
    try:
        pm = json.loads(sorted((ROOT / "profiles").glob("r*_bow_pmc_traffic.json"))[-1].read_text())["kernels"]
        out["transform"]["traffic"] = pm["bow_descend_kernel"]["bytes_largest_dispatch"] + pm["bow_assemble_kernel"]["bytes_largest_dispatch"]
        out["score_batch"][-1]["traffic"] = pm["bow_score_lds_kernel"]["bytes_largest_dispatch"]
    except Exception:
        pass
    if orc is not None:
        t0 = time.perf_counter()
        ov = orc.Vocabulary(voc_path)
        out["vocabulary"]["cpu_oracle_text_load_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        for _ in range(5):
            o = ov.transform(descs[0], 4)
        out["transform"]["cpu_oracle_ms"] = round(1e3 * (time.perf_counter() - t0) / 5, 3)
        g = voc.transform(descs[0], 4)
        out["transform"]["equal_oracle"] = bool(all(np.array_equal(a, b) for a, b in zip(o, g)))
        del ov
    db.close()
    voc.close()
    return out


def device_accounting(e2e_run):
    """us per frame against the device work behind it.  Launch counts and kernel time per frame come from
    the newest committed rocprofv3 --kernel-trace --stats summary of `slam_headless --fused` on the same sequence and
    flags (profiles/rNN_e2e_kernel_stats.json, written by tools/e2e_profile.sh); the wall figure is this run's."""
    try:
        newest = sorted((ROOT / "profiles").glob("r*_e2e_kernel_stats.json"))[-1]
        pm = json.loads(newest.read_text())
    except Exception:
        return None
    return {"source": "profiles/" + newest.name, "frames_profiled": pm.get("frames"),
            "kernel_launches_per_frame": pm.get("kernel_launches_per_frame"),
            "memcpy_calls_per_frame": pm.get("memcpy_calls_per_frame"),
            "sum_kernel_us_per_frame": pm.get("sum_kernel_us_per_frame"),
            "wall_us_per_frame_this_run": round(1e3 * e2e_run["ms_per_frame"], 1),
            "launch_floor_us_per_frame": pm.get("launch_floor_us_per_frame"),
            "note": pm.get("note")}


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks through torch.distributed.run (one process per
    GPU, rendezvous on 127.0.0.1) as a CHILD process -- this process has not touched the GPU -- and exit with its code.
    The ranks' stdout (rank 0's JSON line) and stderr pass through."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.run(cmd, env=env).returncode


def rehearse_plumbing(args, vdist, rank, world):
    """--rehearse-plumbing: everything around the hot path (rank set-up, barriers, MAX-over-ranks timing, per-rank
    list, rank 0's single JSON line) with a step that only sleeps.  Not a measurement: value is null."""
    backend = os.environ.get("VSL_BENCH_BACKEND", "gloo")
    if backend != "gloo":
        raise SystemExit("--rehearse-plumbing runs without a GPU: set VSL_BENCH_BACKEND=gloo")
    vdist.init(backend)
    for _ in range(args.warmup):
        time.sleep(0.001)
    vdist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (1 + rank))   # rank r is the slower one: the straggler must show in the list
    own = time.perf_counter() - t0
    vdist.barrier()
    elapsed = vdist.max_over_ranks(time.perf_counter() - t0)
    per_rank = vdist.gather_over_ranks(own)
    if rank == 0:
        print(json.dumps({"metric": "REHEARSAL of the benchmark plumbing -- no GPU work, not a measurement", "value": None,
                          "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * elapsed / max(args.steps, 1), 4), "rehearsal": True,
                          "per_rank_ms_per_step": [round(1e3 * t / max(args.steps, 1), 4) for t in per_rank]}), flush=True)
    vdist.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="distinct stereo frames resident in HBM per GPU (one pass)")
    ap.add_argument("--passes", type=int, default=18,
                    help="passes over the resident batch per step (18 x 1024 frames ~ 62 ms: 20 steps > 1.2 s of sustained clocks)")
    ap.add_argument("--streams", type=int, default=2,
                    help="HIP streams the batch is split over (512 frames = 1024 images per launch)")
    ap.add_argument("--scenes", type=int, default=64,
                    help="distinct synthetic scenes per rank; batch / scenes sensor-noise realisations of each, so every "
                         "resident stereo pair is distinct")
    ap.add_argument("--gen-workers", type=int, default=8, help="processes generating the synthetic frames (before GPU init)")
    ap.add_argument("--cpu-frames", type=int, default=600, help="stereo frames of the CPU-baseline sample (0 = skip)")
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--diag", action="append", default=[], help="name=value knob for vsl_ctx_set_diagnostic (repeatable; tuning experiments)")
    ap.add_argument("--clock-ramp-ms", type=float, default=80.0,
                    help="set-up: run passes for this long before the warm-up steps (the chip's clock ramps up from idle)")
    ap.add_argument("--stream-seconds", type=float, default=1.5,
                    help="N = 1: length of the upload-inclusive streaming measurement (0 = skip)")
    ap.add_argument("--no-ba", dest="ba", action="store_false", help="skip the local-BA ms/iter measurement")
    ap.add_argument("--no-gba", dest="gba", action="store_false",
                    help="skip the global-BA ms/iter measurement (BASELINE configs[4] scale, one rank)")
    ap.add_argument("--gba-timeout", type=float, default=600.0, help="watchdog of the multi-rank global-BA leg, seconds")
    ap.add_argument("--gba-kf", type=int, default=500, help="keyframes of the global-BA problem (configs[4]: 500 = 1000 cameras)")
    ap.add_argument("--gba-lms", type=int, default=100000, help="landmark candidates of the global-BA problem (configs[4]: 100000)")
    ap.add_argument("--no-e2e", dest="e2e", action="store_false",
                    help="skip the single-stream end-to-end run of the headless next_step pipeline")
    ap.add_argument("--no-e2e-natural", dest="e2e_natural", action="store_false",
                    help="skip the natural-loop leg (a second rendered lap, larger room, reference defaults only)")
    ap.add_argument("--e2e-frames", type=int, default=640, help="frames of the rendered lap of the end-to-end legs")
    ap.add_argument("--e2e-step", type=float, default=0.03, help="metres per frame along the circle")
    ap.add_argument("--e2e-look", type=float, default=90.0,
                    help="viewing direction relative to the path tangent, degrees (90: towards the nearest wall -- close structure)")
    ap.add_argument("--e2e-radius", type=float, default=2.674,
                    help="circle radius: 2 pi r / step = 560 frames per lap, so the revisit is > loop_closing_time (500) frames later")
    ap.add_argument("--no-bow", dest="bow", action="store_false", help="skip the BoW transform / score measurement (k = 10, L = 6 vocabulary)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline figure: streaming mode, per-stage times and "
                         "rooflines, CPU baseline and oracle check, BA / pose graph / BoW / end-to-end legs, and the "
                         "multi-rank global BA for N > 1 (the --no-* and leg options apply to these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (float32 / float64, a few MB)")
    ap.add_argument("--rehearse-plumbing", action="store_true",
                    help="NO GPU work: the launcher / rank / timing / JSON plumbing with a sleeping step (CPU tests of "
                         "--gpus N; set VSL_BENCH_BACKEND=gloo).  The line says so and carries no value.")
    args = ap.parse_args()

    # --gpus N means N ranks, one per GPU.  Under a launcher (WORLD_SIZE set) the two must agree; without one the
    # script launches the ranks itself -- BEFORE anything in this process touches the GPU -- and relays rank 0's line.
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus))
    vsl = entry.load_package()
    synth = importlib.import_module("visual_slam_amd.synth")
    vdist = importlib.import_module("visual_slam_amd.dist")
    rank, world, local_rank = vdist.env_rank_world()
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d; launch as: python -m torch.distributed.run --nnodes=1 "
                         "--nproc-per-node %d --master-addr 127.0.0.1 --master-port <port> bench.py --gpus %d ... "
                         "(or plain `python bench.py --gpus %d`, which starts the ranks itself)"
                         % (args.gpus, world, args.gpus, args.gpus, args.gpus))
    if args.rehearse_plumbing:
        return rehearse_plumbing(args, vdist, rank, world)
    B, S, P = args.batch, args.streams, max(1, args.passes)
    if S < 1 or B % S:
        raise SystemExit("--batch must be a multiple of --streams")
    n_scenes = min(args.scenes, B)
    if B % n_scenes:
        raise SystemExit("--batch must be a multiple of --scenes")
    Bu = B // S          # stereo frames per launch
    n_img = 2 * Bu       # images per launch

    # Synthetic input, generated before anything touches the GPU (forked workers): B distinct stereo pairs per rank
    t_gen = time.perf_counter()
    # (cached under /tmp: profiler passes re-run this script many times, and a process that rocprofv3 has already
    # attached the GPU runtime to must not fork workers -- tools/refresh_profiles.sh passes --gen-workers 1)
    # The name carries a hash of the generator's source and of the seed list: a file written by an older synth.py or
    # for other seeds is never reused.
    import hashlib
    seeds = vdist.stream_seeds(rank, n_scenes)
    gen_id = hashlib.sha256((ROOT / "visual-slam_amd" / "synth.py").read_bytes() + repr((seeds, B // n_scenes, SYNTH_MARGIN, W, H)).encode()).hexdigest()[:16]
    cache = Path("/tmp") / ("vsl_bench_frames_r%d_s%d_b%d_m%d_%s.npy" % (rank, n_scenes, B, SYNTH_MARGIN, gen_id))
    host_frames = None
    if cache.exists():
        try:
            host_frames = np.load(cache)
            if host_frames.shape != (B, 2, H, W):
                host_frames = None
        except Exception:
            host_frames = None
    if host_frames is None:
        host_frames = distinct_stereo_frames(seeds, B // n_scenes, args.gen_workers)
        try:
            np.save(cache, host_frames)
        except Exception:
            pass
    # interleave the scenes so that every launch (and the CPU sample) sees all of them
    host_frames = np.ascontiguousarray(host_frames.reshape(n_scenes, B // n_scenes, 2, H, W).transpose(1, 0, 2, 3, 4)).reshape(B, 2, H, W)
    t_gen = time.perf_counter() - t_gen

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # one rank per GPU; `% device_count` only matters when several ranks rehearse on a one-GPU box
    local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    backend = os.environ.get("VSL_BENCH_BACKEND", "nccl")  # nccl = RCCL over xGMI; "gloo" for rehearsals
    vdist.init(backend)  # a no-op at world size 1

    # the pinned host ring of the streaming mode doubles as the upload source of the resident batch
    pinned = torch.empty((B, 2, H, W), dtype=torch.uint8).pin_memory()
    ring = pinned.numpy()
    ring[...] = host_frames
    del host_frames
    slot_pairs = np.array([[2 * k, 2 * k + 1] for k in range(Bu)], np.int32)
    units = []  # one (stream, context, frame store) per HIP stream; inputs resident in HBM before the timed region
    for u in range(S):
        stream = torch.cuda.Stream()
        ctx = vsl.Context(local_rank, stream=stream.cuda_stream)
        for kv in args.diag:  # tuning / diagnostic knobs of the library (vsl_ctx_set_diagnostic), e.g. --diag k1_extra_lds=8192
            ctx.set_diagnostic(kv.split("=")[0], int(kv.split("=")[1]))
        frames = vsl.Frames(ctx, n_img, W, H, NUM_FEATURES, max_pairs=Bu)
        frames.upload(0, ring[u * Bu:(u + 1) * Bu].reshape(n_img, H, W))
        units.append((stream, ctx, frames))

    def one_pass():
        for _, _, frames in units:
            frames.detect_describe(0, n_img, NUM_FEATURES, True)
        for _, _, frames in units:
            frames.resolve_ties()
            frames.match(slot_pairs, 70, 1.2)

    def step():
        for _ in range(P):
            one_pass()

    def barrier():
        vdist.barrier()
        torch.cuda.synchronize()

    # Set-up, before the W warm-up steps: wake the device.  After idle the chip's clock ramps for ~50 ms and the
    # kernels of that window run up to 15 % slower (profiles/r01_bench_kernel_trace_summary.txt).  Reported in `config`.
    t_ramp = time.perf_counter()
    while 1e3 * (time.perf_counter() - t_ramp) < args.clock_ramp_ms:
        one_pass()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0     # this rank's own K steps (before waiting for the others)
    barrier()
    ddev = "cuda" if backend == "nccl" else "cpu"
    elapsed = vdist.max_over_ranks(time.perf_counter() - t0, device=ddev)
    per_rank_s = vdist.gather_over_ranks(own_elapsed, device=ddev)

    counts = [frames.counts(n_img, Bu) for _, _, frames in units]
    # the resident run's OUTPUTS for the frames the CPU baseline will redo (rank 0, N = 1): keypoints, descriptors, matches
    sample_out = []
    if args.full and rank == 0 and world == 1 and args.cpu_frames > 0:
        for nfr in range(min(args.cpu_frames, B)):
            fr = units[nfr // Bu][2]
            k = nfr % Bu
            kl, kr = fr.keypoints(2 * k), fr.keypoints(2 * k + 1)
            sample_out.append((kl[0], kl[2], kr[0], kr[2], fr.matches(k)))
    nk = np.concatenate([c[0] for c in counts])
    nm = np.concatenate([c[1] for c in counts])
    ctx, frames = units[0][1], units[0][2]
    if not (nk.min() > 0 and nm.min() > 0):
        raise SystemExit("benchmark produced empty outputs: keypoints %s matches %s" % (nk.min(), nm.min()))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, units, counts, B, Bu)

    out = None
    if rank == 0:
        value = world * B * P * args.steps / elapsed
        out = {
            "metric": "stereo frames/sec, detect+describe (1500 feats) + stereo match, 752x480",
            "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/f32/f64",
            "data": "synthetic",
            # every rank's own rate over the same K steps (weak scaling: each rank runs the same work; a straggler shows here)
            "per_rank": {"frames_per_s": [round(B * P * args.steps / t, 1) for t in per_rank_s],
                         "min": round(B * P * args.steps / max(per_rank_s), 1), "max": round(B * P * args.steps / min(per_rank_s), 1)},
            "config": {"workload": "synthetic 752x480 stereo, 1500 feats/frame (BASELINE configs[1]); "
                                   "independent streams per GPU (configs[3])",
                       "value_is": "kernel pipeline: inputs resident in HBM when the timed region starts, outputs stay "
                                   "in HBM (the upload-inclusive rate is value_incl_upload)",
                       "inputs_resident_in_hbm": True, "h2d_in_timed_region": False,
                       "distinct_stereo_pairs_per_gpu": B, "distinct_scenes_per_gpu": n_scenes,
                       "stereo_frames_per_pass_per_gpu": B, "passes_per_step": P,
                       "stereo_frames_per_step_per_gpu": B * P, "timed_region_s": round(elapsed, 3),
                       "hip_streams": S, "stereo_frames_per_launch": Bu,
                       "clock_ramp_ms_before_warmup": args.clock_ramp_ms,
                       "num_features": NUM_FEATURES,
                       "match": "threshold 70, ratio 1.2, cross-check",
                       "mean_keypoints_per_image": round(float(nk.mean()), 1),
                       "mean_matches_per_pair": round(float(nm.mean()), 1),
                       "synthetic_input_generation_s": round(t_gen, 2)},
        }

    # ---- everything below the headline figure: --full only
    if args.full and rank == 0:
        # ---- streaming mode (N = 1): the same hot path fed from the pinned host ring, upload inside the timed region
        if args.stream_seconds > 0 and world == 1 and S >= 2:
            out.update(streaming_measurement(vsl, units, ring, Bu, slot_pairs, args.stream_seconds, local_rank,
                                             [c[1] for c in counts]))

        # ---- per-stage device time, HIP events around every stage on the stream each kernel is launched on.
        # Pass 1: one stream at a time (kernel durations in isolation -> roofline); pass 2: all streams active
        # as in the timed region (durations stretch because kernels of different streams share the CUs).
        def staged(fn):
            # (the phases before this one end in host work: let the clocks ramp again -- ~50 ms after idle -- before the
            # profiled passes, as the timed region does; without it the first launches read ~15 % long)
            t_ramp = time.perf_counter()
            while time.perf_counter() - t_ramp < 0.12:
                fn()
            for _, c, _ in units:
                c.synchronize()
                c.set_profiling(True)
                c.reset_profiling()
            for _ in range(max(1, args.profile_steps)):
                fn()
            tot = {}
            for _, c, _ in units:
                for k, (ms, n) in c.stage_ms().items():
                    a = tot.setdefault(k, [0.0, 0])
                    a[0] += ms
                    a[1] += n
                c.set_profiling(False)
            return {k: ms / n for k, (ms, n) in tot.items() if n > 0}   # average per launch (Bu frames)

        def step_one_stream_at_a_time():
            for _, c, fr in units:
                fr.detect_describe(0, n_img, NUM_FEATURES, True)
                fr.resolve_ties()
                fr.match(slot_pairs, 70, 1.2)
                c.synchronize()

        stages = staged(step_one_stream_at_a_time)
        stages_overlapped = staged(one_pass) if S > 1 else None
        dom = max(stages, key=stages.get)
        # counts for the byte model: read back once (unit 0 = one launch)
        kp_total, match_total = int(counts[0][0].sum()), int(counts[0][1].sum())
        cand_total = int(frames.candidate_counts(n_img).sum())
        out["config"]["mean_candidates_per_image"] = round(cand_total / n_img, 1)
        ab = stage_algorithmic_bytes(dom, n_img, Bu, kp_total, cand_total, match_total)
        achieved = ab / (stages[dom] * 1e-3) / 1e9
        # HBM traffic of that kernel per launch from the newest committed rocprofv3 PMC passes (FETCH_SIZE and
        # WRITE_SIZE in separate passes, corrected as MI355X_MICROARCH.md prescribes -- see the file's note); only
        # valid for the launch size it was taken at
        traffic, traffic_source = None, None
        try:
            newest = sorted((ROOT / "profiles").glob("r*_pmc_traffic.json"))[-1]
            pm = json.loads(newest.read_text())
            if pm.get("batch_stereo_frames") == Bu and dom in pm["kernels"]:
                traffic = pm["kernels"][dom].get("bytes_per_launch", pm["kernels"][dom].get("bytes_per_launch_uncorrected"))
                traffic_source = ("profiles/%s: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this kernel at this launch "
                                  "size, committed with the tree -- NOT collected in this run (PMC passes cannot share a "
                                  "process with the timed loop)" % newest.name)
        except Exception:
            traffic, traffic_source = None, None
        out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                           "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                           "traffic_source": traffic_source,
                           "algorithmic_bytes_per_launch": int(ab),
                           "algorithmic_bytes_are": "SURVEY 8(d) detect+angle+describe: image in + 56 B per keypoint out, "
                                                    "x %d images per launch" % n_img,
                           "avg_launch_ms": round(stages[dom], 5)}
        # the whole keypoint stage (K1 + selection + describe) and the whole pass against the same HBM peak
        dd_ms = sum(stages.get(k, 0.0) for k in ("response", "select", "describe"))
        if dd_ms > 0:
            out["roofline_detect_describe_stage"] = {
                "bound": "hbm", "achieved": round(ab / (dd_ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ab / (dd_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "sum_of_kernel_ms": round(dd_ms, 5)}
        pass_bytes = B * (2 * W * H + 2 * 56 * NUM_FEATURES + 2 * 32 * NUM_FEATURES + 8 * NUM_FEATURES)  # 8(d): 997,920 B per stereo frame
        out["roofline_whole_pass"] = {"bound": "hbm", "achieved": round(pass_bytes * P * args.steps / elapsed / 1e9, 2),
                                      "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": round(pass_bytes * P * args.steps / elapsed / 1e9 / HBM_PEAK_GBS, 5),
                                      "algorithmic_bytes_per_stereo_frame": pass_bytes // B}
        # the matcher is the one matrix-core kernel: ALGORITHMIC multiply-adds = ONE n_a x n_b distance matrix of 256 bits
        # per pair (convention since round 3: the reverse pass over the ~1/3 of the columns that need the cross-check and
        # the padding of the 256-query x 64-row tiles are the kernel's own overhead, not algorithmic work; rounds 1-2
        # counted both directions, i.e. twice this) against the dense peak of the instruction it runs on (block-scaled
        # FP4, v_mfma_scale_f32_32x32x64_f8f6f4, for <= 2048 features per image)
        if "match" in stages:
            nk0 = counts[0][0].astype(np.int64)
            macs = 0
            for k in range(Bu):
                a, b = int(nk0[2 * k]), int(nk0[2 * k + 1])
                macs += a * b * 256
            tops = 2.0 * macs / (stages["match"] * 1e-3) / 1e12
            out["roofline_matcher"] = {"bound": "mfma", "kernel": "match", "instruction": "fp4 block-scaled MFMA (unit scales, exact on bits)",
                                       "algorithmic_macs_are": "n_a x n_b x 256 per pair, once (rounds 1-2 priced both directions: 2x)",
                                       "achieved": round(tops, 1), "peak": FP4_PEAK_TOPS, "unit": "TOP/s",
                                       "frac": round(tops / FP4_PEAK_TOPS, 4), "frac_of_int8_peak": round(tops / I8_PEAK_TOPS, 4),
                                       "avg_launch_ms": round(stages["match"], 5)}
        out["stage_ms_per_launch"] = {k: round(v, 5) for k, v in stages.items()}
        if stages_overlapped:
            out["stage_ms_per_launch_streams_overlapped"] = {k: round(v, 5) for k, v in stages_overlapped.items()}

        # ---- CPU baseline: the oracle (port of the reference path), 1 core, bounded sample of the same frames,
        # starting from host images like the reference does -- compared like for like with the upload-inclusive rate
        if args.cpu_frames > 0 and world == 1:   # the CPU baseline is an N = 1 measurement
            orc = entry.load_oracle()
            t0 = time.perf_counter()
            n_done = 0
            cpu_results = []
            while n_done < args.cpu_frames:
                left, right = ring[n_done % B]
                x1, _, d1 = orc.detect_describe(left, NUM_FEATURES, True)
                x2, _, d2 = orc.detect_describe(right, NUM_FEATURES, True)
                mm = orc.match_descriptors(d1, d2, 70, 1.2)
                if n_done < len(sample_out):
                    cpu_results.append((x1, d1, x2, d2, mm))
                n_done += 1
            cpu_s = time.perf_counter() - t0
            # the benchmark checks itself: the timed GPU run's keypoints, descriptors and match lists of these very
            # frames against the oracle's (outside the timed loop above)
            n_equal = 0
            for got, exp in zip(sample_out, cpu_results):
                n_equal += int(all(np.array_equal(np.asarray(g), np.asarray(e)) for g, e in zip(got, exp)))
            out["outputs_equal_oracle_sample"] = {"frames_compared": len(cpu_results), "frames_equal": n_equal,
                                                  "all_equal": bool(cpu_results) and n_equal == len(cpu_results),
                                                  "what": "keypoint positions, 256-bit descriptors (both images) and the ordered "
                                                          "stereo match list of the timed resident run vs the oracle, bit for bit"}
            out["cpu_baseline"] = {"value": round(n_done / cpu_s, 3), "unit": "frames/s", "cores": 1,
                                   "kind": "port", "cpu_model": cpu_model(), "host_cores_available": os.cpu_count(),
                                   "sample": "the first %d of the %d distinct synthetic stereo frames of the run, oracle "
                                             "detect+describe x2 + match from host images, single thread (the "
                                             "reference's keypoints.h path has no parallel loops), %.1f s"
                                             % (n_done, B, cpu_s)}
            if "value_incl_upload" in out:
                out["speedup_vs_cpu_1core_incl_upload"] = round(out["value_incl_upload"] / out["cpu_baseline"]["value"], 1)
        # ---- second metric of BASELINE.json: ms per LM iteration of local bundle adjustment
        # (configs[2]: 7 keyframes = 14 cameras, ~20k landmarks), GPU next to the oracle on all host cores
        if args.ba and world == 1:
            d = synth.ba_problem(4, n_kf=7, n_lms=20000)
            orc = entry.load_oracle()
            mk = lambda: vsl.BaArrays.from_dict(d)  # noqa: E731
            ctx.bundle_adjust(mk(), max_iters=2)  # warm-up (allocations, code objects)
            ctx.synchronize()
            a = mk()
            t0 = time.perf_counter()
            sg = ctx.bundle_adjust(a, max_iters=20)
            gpu_ms = 1e3 * (time.perf_counter() - t0)
            # the per-kernel device times come from a second, profiled run (HIP events on the solver's stream around every
            # launch): the events cost ~60 us per LM iteration, so the timed run above goes without them
            ctx.reset_profiling()
            ctx.set_profiling(1)
            sp = ctx.bundle_adjust(mk(), max_iters=20)
            stg = ctx.stage_ms()
            ctx.set_profiling(0)
            ncpu = os.cpu_count() or 1
            b = orc.BaArrays(d["poses"], d["cam_fixed"], d["cam_intr"], d["intr"], d["points"], d["obs_cam"], d["obs_lm"],
                             d["obs_uv"], d["cam_model"])   # the oracle's own holder: the cpu_baseline leg
            t0 = time.perf_counter()
            sc = orc.bundle_adjust(b, max_iters=20, threads=ncpu)
            cpu_ms = 1e3 * (time.perf_counter() - t0)
            n_red = 6 * int((d["cam_fixed"] == 0).sum())
            alg = ba_algorithmic_bytes(d, n_red * n_red)
            knames = {"ba_schur": "baf_schur_kernel", "ba_finish": "baf_finish_kernel", "ba_solve": "baf_chol_kernel",
                      "ba_step": "baf_step_kernel+baf_decide_kernel"}
            kms = {knames[k]: stg[k][0] / stg[k][1] for k in knames if stg.get(k, (0, 0))[1] > 0}
            dom = max(kms, key=kms.get) if kms else None
            it_ms = sum(kms.values())
            tr_iter, tr_k, tr_src = ba_traffic("local7", {kk for k in kms for kk in k.split("+")})
            out["local_ba"] = {"workload": "7 keyframes (14 cameras, 2 fixed), %d landmarks, %d observations, "
                                           "Huber 1.0, <= 20 LM iterations" % (len(d["points"]), len(d["obs_cam"])),
                               "iterations": sg.iterations, "ms_per_iter": round(gpu_ms / max(sg.iterations, 1), 4),
                               "ms_total_incl_upload": round(gpu_ms, 3),
                               "launches_per_iteration": len(kms) + 1, "host_syncs_per_iteration": 0,
                               "loop": "the Levenberg-Marquardt decision is taken on the device (baf_decide_kernel); the host "
                                       "enqueues iterations one ahead of the decision it has polled from pinned memory",
                               "kernel_ms_per_launch": {k: round(v, 5) for k, v in kms.items()},
                               "device_ms": {"linearize": round(sp.linearize_ms, 3), "schur": round(sp.schur_ms, 3),
                                             "solve": round(sp.solve_ms, 3)},
                               "final_cost_rel_diff_vs_oracle": abs(sg.final_cost - sc.final_cost) / sc.final_cost,
                               "cpu_oracle_ms_per_iter": round(cpu_ms / max(sc.iterations, 1), 3),
                               "cpu_threads": ncpu, "cpu_model": cpu_model()}
            if dom:
                ach = alg / (kms[dom] * 1e-3) / 1e9
                ach_it = alg / (it_ms * 1e-3) / 1e9
                out["local_ba"]["roofline"] = {
                    "bound": "hbm", "kernel": dom, "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": tr_k.get(dom), "traffic_source": tr_src,
                    "algorithmic_bytes_per_launch": int(alg), "avg_launch_ms": round(kms[dom], 5),
                    "algorithmic_bytes_are": "SURVEY 8(d), one LM iteration of THIS problem: 24 B per observation + 24 B per "
                                             "landmark + 56 B per camera + 128 in; (6C)^2 * 8 + 6C * 8 + 96 B per landmark out",
                    "whole_iteration": {"sum_of_kernel_ms": round(it_ms, 5), "achieved": round(ach_it, 2),
                                        "frac": round(ach_it / HBM_PEAK_GBS, 5), "traffic": tr_iter,
                                        "wall_ms_per_iter_incl_setup": round(gpu_ms / max(sg.iterations, 1), 4)},
                    "note": "latency-bound, not bandwidth-bound: 5.6 MB per iteration against five dependent launches; the "
                            "Schur tiles run at the fp64 matrix rate (DESIGN 8.6)"}
        # ---- global bundle adjustment at BASELINE configs[4] scale (500 keyframes = 1000 cameras, ~100k landmarks)
        # through the step-wise session API (the multi-GPU path at world size 1): marginal time per LM iteration
        if args.gba and world == 1:
            ba_dist = importlib.import_module("visual_slam_amd.ba_dist")
            dg = synth.ba_problem(5, n_kf=args.gba_kf, n_lms=args.gba_lms, loop_radius=200.0 * args.gba_kf / 500.0, max_range=15.0)

            def mk_g():
                return vsl.BaArrays.from_dict(dg)

            ba_dist.bundle_adjust_distributed(vsl, ctx, mk_g(), max_iters=1)   # warm-up: allocations, code objects
            times, loops = {}, {}
            for iters in (3, 12, 3, 12, 3, 12):  # best of three per length: the one-off host set-up (~8 ms) jitters by more than an iteration
                a = mk_g()
                ctx.synchronize()
                t0 = time.perf_counter()
                sg = ba_dist.bundle_adjust_distributed(vsl, ctx, a, max_iters=iters)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                if iters not in times or dt < times[iters][0]:
                    times[iters] = (dt, sg.iterations)
                # the solver's own clock: from the start of the LM loop (set-up done) to the downloaded result
                if iters not in loops or sg.total_ms < loops[iters]:
                    loops[iters] = sg.total_ms
            (t3, i3), (t12, i12) = times[3], times[12]
            # marginal time of an iteration from the SOLVER's clock of the two lengths (the wall-clock difference carries the
            # jitter of two host set-ups of ~8 ms each: it scattered between 0.8 and 1.4 ms for 1.21 ms of kernels)
            t12w, t3w = t12, t3
            t12, t3 = t3w + 1e-3 * (loops[12] - loops[3]), t3w
            # per-stage device time of one iteration from a profiled run (HIP events on the solver's stream)
            ctx.reset_profiling()
            ctx.set_profiling(1)
            sgp = ba_dist.bundle_adjust_distributed(vsl, ctx, mk_g(), max_iters=6)
            stg_g = ctx.stage_ms()
            ctx.set_profiling(0)
            g_iters = max(sgp.iterations, 1)
            g_dev = {k: round(stg_g[k][0] / g_iters, 4) for k in ("ba_linearize", "ba_schur", "ba_solve", "ba_step")
                     if stg_g.get(k, (0, 0))[1] > 0}
            lay0 = ctx.last_ba_layout()
            out["global_ba"] = {"workload": "%d cameras (%d fixed), %d landmarks, %d observations; reduced system %d x %d, %s; "
                                            "session API, 1 rank" % (len(dg["poses"]), int(dg["cam_fixed"].sum()), len(dg["points"]),
                                                                     len(dg["obs_cam"]), 6 * int((dg["cam_fixed"] == 0).sum()),
                                                                     6 * int((dg["cam_fixed"] == 0).sum()),
                                                                     ("%sband form, half bandwidth %d" % ("cyclic " if lay0[1] == 2 else "", lay0[2]))
                                                                     if lay0[1] else "dense"),
                               "ms_per_lm_iteration_marginal": round(1e3 * (t12 - t3) / max(i12 - i3, 1), 2),
                               "marginal_is": "(solver clock of the 12-iteration solve - of the 3-iteration solve) / 9, best of three each",
                               "ms_per_lm_iteration_marginal_wall": round(1e3 * (t12w - t3w) / max(i12 - i3, 1), 2),
                               "ms_total_12_iterations_incl_setup": round(1e3 * t12w, 1), "iterations": i12,
                               "device_ms_per_iteration": g_dev}
            lay = ctx.last_ba_layout()   # (doubles of S, banded, bandwidth) of the session just run
            if not lay[0]:
                lay = None
            if g_dev:
                n_red = 6 * int((dg["cam_fixed"] == 0).sum())
                s_doubles = lay[0] if lay else n_red * n_red
                alg_g = ba_algorithmic_bytes(dg, s_doubles)
                dom_g = max(g_dev, key=g_dev.get)
                it_ms_g = 1e3 * (t12 - t3) / max(i12 - i3, 1)
                tr_iter_g, _, tr_src_g = ba_traffic("global", set())
                ach_g = alg_g / (it_ms_g * 1e-3) / 1e9
                out["global_ba"]["roofline"] = {
                    "bound": "hbm", "kernel": {"ba_linearize": "bal_prep / bal_cam kernels, Jacobi-scaling pass (once per solve)",
                                               "ba_schur": "bal_prep / bal_cam / ba_schur_gather kernels (recompute form, ba_large.h)",
                                               "ba_solve": "block-cyclic-reduction band Cholesky (bcr_* kernels) + back-substitution",
                                               "ba_step": "bal_pose / bal_step kernels"}[dom_g],
                    "achieved": round(ach_g, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach_g / HBM_PEAK_GBS, 5),
                    "traffic": tr_iter_g, "traffic_source": tr_src_g, "algorithmic_bytes_per_launch": int(alg_g),
                    "avg_launch_ms": round(it_ms_g, 4),
                    "launch_is": "one LM iteration (a chain of ~55 kernels, ONE host round trip; the dominant stage is named in "
                                 "`kernel`, its device time in device_ms_per_iteration)",
                    "algorithmic_bytes_are": "SURVEY 8(d) with S in band storage: 24 B per observation + 24 B per landmark + "
                                             "56 B per camera + 128 in; %d doubles of S + rhs + 96 B per landmark out" % s_doubles,
                    "note": "latency- and fp64-compute-bound, not bandwidth-bound: the solve is log2(n / B) dependent levels of "
                            "dense 224-block factorisations (DESIGN 8.4)"}

        # ---- pose graph optimisation at BASELINE configs[4] scale ("loop-closure pose-graph, ~500 keyframes"): odometry +
        # covisibility edges inside a window of six keyframes + the loop edge -- the shape pose_graph_optimization builds
        # (loop_closure_utils.h:446-587); the normal equations are a narrow CYCLIC band, solved by the ring solver
        if args.gba and world == 1:
            import types
            dpg = synth.pose_graph(5, 500, 0, meas_noise=0.002, drift=0.02, window=6)

            def mk_pg():
                return types.SimpleNamespace(poses=np.ascontiguousarray(dpg["poses"], np.float64).copy(),
                                             node_fixed=np.ascontiguousarray(dpg["node_fixed"], np.uint8),
                                             edge_a=np.ascontiguousarray(dpg["edge_a"], np.int32),
                                             edge_b=np.ascontiguousarray(dpg["edge_b"], np.int32),
                                             edge_meas=np.ascontiguousarray(dpg["edge_meas"], np.float64))

            pg = {}
            for form, dense in (("band", 0), ("dense", 1)):
                ctx.set_diagnostic("ba_force_dense", dense)
                try:
                    ctx.pose_graph_optimize(mk_pg(), True, 1.0, 3)
                    best = None
                    for _ in range(3 if not dense else 1):
                        apg = mk_pg()
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        spg = ctx.pose_graph_optimize(apg, True, 1.0, 20)
                        dt = 1e3 * (time.perf_counter() - t0)
                        best = dt if best is None else min(best, dt)
                    pg[form] = (best, spg)
                finally:
                    ctx.set_diagnostic("ba_force_dense", 0)
            (tb, sb), (td, sd) = pg["band"], pg["dense"]
            out["pose_graph"] = {"workload": "500 keyframes on a loop (1 fixed), %d relative-pose edges (odometry, covisibility window 6, loop edge), "
                                             "Huber 1.0, <= 20 LM iterations; normal equations 2994 x 2994 in cyclic band storage" % len(dpg["edge_a"]),
                                 "iterations": sb.iterations, "ms_per_lm_iteration": round(tb / max(sb.iterations, 1), 3),
                                 "ms_total_incl_setup": round(tb, 2),
                                 "dense_solver_ms_per_lm_iteration": round(td / max(sd.iterations, 1), 3),
                                 "same_trajectory_as_dense": (sb.iterations, sb.termination) == (sd.iterations, sd.termination),
                                 "final_cost_rel_diff_vs_dense": abs(sb.final_cost - sd.final_cost) / max(sd.final_cost, 1e-300),
                                 "note": "the host takes the LM decision with four synchronisations per iteration (a small problem: "
                                         "~0.1 ms of kernels); the reference hands this to Ceres (SPARSE_NORMAL_CHOLESKY)"}

        # ---- BoW (K8 / K9) at the reference's vocabulary shape; the vocabulary file also serves the end-to-end legs
        voc_path = None
        if (args.bow or args.e2e) and world == 1:
            import hashlib
            # (the name carries a hash of the generator's source: a file written by an older synth.py is not reused)
            voc_path = write_orb_shaped_vocabulary(synth, "/tmp/vsl_voc_k10L6_s7_%s.txt" % hashlib.sha256(
                (ROOT / "visual-slam_amd" / "synth.py").read_bytes()).hexdigest()[:12])
        if args.bow and world == 1:
            out["bow"] = bow_measurement(vsl, ctx, synth, ring, voc_path, entry.load_oracle() if args.cpu_frames > 0 else None)

        # ---- third metric: frames/s of ONE stream through the whole per-frame pipeline, end to end (the reference's
        # next_step order) and its ATE, on a rendered EuRoC-layout LAP that revisits its start, with the reference's
        # default-ON branches: relocalisation (ui.relocalization), loop closure + pose graph + global BA (ui.loop_closure,
        # ui.GBA_after), per-keyframe compute_bow_vector on a k = 10 / L = 6 vocabulary (src/slam.cpp:244-247, :1198-1258).
        # Child processes, so that each owns its HIP context.
        exe = ROOT / "visual-slam_amd" / "slam_headless"
        cpu_exe = ROOT / "oracle" / "_cpu" / "slam_headless_cpu"   # the same application on the CPU oracle's operators
        if args.e2e and exe.exists() and world == 1:
            import subprocess
            import tempfile
            lap_frames = int(round(2 * np.pi * args.e2e_radius / args.e2e_step))
            n_frames = args.e2e_frames
            with tempfile.TemporaryDirectory(prefix="vsl_seq_") as d:
                # rendered in a fresh python process (forked render workers, no GPU state to inherit)
                t_render = time.perf_counter()
                code = ("import sys, importlib; sys.path.insert(0, %r); import __graft_entry__ as e; e.load_package(); "
                        "sq = importlib.import_module('visual_slam_amd.synth_sequence'); "
                        "sq.render_sequence(%r, n_frames=%d, seed=1, step_m=%r, radius=%r, workers=%d, look_deg=%r)"
                        % (str(ROOT), d, n_frames, args.e2e_step, args.e2e_radius, max(1, min(16, os.cpu_count() or 1)), args.e2e_look))
                subprocess.run([sys.executable, "-c", code], check=True, timeout=1500)
                t_render = time.perf_counter() - t_render
                # MAIN LEG: the reference's defaults, no test hooks.  In this room the map stays consistent over the lap
                # (ATE ~2 cm), tracking falls back onto the first lap's landmarks at the revisit and no keyframe -- hence no
                # loop candidate -- is taken there: loop DETECTION runs and is timed on every keyframe, nothing closes.
                default_flags = ["--relocalization", "--loop-closure", "--voc-path", voc_path]
                # LOOP-CLOSING STAGES LEG (labelled as such): a displaced pose estimate at frame 300 stands in for drift
                # (--inject-drift, a test hook: the second half of the lap is mapped ~0.6 m off) and the first keyframe
                # after the lap is complete is handed keyframe 0 as a consistent loop candidate (--force-loop, a test hook:
                # the 3-keyframe consistency test has no keyframes to work with there) -> compute_sim3, pose graph, global
                # BA and the merge-back run on GPU and CPU; relocalisation is off in this leg (its motion-model gate
                # rejects the injected jump)
                stage_flags = ["--loop-closure", "--voc-path", voc_path, "--inject-drift", "300:0.5,0,0.3",
                               "--force-loop", "%d:0" % max(lap_frames - 20, 1)]

                def run(binary, extra, reps):
                    if not binary.exists():
                        return {"error": "%s not built" % binary.name}
                    best = None
                    for _ in range(reps):
                        r = subprocess.run([str(binary), "--dataset-path", d, "--cam-calib", d + "/calib.json", *extra],
                                           capture_output=True, text=True, timeout=1500)
                        if r.returncode != 0:
                            return {"error": (r.stderr or r.stdout)[-300:]}
                        cur = json.loads(r.stdout.strip().splitlines()[-1])
                        if best is None or cur.get("frames_per_s", 0) > best.get("frames_per_s", 0):
                            best = cur
                    return best

                runs = {
                    "operator_sequence": run(exe, default_flags + ["--traj", d + "/gpu_ops.csv"], 1),
                    "device_resident": run(exe, default_flags + ["--fused", "--traj", d + "/gpu.csv"], 2),
                    "device_resident_4_streams": run(exe, default_flags + ["--fused", "--replicas", "4"], 1),
                    "device_resident_16_streams": run(exe, default_flags + ["--fused", "--replicas", "16"], 1),
                    "cpu_oracle": run(cpu_exe, default_flags + ["--traj", d + "/cpu.csv"], 1),
                    "stages_open_loop": run(exe, ["--voc-path", voc_path, "--inject-drift", "300:0.5,0,0.3", "--fused"], 1),  # loop closure off
                    "stages_device_resident": run(exe, stage_flags + ["--fused"], 1),
                    "stages_cpu_oracle": run(cpu_exe, stage_flags, 1),
                    # the round-2 figure, kept as a second, labelled entry: the VO subset (all three branches OFF) on the
                    # first 90 frames
                    "vo_subset_device_resident": run(exe, ["--fused", "--frames", "90"], 3),
                    "vo_subset_cpu_oracle": run(cpu_exe, ["--frames", "90"], 1),
                }
                same_traj = None
                try:
                    same_traj = (Path(d) / "gpu.csv").read_bytes() == (Path(d) / "gpu_ops.csv").read_bytes()
                except OSError:
                    pass
            # NATURAL LOOP LEG: a lap with real accumulated drift that closes its loop under the
            # reference's defaults and NOTHING else -- a larger room (half extents 8 x 3 x 8 m, radius 6 m, 6 cm per frame:
            # a 628-frame lap, ~8 cm of drift), 720 frames so that the revisit yields the three consecutive consistent
            # detections num_consistency asks for.  The CPU build runs beside it, whatever it does.
            natural = None
            if args.e2e_natural:
                with tempfile.TemporaryDirectory(prefix="vsl_seq_nat_") as d2:
                    t_render2 = time.perf_counter()
                    code = ("import sys, importlib; sys.path.insert(0, %r); import __graft_entry__ as e; e.load_package(); "
                            "sq = importlib.import_module('visual_slam_amd.synth_sequence'); "
                            "sq.render_sequence(%r, n_frames=720, seed=1, step_m=0.06, radius=6.0, workers=%d, look_deg=90.0, "
                            "room_half=(8.0, 3.0, 8.0), px_per_m=60.0)" % (str(ROOT), d2, max(1, min(16, os.cpu_count() or 1))))
                    subprocess.run([sys.executable, "-c", code], check=True, timeout=1500)
                    t_render2 = time.perf_counter() - t_render2

                    def run2(binary, extra):
                        if not binary.exists():
                            return {"error": "%s not built" % binary.name}
                        r = subprocess.run([str(binary), "--dataset-path", d2, "--cam-calib", d2 + "/calib.json", *extra],
                                           capture_output=True, text=True, timeout=1500)
                        if r.returncode != 0:
                            return {"error": (r.stderr or r.stdout)[-300:]}
                        return json.loads(r.stdout.strip().splitlines()[-1])

                    natural = {"gpu": run2(exe, default_flags + ["--fused"]), "cpu": run2(cpu_exe, default_flags),
                               "gpu_loop_closure_off": run2(exe, ["--relocalization", "--voc-path", voc_path, "--fused"]),
                               "render_s": round(t_render2, 1)}
            flags_txt = " ".join(f if f != voc_path else "<k=10 L=6 vocabulary, 1,111,111 nodes>" for f in default_flags)
            e = runs["device_resident"]
            if "error" not in e:
                out["end_to_end_single_stream"] = {
                    "flags": flags_txt + " --fused",
                    "workload": "rendered EuRoC-layout stereo lap (textured room, double-sphere cameras looking at the nearest "
                                "wall): %d frames on a circle of %d frames (the last %d revisit the start), reference defaults (1500 "
                                "features, new_kf_min_inliers 80, 10-keyframe window, loop_closing_time 500, num_consistency 3), "
                                "relocalisation + loop closure + global BA after a loop + per-keyframe compute_bow_vector ON, no "
                                "test hooks; synchronous local BA, images decoded up front; device-resident frame store + map"
                                % (n_frames, lap_frames, n_frames - lap_frames),
                    "loops_note": "no loop closes in this leg (the map is consistent at the revisit and no keyframe is taken "
                                  "there): loop detection runs on every keyframe (stage_ms_total.loop); the stages behind a "
                                  "detection are timed in end_to_end_loop_closing_stages",
                    "frames": e["frames"], "keyframes": e["keyframes"], "frames_per_s": e["frames_per_s"], "best_of_runs": 2,
                    "ms_per_frame": e["ms_per_frame"], "ate_rmse_m": e["ate_rmse_m"],
                    "loops_closed": e["loops_closed"], "global_ba_runs": e["global_ba_runs"], "bow_vectors": e["bow_vectors"],
                    "tracking_lost": e["tracking_lost"], "relocalized": e["relocalized"],
                    "stage_ms_total": e["stage_ms_total"],
                    "frames_per_s_operator_by_operator": runs["operator_sequence"].get("frames_per_s"),
                    "frames_per_s_4_independent_streams_one_gpu": runs["device_resident_4_streams"].get("frames_per_s"),
                    # BASELINE configs[3] in miniature: independent streams (one host thread, context, frame store and map
                    # each) sharing ONE GPU; every stream reproduces the same trajectory bit for bit (streams_agree)
                    "frames_per_s_16_independent_streams_one_gpu": runs["device_resident_16_streams"].get("frames_per_s"),
                    "independent_streams_agree": bool(runs["device_resident_4_streams"].get("streams_agree")) and
                                                 bool(runs["device_resident_16_streams"].get("streams_agree")),
                    "operator_path_and_device_resident_path_same_trajectory_file": same_traj,
                    "sequence_render_s": round(t_render, 1)}
                out["end_to_end_single_stream"]["device_accounting"] = device_accounting(e)
                c = runs["cpu_oracle"]
                if "error" not in c:
                    # the north star's comparison: frames/s end to end, GPU next to the CPU path on the same sequence
                    out["cpu_baseline_end_to_end"] = {
                        "flags": flags_txt,
                        "value": c["frames_per_s"], "unit": "frames/s", "kind": "port", "cpu_model": cpu_model(),
                        "cores": "1 for detect / describe / match / tracking / BoW (the reference's per-frame path is single-threaded), "
                                 "%d for the bundle-adjustment Jacobians (ceres num_threads = hardware_concurrency)" % (os.cpu_count() or 1),
                        "what": "the same application source (slam_headless.cpp + drop-in headers) linked against the C ABI "
                                "implemented on the CPU oracle (oracle/abi_on_oracle.cpp), same rendered sequence, same flags",
                        "frames": c["frames"], "keyframes": c["keyframes"], "ate_rmse_m": c["ate_rmse_m"],
                        "loops_closed": c["loops_closed"], "global_ba_runs": c["global_ba_runs"], "bow_vectors": c["bow_vectors"],
                        "tracking_lost": c["tracking_lost"], "relocalized": c["relocalized"],
                        "stage_ms_total": c["stage_ms_total"],
                        "trajectory_note": "operators are bit-exact and the host code is the same source: with bundle adjustment off "
                                           "the two trajectory files are identical (tests/test_headless_gpu.py); with it on, ~1e-7 "
                                           "differences after the first optimisation flip borderline RANSAC inliers and the runs "
                                           "diverge like two runs of the reference would -- compare the two ATE values",
                        "gpu_over_cpu_end_to_end": round(e["frames_per_s"] / c["frames_per_s"], 1),
                        "gpu_4_streams_over_cpu_end_to_end": (round(runs["device_resident_4_streams"]["frames_per_s"] / c["frames_per_s"], 1)
                                                              if "frames_per_s" in runs["device_resident_4_streams"] else None)}
                else:
                    out["cpu_baseline_end_to_end"] = c
            else:
                out["end_to_end_single_stream"] = e
            so, sg, sc = runs["stages_open_loop"], runs["stages_device_resident"], runs["stages_cpu_oracle"]
            if "error" not in sg:
                keys = ("frames_per_s", "keyframes", "ate_rmse_m", "loops_closed", "global_ba_runs", "tracking_lost", "stage_ms_total")
                out["end_to_end_loop_closing_stages"] = {
                    "flags": " ".join(f if f != voc_path else "<k=10 L=6 vocabulary>" for f in stage_flags),
                    "test_hooks": "--inject-drift (a displaced pose estimate stands in for accumulated drift) and --force-loop "
                                  "(keyframe 0 handed to the loop-closing stage once the lap is complete); everything behind "
                                  "them -- compute_sim3, loop_align, pose_graph_optimization, global_bundle_adjustment, merge-back "
                                  "-- is the product path",
                    "gpu_device_resident": {k: sg.get(k) for k in keys},
                    "cpu_oracle": ({k: sc.get(k) for k in keys} if "error" not in sc else sc),
                    "gpu_ate_rmse_m_with_loop_closure_off": so.get("ate_rmse_m"),
                    "gpu_over_cpu": (round(sg["frames_per_s"] / sc["frames_per_s"], 1) if "error" not in sc else None)}
            if natural is not None and "error" not in natural["gpu"]:
                keys = ("frames", "frames_per_s", "ms_per_frame", "keyframes", "ate_rmse_m", "loops_closed", "global_ba_runs",
                        "tracking_lost", "relocalized", "stage_ms_total")
                ng, nc, no = natural["gpu"], natural["cpu"], natural["gpu_loop_closure_off"]
                out["end_to_end_natural_loop"] = {
                    "flags": flags_txt + " --fused   (the reference's defaults, NO test hook)",
                    "workload": "rendered EuRoC-layout stereo lap in a larger room (half extents 8 x 3 x 8 m, radius 6 m, 6 cm per "
                                "frame, cameras looking at the nearest wall): 720 frames on a circle of 628 -- the drift of one lap "
                                "is real (no --inject-drift), the candidate comes from the BoW database and three consecutive "
                                "consistent detections (no --force-loop)",
                    "gpu_device_resident": {k: ng.get(k) for k in keys},
                    "cpu_oracle": ({k: nc.get(k) for k in keys} if "error" not in nc else nc),
                    "gpu_ate_rmse_m_with_loop_closure_off": no.get("ate_rmse_m"),
                    "gpu_over_cpu": (round(ng["frames_per_s"] / nc["frames_per_s"], 1) if "error" not in nc and nc.get("frames_per_s") else None),
                    "note": "whether a rendered lap closes is sensitive to which keyframes are taken: the CPU build follows its own "
                            "trajectory after the first bundle adjustment (~1e-7 differences flip borderline RANSAC inliers) and is "
                            "reported as it ran, closed loop or not",
                    "sequence_render_s": natural["render_s"]}
            v, vc = runs["vo_subset_device_resident"], runs["vo_subset_cpu_oracle"]
            if "error" not in v:
                out["end_to_end_vo_subset"] = {
                    "flags": "--fused --frames 90 (relocalisation, loop closure, BoW all OFF: NOT the reference's defaults; the "
                             "round-2 figure, kept for continuity)",
                    "frames": v["frames"], "keyframes": v["keyframes"], "frames_per_s": v["frames_per_s"], "best_of_runs": 3,
                    "ms_per_frame": v["ms_per_frame"], "ate_rmse_m": v["ate_rmse_m"], "stage_ms_total": v["stage_ms_total"],
                    "cpu_oracle_frames_per_s": vc.get("frames_per_s"), "cpu_oracle_ate_rmse_m": vc.get("ate_rmse_m")}
    # ---- N > 1: the global-BA leg over ALL ranks (the J^T J all-reduce of BASELINE configs[4]; N = 1 ran it above).  It
    # is the last thing before the line is printed, under a watchdog: if a collective does not come back (a rank lost, a
    # communicator that never forms) rank 0 still prints the frame-pipeline line -- with the failure named -- and every
    # rank leaves.
    if args.full and args.gba and world > 1:
        import threading

        def give_up():
            if rank == 0:
                out["global_ba"] = {"error": "the multi-rank global-BA leg did not finish within %d s; the line carries the "
                                             "replicated frame pipeline only" % args.gba_timeout, "world": world}
                print(json.dumps(out), flush=True)
            os._exit(0)

        dog = threading.Timer(args.gba_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            gba_multi = global_ba_multi_rank(args, vsl, ctx, synth, vdist, rank, world, backend)
        except Exception as e:  # a rank-local failure: say so in the line, do not lose the frame-pipeline figure
            gba_multi = {"error": "%s: %s" % (type(e).__name__, e), "world": world}
        dog.cancel()
        if rank == 0:
            out["global_ba"] = gba_multi
    if rank == 0:
        print(json.dumps(out), flush=True)

    for _, c, f in units:
        f.close()
        c.close()
    vdist.barrier()
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
