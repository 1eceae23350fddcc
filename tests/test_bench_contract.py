"""The committed bench line of the newest round (profiles/rNN_bench_line.json = the stdout of `python bench.py` on an
MI355X) carries every key the benchmark contract names, with consistent values; and bench.py's command line still
parses the driver's flags."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
ROUND = sorted(p.name.split("_")[0] for p in (ROOT / "profiles").glob("r[0-9][0-9]_bench_line.json"))[-1]


def test_committed_bench_line_has_the_contract_keys():
    d = json.loads((ROOT / "profiles" / (ROUND + "_bench_line.json")).read_text())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None  # BASELINE.md holds no published number for this metric
    assert "workload" in d["config"] and "model" not in d["config"]
    # value = frames of all ranks / time of the K timed steps
    frames = d["n_gpus"] * d["config"]["stereo_frames_per_step_per_gpu"] * d["steps"]
    assert abs(frames / (d["ms_per_step"] * 1e-3 * d["steps"]) - d["value"]) < 1e-3 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-4
    # achieved = algorithmic bytes per launch / average launch duration
    assert abs(r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9 - r["achieved"]) < 1e-2 * r["achieved"]
    # K1 must at least read every image byte of the launch (its own outputs are a few MB; the 56 B per keypoint of the
    # stage's algorithmic figure are written by the kernels behind it)
    images = 2 * d["config"]["stereo_frames_per_launch"]
    assert r["traffic"] is None or 0.95 * images * 752 * 480 <= r["traffic"] <= 3 * r["algorithmic_bytes_per_launch"]
    # the sustained-rate and upload-inclusive figures of round 2
    assert d["config"]["inputs_resident_in_hbm"] is True and d["config"]["h2d_in_timed_region"] is False
    assert d["config"]["timed_region_s"] >= 1.0
    assert 0 < d["value_incl_upload"] < d["value"] and d["streaming"]["outputs_equal_resident_run"] is True
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["unit"] == d["unit"]


def test_pmc_traffic_profile_matches_the_bench_launch_size():
    # bench.py fills roofline.traffic from this file only when it was collected at the launch size it runs at
    d = json.loads((ROOT / "profiles" / (ROUND + "_bench_line.json")).read_text())
    pm = json.loads((ROOT / "profiles" / (ROUND + "_pmc_traffic.json")).read_text())
    assert pm["batch_stereo_frames"] == d["config"]["stereo_frames_per_launch"]
    k = pm["kernels"][d["roofline"]["kernel"]]
    assert abs(k["bytes_per_launch_uncorrected"] - (k["FETCH_SIZE_KiB"] + k["WRITE_SIZE_KiB"]) * 1024) < 2048
    # the calibrated figure (FETCH_SIZE x its measured factor + WRITE_SIZE x its factor) is what the bench line carries
    want = (k["FETCH_SIZE_KiB"] * k["FETCH_SIZE_factor"] + k["WRITE_SIZE_KiB"] * k["WRITE_SIZE_factor"]) * 1024
    assert abs(k["bytes_per_launch"] - want) < 1e-3 * want


def test_sq_counter_summaries_hold_physically_possible_values():
    # a summary that folded two kernels into one row carried 53.6 resident waves per SIMD (the
    # hardware holds 8) and 0.55 SIMD-cycles per vector instruction (a SIMD issues at most one per cycle).  Every
    # committed summary from round 4 on is checked; the tool asserts the same when it writes one.
    for p in sorted((ROOT / "profiles").glob("r*_sq_counters.json")):
        if int(p.name[1:3]) < 4:
            continue
        doc = json.loads(p.read_text())
        for name, k in doc["kernels"].items():
            assert k.get("mean_resident_waves_per_simd", 0) <= 8.4, (p.name, name, k)
            assert k.get("simd_cycles_per_valu_instruction", 9) >= 1.0, (p.name, name, k)
    sys.path.insert(0, str(ROOT / "tools"))
    import frame_sq_summary as fs
    # whole kernel names: no substring hits across kernels, the two matcher instances apart
    assert fs.row_name("(anonymous namespace)::match_select_kernel(int const*, int const*)") == "match_select"
    assert fs.row_name("void select_kernel<false>(unsigned long const*, int*)") == "select"
    assert fs.row_name("void hamming_mx_kernel<true>(unsigned long const*)") == "match_reverse"
    assert fs.row_name("void hamming_mx_kernel<false>(unsigned long const*)") == "match_forward"
    assert fs.row_name("exact_bits_kernel(unsigned char const*)") is None


def test_bench_command_line_accepts_the_driver_flags():
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in out.stdout


def _run_bench(args, env_extra, timeout=300):
    import os
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(env_extra)
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)


def test_gpus_n_without_a_launcher_starts_n_ranks():
    # `python bench.py --gpus 2` (no torchrun around it) must produce 2 ranks -- it used to run one
    # rank and print "n_gpus": 1.  Rehearsed on the CPU: gloo, a sleeping step (--rehearse-plumbing), the real launcher path.
    r = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--rehearse-plumbing"], {"VSL_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # ONE line, rank 0's
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["rehearsal"] is True and d["value"] is None
    assert len(d["per_rank_ms_per_step"]) == 2
    assert d["per_rank_ms_per_step"][1] > d["per_rank_ms_per_step"][0]          # the planted straggler shows
    assert d["ms_per_step"] >= max(d["per_rank_ms_per_step"]) - 1e-3            # MAX over ranks


def test_gpus_n_that_disagrees_with_the_launcher_fails():
    r = _run_bench(["--gpus", "8", "--rehearse-plumbing"], {"WORLD_SIZE": "1", "RANK": "0", "VSL_BENCH_BACKEND": "gloo"}, timeout=120)
    assert r.returncode != 0 and "does not match WORLD_SIZE" in (r.stdout + r.stderr)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _FakeFrames:
    """Stands in for visual_slam_amd.Frames: image slot s of unit u carries 3 + (u * 7 + s) % 5 keypoints whose
    values encode (u, s, i); pair k carries k % 4 matches."""

    def __init__(self, u):
        self.u = u

    def keypoints(self, slot):
        n = 3 + (self.u * 7 + slot) % 5
        i = np.arange(n, dtype=np.float64)
        xy = np.stack([1000.0 * self.u + slot + 0.5 + 0 * i, i], 1)
        desc = (np.arange(4 * n, dtype=np.uint64).reshape(n, 4) + np.uint64(1 << 40) * np.uint64(slot + 1))
        return xy, 0.25 * i, desc

    def matches(self, pair):
        m = pair % 4
        return np.stack([np.arange(m), np.arange(m)[::-1]], 1).astype(np.int32)


def test_dump_outputs_writes_float_arrays_of_the_last_step(tmp_path):
    # --dump-outputs on fake frame stores (the real ones need a GPU): every file float32 / float64, the counts of all
    # frames, a fixed sample whose keypoints and matches are the stores' own, the same files on a second call
    bench = _bench_module()
    B, Bu = 64, 32
    units = [(None, None, _FakeFrames(u)) for u in range(2)]
    counts = [(np.array([len(units[u][2].keypoints(s)[0]) for s in range(2 * Bu)], np.int32),
               np.array([len(units[u][2].matches(k)) for k in range(Bu)], np.int32)) for u in range(2)]
    bench.dump_outputs(str(tmp_path / "a"), units, counts, B, Bu)
    bench.dump_outputs(str(tmp_path / "b"), units, counts, B, Bu)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir()) and len(files) >= 5
    d = {}
    for name in files:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, b), name
        d[name[:-4]] = a
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert np.array_equal(d["keypoints_per_image"], np.concatenate([c[0] for c in counts]))
    assert np.array_equal(d["matches_per_pair"], np.concatenate([c[1] for c in counts]))
    sample = d["sample_stereo_frames"].astype(np.int64)
    assert len(sample) == min(bench.DUMP_SAMPLE_FRAMES, B) and len(set(sample.tolist())) == len(sample)
    assert np.array_equal(d["sample_keypoints_per_image"], d["keypoints_per_image"].reshape(-1, 2)[sample].ravel())
    assert np.array_equal(d["sample_matches_per_pair"], d["matches_per_pair"][sample])
    n_kp = int(d["sample_keypoints_per_image"].sum())
    assert d["sample_keypoints_xy"].shape == (n_kp, 2) and d["sample_keypoints_angle"].shape == (n_kp,)
    assert d["sample_descriptor_bytes"].shape == (n_kp, 32)
    assert d["sample_matches"].shape == (int(d["sample_matches_per_pair"].sum()), 2)
    # the first sampled frame, left image: the store's own keypoints and descriptor bytes
    f = int(sample[0])
    xy, ang, desc = units[f // Bu][2].keypoints(2 * (f % Bu))
    n = len(xy)
    assert np.array_equal(d["sample_keypoints_xy"][:n], xy) and np.array_equal(d["sample_keypoints_angle"][:n], ang)
    assert np.array_equal(d["sample_descriptor_bytes"][:n], desc.view(np.uint8).reshape(n, 32))


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_only_and_dumps_its_outputs(tmp_path):
    # a plain run times K steps and prints the headline line, nothing of --full; --dump-outputs writes the last step's
    # outputs, and they are the same on a second run with the same arguments
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "64", "--scenes", "8", "--passes", "2",
            "--gen-workers", "2"]
    lines = []
    for tag in ("a", "b"):
        r = _run_bench(args + ["--dump-outputs", str(tmp_path / tag)], {}, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines += [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    frames = d["config"]["stereo_frames_per_step_per_gpu"] * d["steps"]
    assert abs(frames / (d["ms_per_step"] * 1e-3 * d["steps"]) - d["value"]) < 1e-3 * d["value"]
    for k in ("roofline", "cpu_baseline", "value_incl_upload", "stage_ms_per_launch", "local_ba", "global_ba",
              "pose_graph", "bow", "end_to_end_single_stream"):
        assert k not in d, k
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir()) and "sample_descriptor_bytes.npy" in names
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    nk = np.load(tmp_path / "a" / "keypoints_per_image.npy")
    assert nk.shape == (128,) and nk.min() > 0
    assert abs(nk.mean() - d["config"]["mean_keypoints_per_image"]) < 0.1
