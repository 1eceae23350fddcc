"""GPU: the headless application with the keyframe BoW on the frame store (slam_headless --device-bow,
OdometryOptions::device_bow): the keyframe's vector is computed by vsl_frames_bow_vectors (n = 1) on the slot that
already holds the left image and appended to the device keyframe database there.  On the rendered lap of
tests/test_headless_gpu.py (same recipe, its loop-closing run with relocalisation as in
tests/test_place_db_headless_gpu.py) the trajectory BYTES and the loop / relocalisation candidates of every keyframe
must be those of the same command without the flag."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "visual-slam_amd" / "slam_headless"


@pytest.fixture(scope="module")
def loop_sequence(tmp_path_factory, vsl, synth):
    # a full lap and a bit: 230 frames on a circle of 168 frames
    d = tmp_path_factory.mktemp("loopseq")
    code = ("import sys, importlib; sys.path.insert(0, %r); import __graft_entry__ as e; e.load_package(); "
            "sq = importlib.import_module('visual_slam_amd.synth_sequence'); "
            "sq.render_sequence(%r, n_frames=230, seed=1, step_m=0.045, radius=1.2, workers=12)" % (str(ROOT), str(d)))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=600)   # a fresh process: forked render workers, no GPU
    (d / "voc.txt").write_text(synth.vocabulary_text(3, 10, 4))
    return d


def _run(seq_dir, *extra, expect=0):
    assert EXE.exists(), "build() did not produce visual-slam_amd/slam_headless"
    env = dict(os.environ, VISNAV_AMD_TRACE="1")   # one stderr line per loop detection / relocalisation with its candidates
    r = subprocess.run([str(EXE), "--dataset-path", str(seq_dir), "--cam-calib", str(seq_dir / "calib.json"), *extra],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == expect, r.stdout + r.stderr
    if expect:
        return None, r.stderr
    cands = [ln for ln in r.stderr.splitlines() if ln.startswith(("loop detection keyframe", "relocalize", "relocalization"))]
    return json.loads(r.stdout.strip().splitlines()[-1]), cands


def test_device_bow_writes_the_same_trajectory_and_candidates(loop_sequence):
    d = loop_sequence
    common = ["--kf-min-inliers", "400", "--voc-path", str(d / "voc.txt"), "--loop-closure", "--relocalization", "--loop-time", "30",
              "--inject-drift", "100:1.0,0,0.5", "--force-loop", "170:0", "--fused", "--device-place-db", "--reloc-check", "70"]
    ta, tb = d / "bow_host.csv", d / "bow_device.csv"
    a, ca = _run(d, *common, "--traj", str(ta))
    b, cb = _run(d, *common, "--traj", str(tb), "--device-bow")
    assert "device_bow" not in a and b["device_bow"] is True
    assert a["keyframes"] == b["keyframes"] > 10 and b["bow_vectors"] == b["keyframes"]
    assert a["loops_closed"] == b["loops_closed"] == 1 and a["global_ba_runs"] == b["global_ba_runs"]
    assert (a["tracking_lost"], a["relocalized"]) == (b["tracking_lost"], b["relocalized"])
    assert (a["reloc_check_ok"], a["reloc_check_err_m"]) == (b["reloc_check_ok"], b["reloc_check_err_m"])
    # the candidates of every keyframe: one line per loop detection (and per relocalisation), with the candidate list
    loops = [ln for ln in ca if ln.startswith("loop detection keyframe")]
    assert len(loops) >= a["keyframes"]          # every keyframe taken went through the loop detection (old ones are removed later)
    assert any(ln.startswith("relocalize frame") for ln in ca)   # ... and the relocalisation check queried the database
    assert ca == cb
    assert ta.read_bytes() == tb.read_bytes()


def test_device_bow_needs_the_fused_path_and_the_device_database(loop_sequence):
    d = loop_sequence
    base = ["--voc-path", str(d / "voc.txt"), "--loop-closure", "--device-bow"]
    for extra in ([], ["--fused"], ["--device-place-db"]):
        _, err = _run(d, *base, *extra, expect=2)
        assert "--device-bow needs --fused and --device-place-db" in err
