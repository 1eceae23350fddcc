"""GPU: `slam_headless --fused --rig-ba --rig-global-ba` on the forced-loop sequence of tests/test_headless_gpu.py
(`--inject-drift` stands in for drift, `--force-loop` hands keyframe 0 to the loop-closing stage): the global bundle
adjustment after the loop closure goes through visnav::global_bundle_adjustment_rig (one pose per stereo keyframe, the
reduced body system over co-visible keyframes in band storage).  The run exits with status 0, two runs write
byte-identical trajectories, and right after the global BA every right camera sits on left * T_0_1 to 4 ulp.  Without
the flag the global BA goes back to two free cameras per keyframe and pulls them apart: asserted too, so the test shows
the feature."""
import json
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "visual-slam_amd" / "slam_headless"


@pytest.fixture(scope="module")
def loop_sequence(tmp_path_factory, vsl, synth):
    # a full lap and a bit: 230 frames on a circle of 168 frames (the sequence of the other forced-loop tests)
    d = tmp_path_factory.mktemp("loopseq")
    code = ("import sys, importlib; sys.path.insert(0, %r); import __graft_entry__ as e; e.load_package(); "
            "sq = importlib.import_module('visual_slam_amd.synth_sequence'); "
            "sq.render_sequence(%r, n_frames=230, seed=1, step_m=0.045, radius=1.2, workers=12)" % (str(ROOT), str(d)))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=600)   # a fresh process: forked render workers, no GPU
    (d / "voc.txt").write_text(synth.vocabulary_text(3, 10, 4))
    return d


def _run(seq_dir, *extra):
    assert EXE.exists(), "build() did not produce visual-slam_amd/slam_headless"
    r = subprocess.run([str(EXE), "--dataset-path", str(seq_dir), "--cam-calib", str(seq_dir / "calib.json"), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_rig_global_ba_keeps_the_stereo_pairs_on_the_calibration(loop_sequence, tmp_path):
    d = loop_sequence
    common = ["--kf-min-inliers", "400", "--voc-path", str(d / "voc.txt"), "--loop-closure", "--loop-time", "30",
              "--inject-drift", "100:1.0,0,0.5", "--force-loop", "170:0", "--fused", "--rig-ba"]
    out = []
    for k in range(2):
        traj = tmp_path / ("rig_gba_%d.csv" % k)
        out.append((_run(d, *common, "--rig-global-ba", "--traj", str(traj)), traj.read_bytes()))
    res = out[0][0]
    print("rig global BA: %d keyframes, %d loops, %d global BAs, ATE %.4f m, stereo deviation after the global BA %.3f ulp" %
          (res["keyframes"], res["loops_closed"], res["global_ba_runs"], res["ate_rmse_m"], res["gba_stereo_deviation_ulp"]))
    assert res["rig_global_ba"] is True and res["loops_closed"] == 1 and res["global_ba_runs"] == 1
    assert 0.0 <= res["gba_stereo_deviation_ulp"] <= 4.0
    assert len(out[0][1]) > 0 and out[0][1] == out[1][1]
    free = _run(d, *common)
    print("free global BA under --rig-ba: stereo deviation after the global BA %.3g ulp, ATE %.4f m" %
          (free["gba_stereo_deviation_ulp"], free["ate_rmse_m"]))
    assert free["rig_global_ba"] is False and free["global_ba_runs"] == 1
    assert free["gba_stereo_deviation_ulp"] > 1e3        # the free solver moves the two cameras of a keyframe apart
