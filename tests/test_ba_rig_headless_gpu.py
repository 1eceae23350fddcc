"""GPU: `slam_headless --fused --rig-ba` on the 90-frame rendered sequence of tests/test_headless_gpu.py: the local bundle
adjustment of include/visnav_amd/harness/odometry.h goes through visnav::bundle_adjustment_rig (one pose per stereo
keyframe).  The run exits with status 0, its ATE is finite, and two runs write byte-identical trajectory files."""
import importlib
import json
import math
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "visual-slam_amd" / "slam_headless"


def test_rig_local_ba_in_the_headless_pipeline(tmp_path, vsl):
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    seq = tmp_path / "seq"
    seq.mkdir()
    sq.render_sequence(str(seq), n_frames=90, seed=1, step_m=0.04, radius=1.6)
    assert EXE.exists(), "build() did not produce visual-slam_amd/slam_headless"
    out = []
    for k in range(2):
        traj = tmp_path / ("traj%d.csv" % k)
        r = subprocess.run([str(EXE), "--dataset-path", str(seq), "--cam-calib", str(seq / "calib.json"), "--traj", str(traj),
                            "--kf-min-inliers", "500", "--fused", "--rig-ba"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append((json.loads(r.stdout.strip().splitlines()[-1]), traj.read_bytes()))
    res = out[0][0]
    print("rig local BA: %d keyframes, ATE %.4f m over %d associations" % (res["keyframes"], res["ate_rmse_m"], res["ate_associations"]))
    assert res["frames"] == 90 and res["keyframes"] >= 2 and res["fused_tracking"] is True
    assert math.isfinite(res["ate_rmse_m"])
    assert len(out[0][1]) > 0 and out[0][1] == out[1][1]
