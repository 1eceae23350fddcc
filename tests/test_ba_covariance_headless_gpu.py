"""GPU: slam_headless --ba-covariance FILE (visual-slam_amd/apps/slam_headless.cpp, harness/odometry.h
write_window_covariance) on the 90-frame rendered sequence of tests/test_headless_gpu.py: after every local bundle
adjustment one line per keyframe of the window whose pose was optimised (the oldest keyframe is fixed: it is the gauge
and has no covariance) -- frame id, sqrt trace of the translational block, sqrt trace of the rotational block of the
left camera's pose covariance -- and a trajectory file that is byte for byte the one of a run without the flag."""
import importlib
import json
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = ROOT / "visual-slam_amd" / "slam_headless"


def _run(seq_dir, *extra, expect=0):
    assert EXE.exists(), "build() did not produce visual-slam_amd/slam_headless"
    r = subprocess.run([str(EXE), "--dataset-path", str(seq_dir), "--cam-calib", str(seq_dir / "calib.json"), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == expect, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]) if expect == 0 else r.stderr


def test_window_covariance_file_and_unchanged_trajectory(tmp_path, vsl):
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    seq = tmp_path / "seq"
    seq.mkdir()
    sq.render_sequence(str(seq), n_frames=90, seed=1, step_m=0.04, radius=1.6)
    t0, t1, cov = tmp_path / "t0.csv", tmp_path / "t1.csv", tmp_path / "cov.txt"
    a = _run(seq, "--traj", str(t0), "--kf-min-inliers", "500")
    b = _run(seq, "--traj", str(t1), "--kf-min-inliers", "500", "--ba-covariance", str(cov))
    assert t0.read_bytes() == t1.read_bytes()
    assert a["keyframes"] == b["keyframes"] >= 5
    rows = np.loadtxt(cov, ndmin=2)
    assert rows.shape[1] == 3 and np.isfinite(rows).all() and (rows[:, 1:] > 0).all()
    # one block of lines per keyframe solve, frame ids ascending inside it (std::map order); the window holds at most
    # 10 keyframes of which the oldest is fixed; the first keyframe's window has no free camera and writes nothing
    ids = rows[:, 0].astype(int)
    starts = [0] + [i for i in range(1, len(ids)) if ids[i] <= ids[i - 1]] + [len(ids)]
    sizes = np.diff(starts)
    assert len(sizes) == b["keyframes"] - 1, (sizes, b)
    assert list(sizes) == [min(k, 9) for k in range(1, len(sizes) + 1)]
    assert ids.min() > 0 and ids.max() < 90
    # uncertainty grows with the distance from the gauge inside a window
    last = rows[starts[-2]:]
    assert last[-1, 1] > last[0, 1]
    err = _run(seq, "--ba-covariance", str(cov), "--replicas", "2", expect=2)
    assert "--replicas 1" in err
