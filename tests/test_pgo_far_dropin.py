"""visnav::pose_graph_optimization_far_edges (include/visnav_amd/loop_closure.h) on the small closed loop of
tests/test_pgo_joint_covariance_dropin.py: it compiles against the header and flattens on the host (CPU test), and -- on
the GPU box -- returns the bytes of vsl_pose_graph_optimize on the flattened graph with the "pgo_far_edges" diagnostic
set, reports what vsl_ctx_last_pgo_far reports, and leaves the diagnostic as it found it."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_pgo_joint_covariance_dropin as base

ROOT = Path(__file__).resolve().parents[1]
K, PAIRS = base.K, base.PAIRS


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/pgo_far_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrapper_compiles_and_flattens_on_the_host(tmp_path, vsl, synth):
    assert vsl.library_path().exists()
    exe = _compile(tmp_path / "pgo_far_dropin_test")
    d, cov, sim3, rel = base._map(synth)
    base._write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = base._expected_graph(d, cov, sim3, rel)
    assert r.stdout.strip() == "flatten ok: %d nodes, %d edges" % (K, len(g.edge_a))


@pytest.mark.gpu
def test_wrapper_matches_the_c_abi(tmp_path, synth):
    exe = _compile(tmp_path / "pgo_far_dropin_test")
    d, cov, sim3, rel = base._map(synth)
    base._write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    assert len(buf) == 2 * 7 * K + 10 + 4
    wrap, direct = buf[:7 * K], buf[7 * K:14 * K]
    rep, drep, diag = buf[14 * K:14 * K + 5], buf[14 * K + 5:14 * K + 10], buf[14 * K + 10:]
    print("report (taken, far edges, half bandwidth, columns, solves):", rep)
    assert wrap.tobytes() == direct.tobytes()
    assert np.array_equal(rep, drep) and (rep[0] == 1.0) == (rep[1] > 0)
    assert list(diag) == [0.0, 0.0, 1.0, 1.0]                # left as found, off or on
    assert np.abs(wrap - d["poses"].reshape(-1)).max() > 1e-6  # something was optimised
