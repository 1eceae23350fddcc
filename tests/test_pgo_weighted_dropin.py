"""The EdgeInformation overloads of include/visnav_amd/loop_closure.h (flatten_pose_graph, pose_graph_optimization,
pose_graph_covariance, pose_graph_joint_covariance, loop_candidate_consistency) on the small closed loop of
tests/test_pgo_joint_covariance_dropin.py: the flattening on the host (CPU test), and -- on the GPU box -- the overloads
with a callback beside the _w entry points of the C ABI on the flattened problem, the existing signatures beside the
unweighted C ABI (bit for bit both times: the same calls), and the weights showing in the result."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_pgo_joint_covariance_dropin as base

ROOT = Path(__file__).resolve().parents[1]
K, PAIRS = base.K, base.PAIRS


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/pgo_weighted_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_flattening_with_a_callback_on_the_host(tmp_path, vsl, synth):
    assert vsl.library_path().exists()
    exe = _compile(tmp_path / "pgo_weighted_test")
    d, cov, sim3, rel = base._map(synth)
    base._write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = base._expected_graph(d, cov, sim3, rel)
    assert r.stdout.strip() == "flatten ok: %d nodes, %d edges, 1 weighted as the loop constraint" % (K, len(g.edge_a))


@pytest.mark.gpu
def test_overloads_match_the_c_abi(tmp_path, synth):
    exe = _compile(tmp_path / "pgo_weighted_test")
    d, cov, sim3, rel = base._map(synth)
    base._write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr          # (also: a zero information matrix threw and wrote no pose)
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    nq = len(PAIRS)
    sizes = [7 * K, 36 * nq, 144 * nq, 43]
    assert len(buf) == 2 * 2 * sum(sizes)
    records = []
    for rec in buf.reshape(2, -1):
        parts, at = [], 0
        for n in sizes:
            parts.append((rec[at:at + n], rec[at + n:at + 2 * n]))
            at += 2 * n
        records.append(parts)
    for which, parts in zip(("with a callback", "without"), records):
        for what, (wrap, direct) in zip(("poses", "covariance", "joint covariance", "consistency"), parts):
            assert np.array_equal(wrap, direct), (which, what)          # the same call on the same problem
            assert wrap.any(), (which, what)
    weighted, plain = records
    assert np.abs(weighted[0][0] - d["poses"].reshape(-1)).max() > 1e-6                 # the solve moved the keyframes
    assert np.array_equal(plain[0][0].reshape(K, 7)[K - 1], d["poses"][K - 1])           # the fixed current keyframe
    assert not np.array_equal(weighted[0][0], plain[0][0])                               # the weights show in the solution
    # every information matrix is >= 50 I: the marginal covariances shrink
    wc, pc = weighted[1][0].reshape(nq, 6, 6), plain[1][0].reshape(nq, 6, 6)
    assert np.all(np.trace(wc, axis1=1, axis2=2) < np.trace(pc, axis1=1, axis2=2))
    assert np.array_equal(weighted[3][0][:6], plain[3][0][:6])                           # the candidate's residual is not whitened
