"""visnav::pose_graph_joint_covariance and visnav::loop_candidate_consistency (include/visnav_amd/loop_closure.h) on a
small closed loop of mirror-type keyframes: the flattening on the host (CPU test), and -- on the GPU box -- their results
beside vsl_pgo_joint_covariance / vsl_pgo_edge_consistency called directly on the flattened problem (bit for bit: the
same call) and beside the long-double reference of tests/pgo_joint_ref.py on an independently assembled edge list, to
the bounds of tests/test_pgo_joint_covariance_gpu.py and tests/test_pgo_edge_consistency_gpu.py."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pgo_joint_ref as jr
import pgo_ref as pg
import spd_ref as ref

ROOT = Path(__file__).resolve().parents[1]
K, ESSENTIAL, LOOP_CAND = 30, 30, 2
PAIRS = [(5, 20), (0, 28), (17, 18), (29, 9), (20, 5), (3, 29)]   # keyframe 29 is the current one, fixed


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"),
           str(ROOT / "tests/cpp/pgo_joint_covariance_test.cpp"), "-o", str(out), "-L", str(ROOT / "visual-slam_amd"),
           "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _map(synth):
    """Keyframes 0 .. K - 1 in a loop, the last one current and fixed; a few covisibility links per keyframe with weights
    around the essential threshold."""
    rng = np.random.default_rng(8)
    d = synth.pose_graph(52, K, 0, meas_noise=0.0, drift=0.02)
    gt = d["poses_gt"]
    rel = lambda a, b, P: d["mul"](d["inv"](P[a]), P[b])  # noqa: E731
    cov = []
    for i in range(K):
        c = {}
        for j in rng.choice(i, min(i, 3), replace=False) if i else []:
            r = rel(i, int(j), gt).copy()
            r[4:] += 0.002 * rng.normal(size=3)
            c[int(j)] = (int(rng.integers(10, 60)), r)
        cov.append(c)
    return d, cov, rel(LOOP_CAND, K - 1, gt), rel


def _write(path, d, cov, sim3, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", K, ESSENTIAL, 1, LOOP_CAND))
        for i in range(K):
            f.write(d["poses"][i].astype(np.float64).tobytes())
            f.write(struct.pack("ii", i - 1, len(cov[i])))
            for j, (w, r) in cov[i].items():
                f.write(struct.pack("ii", j, w))
                f.write(np.asarray(r, np.float64).tobytes())
        f.write(np.asarray(sim3, np.float64).tobytes())
        f.write(struct.pack("i", len(pairs)))
        f.write(np.asarray(pairs, np.int32).reshape(-1).tobytes())


def _expected_graph(d, cov, sim3, rel):
    """The reference's edge selection restated independently (as tests/test_loop_closure_gpu.py does), keyframe i = node i."""
    poses = d["poses"]
    ea, eb, meas = [], [], []

    def edges_of(i):
        strong = (i - 1) in cov[i] and cov[i][i - 1][0] > ESSENTIAL
        if not strong and i - 1 >= 0:
            ea.append(i), eb.append(i - 1), meas.append(d["log"](rel(i, i - 1, poses)))
        for j, (w, rr) in sorted(cov[i].items()):
            if w > ESSENTIAL:
                ea.append(i), eb.append(j), meas.append(d["log"](rr))

    edges_of(K - 1)
    ea.append(K - 1), eb.append(LOOP_CAND), meas.append(d["log"](d["inv"](sim3)))
    for i in range(K - 2, -1, -1):
        edges_of(i)
    fixed = np.zeros(K, np.uint8)
    fixed[K - 1] = 1
    return pg.Graph(poses, fixed, ea, eb, np.array(meas))


def test_flattening_on_the_host(tmp_path, vsl, synth):
    assert vsl.library_path().exists()
    exe = _compile(tmp_path / "pgo_joint_covariance_test")
    d, cov, sim3, rel = _map(synth)
    _write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    g = _expected_graph(d, cov, sim3, rel)
    assert r.stdout.strip() == "flatten ok: %d nodes, %d edges" % (K, len(g.edge_a))


@pytest.mark.gpu
@pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)
def test_wrappers_match_the_c_abi_and_the_reference(tmp_path, synth):
    exe = _compile(tmp_path / "pgo_joint_covariance_test")
    d, cov, sim3, rel = _map(synth)
    _write(tmp_path / "in.bin", d, cov, sim3, PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    nq = len(PAIRS)
    assert len(buf) == 288 * nq + 2 * 43 + 4
    wrap, direct = buf[:144 * nq].reshape(nq, 12, 12), buf[144 * nq:288 * nq].reshape(nq, 12, 12)
    cw, cd = buf[288 * nq:288 * nq + 43], buf[288 * nq + 43:288 * nq + 86]
    routes = buf[-4:]
    assert len(set(routes)) == 1 and routes[0] in (0.0, 1.0, 2.0)
    assert np.array_equal(wrap, direct) and np.array_equal(cw, cd)          # the same call on the same problem
    c = jr.make_case(_expected_graph(d, cov, sim3, rel), True, 1.0)
    want = jr.joint_blocks(c, PAIRS)
    err = float(np.abs(wrap - want).max())
    print("joint wrapper vs reference: %.3e, bound %.3e (route %d)" % (err, c.tol, routes[0]))
    assert err <= c.tol
    assert np.array_equal(wrap, wrap.transpose(0, 2, 1))
    perm = np.r_[6:12, 0:6]
    assert np.array_equal(wrap[4], wrap[0][perm][:, perm])                  # (20, 5) against (5, 20)
    assert not wrap[3, :6].any() and not wrap[3, :, :6].any()               # the fixed current keyframe
    # the candidate: the first pair with the measurement sim3
    a, b = PAIRS[0]
    meas = np.asarray(d["log"](sim3), np.float64)
    rr, Sr, Ja, Jb, S = jr.resid_cov(c, a, b, meas)
    nj = float(np.abs(Ja).sum(axis=1).max() + np.abs(Jb).sum(axis=1).max())
    b_cov = c.tol * nj * nj + pg.GPU_TOL * float(max(np.abs(Ja).max(), np.abs(Jb).max())) * 2 * float(np.abs(S).max()) * nj
    b_r = pg.GPU_TOL * float(np.abs(pg.residual(pg._ld(c.g.poses)[a], pg._ld(c.g.poses)[b], np.zeros(6))).max())
    e_r, e_c = float(np.abs(cw[:6] - rr).max()), float(np.abs(cw[6:42].reshape(6, 6) - Sr).max())
    x2 = jr.chi2_ld(rr, Sr)
    b_x = 64 * float(np.linalg.cond(np.asarray(Sr, np.float64))) * b_cov / float(np.abs(Sr).max())
    print("consistency wrapper: resid %.3e (bound %.3e), resid_cov %.3e (bound %.3e), chi2 %.6g rel %.3e (bound %.3e)"
          % (e_r, b_r, e_c, b_cov, x2, abs(cw[42] - x2) / x2, b_x))
    assert e_r <= b_r and e_c <= b_cov and abs(cw[42] - x2) <= b_x * x2
