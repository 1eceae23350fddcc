"""visnav::bundle_adjustment_rig_covariance, visnav::rig_relative_pose_covariance and visnav::rig_map_edge_information
(include/visnav_amd/bundle_adjustment.h) on the mirror-type map of test_ba_rig_dropin.py: they compile against the header
on the host (CPU test) and -- on the GPU box -- give what Context.ba_rig_covariance / ba_rig_relative_pose_covariance give
on the same problem (bar 1e-6, as there; the wrapper builds T_b_c and the body poses itself)."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_rig_ref as ref
from pgo_ref import _ld, se3_exp, se3_inv, se3_mul

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/ba_rig_cov_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrappers_compile_and_link_on_the_host(tmp_path, vsl):
    assert vsl.library_path().exists()
    _compile(tmp_path / "ba_rig_cov_dropin_test")


def _norm(T):
    T = np.asarray(T, np.float64).copy()
    T[..., :4] /= np.linalg.norm(T[..., :4], axis=-1, keepdims=True)
    return T


@pytest.mark.gpu
def test_wrappers_match_the_python_calls(tmp_path, ctx, vsl):
    exe = _compile(tmp_path / "ba_rig_cov_dropin_test")
    E = ref.extrinsics()
    T_i_c = np.array([E[0], _norm(se3_mul(_ld(E[0]), _ld(E[1])).astype(np.float64))])        # body frame = camera 0
    T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], _norm(se3_mul(se3_inv(_ld(T_i_c[0])), _ld(T_i_c[1])).astype(np.float64))])
    rp = ref.rig_scene(4, 1, 12, 600, cams_of_body=[(0, 1), (0, 1), (0, 1), (1,)], T_b_c=T_b_c)
    cams = _norm(rp.cameras().astype(np.float64))
    cams[3] = _norm(se3_mul(_ld(cams[3]), se3_exp(_ld([0.03, 0, 0, 0, 0.01, 0]))).astype(np.float64))   # ignored: body from camera 0
    frame = np.array([10, 10, 11, 11, 12, 12, 15], np.int32)[:len(cams)]
    cam_fixed = np.zeros(len(cams), np.int32)
    cam_fixed[1] = 1                                                     # only the right camera of frame 10
    with open(tmp_path / "rig.bin", "wb") as f:
        f.write(struct.pack("iii", len(cams), len(rp.points), len(rp.obs_lm)))
        for a, t in ((T_i_c, np.float64), (frame, np.int32), (rp.cam_intr, np.int32), (cam_fixed, np.int32), (cams, np.float64),
                     (rp.intr, np.float64), (rp.points, np.float64), (rp.obs_camera, np.int32), (rp.obs_lm, np.int32),
                     (rp.obs_uv, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "rig.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    bodies = np.array([cams[0], cams[2], cams[4], _norm(se3_mul(_ld(cams[6]), se3_inv(_ld(T_b_c[1]))).astype(np.float64))])
    arr = vsl.BaArrays(np.zeros_like(cams), np.zeros(len(cams), np.uint8), rp.cam_intr, rp.intr, rp.points, rp.obs_camera, rp.obs_lm,
                       rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(bodies, [1, 0, 0, 0], rp.cam_body, T_b_c)
    qb, qc, ql = [1, 2, 3], [2, 3, 4, 5, 6], np.arange(len(rp.points))
    cb, cc, cl, nd = ctx.ba_rig_covariance(arr, rig, qb, qc, ql)
    pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    joint, meas, cov, info, ns = ctx.ba_rig_relative_pose_covariance(arr, rig, pairs)
    assert nd == 0 and ns == 0
    want = np.concatenate([cb.ravel(), cc.ravel(), cl.ravel(),
                           np.concatenate([np.concatenate([meas[k], cov[k].ravel(), info[k].ravel()]) for k in range(len(pairs))])])
    assert len(buf) == len(want)
    n_cov = cb.size + cc.size + cl.size
    e_cov = float(np.abs(buf[:n_cov] - want[:n_cov]).max())
    rel = np.abs(buf[n_cov:] - want[n_cov:]) / np.maximum(1.0, np.abs(want[n_cov:]))
    print("wrapper vs python: covariance blocks %.3g, relative poses (meas, cov, info; relative above 1) %.3g" % (e_cov, rel.max()))
    assert e_cov <= 1e-6 and rel.max() <= 1e-6
