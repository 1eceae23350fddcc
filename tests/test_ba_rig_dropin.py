"""visnav::bundle_adjustment_rig (include/visnav_amd/bundle_adjustment.h) on a mirror-type map: it compiles against the
header on the host (CPU test) and -- on the GPU box -- gives what Context.bundle_adjust_rig gives on the same problem
(poses and points 1e-6, the bar of two implementations of one LM trajectory; the wrapper builds T_b_c and the body poses
itself).  The map has a frame whose two cameras were pulled 3 cm apart, a frame with only its right camera (the body is
derived from it), and only ONE camera of the first frame in fixed_cameras (the body is fixed all the same)."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_rig_ref as ref
from pgo_ref import _ld, se3_exp, se3_inv, se3_mul

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/ba_rig_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrapper_compiles_and_links_on_the_host(tmp_path, vsl):
    assert vsl.library_path().exists()
    _compile(tmp_path / "ba_rig_dropin_test")


def _norm(T):
    T = np.asarray(T, np.float64).copy()
    T[..., :4] /= np.linalg.norm(T[..., :4], axis=-1, keepdims=True)
    return T


@pytest.mark.gpu
def test_wrapper_matches_the_python_call(tmp_path, ctx, vsl):
    exe = _compile(tmp_path / "ba_rig_dropin_test")
    E = ref.extrinsics()
    T_i_c = np.array([E[0], _norm(se3_mul(_ld(E[0]), _ld(E[1])).astype(np.float64))])        # body frame = camera 0
    T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], _norm(se3_mul(se3_inv(_ld(T_i_c[0])), _ld(T_i_c[1])).astype(np.float64))])
    rp = ref.rig_scene(4, 1, 12, 600, cams_of_body=[(0, 1), (0, 1), (0, 1), (1,)], T_b_c=T_b_c)
    cams = _norm(rp.cameras().astype(np.float64))
    # the right camera of frame 1 pulled 3 cm and 0.01 rad off the calibration: the wrapper takes the body from camera 0
    cams[3] = _norm(se3_mul(_ld(cams[3]), se3_exp(_ld([0.03, 0, 0, 0, 0.01, 0]))).astype(np.float64))
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
    npz, npt = 7 * len(cams), 3 * len(rp.points)
    assert len(buf) == 2 * (npz + npt)
    poses, points = buf[:npz].reshape(-1, 7), buf[npz:npz + npt].reshape(-1, 3)
    # the same problem through Python: bodies = camera 0 of a frame, or camera 1 * T_b_c[1]^-1 where it is alone
    bodies = np.array([cams[0], cams[2], cams[4], _norm(se3_mul(_ld(cams[6]), se3_inv(_ld(T_b_c[1]))).astype(np.float64))])
    arr = vsl.BaArrays(np.zeros_like(cams), np.zeros(len(cams), np.uint8), rp.cam_intr, rp.intr, rp.points, rp.obs_camera, rp.obs_lm,
                       rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(bodies, [1, 0, 0, 0], rp.cam_body, T_b_c)
    s = ctx.bundle_adjust_rig(arr, rig)
    e_p, e_l = np.abs(poses - arr.poses).max(), np.abs(points - arr.points).max()
    print("wrapper vs python: poses %.3g, points %.3g; %d iterations, cost %.6g -> %.6g" % (e_p, e_l, s.iterations, s.initial_cost, s.final_cost))
    assert s.successful_steps >= 1 and e_p <= 1e-6 and e_l <= 1e-6
    # all camera poses are written back ON the calibration, the pulled one included; frame 10 is fixed as a whole
    want = _norm(se3_mul(_ld(poses[[0, 2, 4]]), _ld(T_b_c[1])[None]).astype(np.float64))
    assert np.abs(poses[[1, 3, 5]] - want).max() <= 1e-12
    assert np.abs(poses[0] - cams[0]).max() == 0 and np.abs(poses[1] - cams[1]).max() <= 1e-12
    assert np.abs(poses[2:] - cams[2:]).max() > 1e-4
    # the second call, every frame fixed, left everything as it was
    assert np.array_equal(buf[npz + npt:], buf[:npz + npt])
