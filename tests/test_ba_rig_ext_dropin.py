"""visnav::bundle_adjustment_rig_extrinsics (include/visnav_amd/bundle_adjustment.h) on a mirror-type map: it compiles
against the header on the host (CPU test) and -- on the GPU box -- gives what Context.bundle_adjust_rig_ext gives on the
same problem (poses, points and the refined T_i_c to 1e-6, the bar of two implementations of one LM trajectory; the
wrapper builds T_b_c and the body poses itself and folds the refined T_b_c back into T_i_c).  Two of the four frames are
fixed; the observations are exact and the extrinsic of the free camera is handed in 5 mm / 0.3 degrees off, so the
refined T_i_c must also be the true one.  Both choices of the free camera run: for camera 0 the body frame is camera 0
AT THE CALIBRATION HANDED IN, so the refined T_b_c[0] is no longer the identity and T_i_c[0] = T_i_c[0] * T_b_c[0]."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_rig_ref
import ba_rig_ext_ref as ref
from pgo_ref import _ld, se3_inv, se3_mul

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/ba_rig_ext_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrapper_compiles_and_links_on_the_host(tmp_path, vsl):
    assert vsl.library_path().exists()
    _compile(tmp_path / "ba_rig_ext_dropin_test")


def _norm(T):
    T = np.asarray(T, np.float64).copy()
    T[..., :4] /= np.linalg.norm(T[..., :4], axis=-1, keepdims=True)
    return T


def _diff(a, b):
    """max |a - b| over poses, the quaternions compared up to sign"""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64).reshape(-1, 7)
    sign = np.where(np.sum(a[:, :4] * b[:, :4], axis=1) < 0, -1.0, 1.0)[:, None]
    return float(max(np.abs(sign * a[:, :4] - b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 0])
def test_wrapper_matches_the_python_call(tmp_path, ctx, vsl, k):
    exe = _compile(tmp_path / "ba_rig_ext_dropin_test")
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    E = ba_rig_ref.extrinsics()
    T_i_c_in = np.array([E[0], _norm(se3_mul(_ld(E[0]), _ld(E[1])).astype(np.float64))])     # the calibration handed in
    T_b_c_in = np.array([ident, _norm(se3_mul(se3_inv(_ld(T_i_c_in[0])), _ld(T_i_c_in[1])).astype(np.float64))])   # body frame = camera 0
    # the TRUE rig, in the body frame of the calibration handed in: the free camera sits 5 mm / 0.3 degrees off it
    T_b_c_true = ref.perturbed_extrinsic(T_b_c_in, k=k)
    T_i_c_true = _norm(se3_mul(_ld(T_i_c_in[0])[None], _ld(T_b_c_true)).astype(np.float64))
    rp = ba_rig_ref.rig_scene(4, 2, 12, 660 + k, T_b_c=T_b_c_true, noise=0.0)  # exact observations: the true extrinsic is THE optimum
    # the camera poses handed in lie on the calibration handed in (the wrapper takes the body from camera 0)
    cams = _norm(se3_mul(_ld(rp.poses)[rp.cam_body], _ld(T_b_c_in)[rp.cam_intr]).astype(np.float64))
    assert np.array_equal(cams[0::2], rp.poses)
    frame = np.array([10, 10, 11, 11, 12, 12, 15, 15], np.int32)
    cam_fixed = np.zeros(len(cams), np.int32)
    cam_fixed[[1, 2]] = 1                                                # one camera of frame 10 and of frame 11: both frames fixed
    with open(tmp_path / "rig.bin", "wb") as f:
        f.write(struct.pack("iii", len(cams), len(rp.points), len(rp.obs_lm)))
        for a, t in ((T_i_c_in, np.float64), (frame, np.int32), (rp.cam_intr, np.int32), (cam_fixed, np.int32), (cams, np.float64),
                     (rp.intr, np.float64), (rp.points, np.float64), (rp.obs_camera, np.int32), (rp.obs_lm, np.int32),
                     (rp.obs_uv, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "rig.bin"), str(tmp_path / "out.bin"), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    npz, npt = 7 * len(cams), 3 * len(rp.points)
    assert len(buf) == 2 * (npz + npt + 14)
    poses, points, tic = buf[:npz].reshape(-1, 7), buf[npz:npz + npt].reshape(-1, 3), buf[npz + npt:npz + npt + 14].reshape(2, 7)
    # the same problem through Python: bodies = camera 0 of every frame
    arr = vsl.BaArrays(np.zeros_like(cams), np.zeros(len(cams), np.uint8), rp.cam_intr, rp.intr, rp.points, rp.obs_camera, rp.obs_lm,
                       rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(cams[[0, 2, 4, 6]], [1, 1, 0, 0], rp.cam_body, np.full((2, 7), np.nan))
    T = T_b_c_in.copy()
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, ext_free=(k == 0, k == 1))
    want_tic = _norm(se3_mul(_ld(T_i_c_in[0]), _ld(T[k])).astype(np.float64))
    e_p, e_l, e_t = np.abs(poses - arr.poses).max(), np.abs(points - arr.points).max(), np.abs(tic[k] - want_tic).max()
    print("camera %d free, wrapper vs python: poses %.3g, points %.3g, T_i_c %.3g; %d iterations, cost %.6g -> %.6g" %
          (k, e_p, e_l, e_t, s.iterations, s.initial_cost, s.final_cost))
    assert s.successful_steps >= 1 and e_p <= 1e-6 and e_l <= 1e-6 and e_t <= 1e-6
    assert np.array_equal(tic[1 - k], T_i_c_in[1 - k]) and not np.array_equal(tic[k], T_i_c_in[k])
    # noise-free observations: the refined T_i_c is the true one, to the bar of the recovery test
    print("refined T_i_c[%d] vs the true one: %.3g (handed in %.3g off)" % (k, np.abs(tic[k] - T_i_c_true[k]).max(), np.abs(T_i_c_in[k] - T_i_c_true[k]).max()))
    assert np.abs(tic[k] - T_i_c_true[k]).max() <= 1e-6
    # every camera pose is written back on the REFINED rig, cameras == body * T_b_c: with the wrapper's own refined
    # T_b_c[j] = T_i_c_in[0]^-1 T_i_c[j] (for camera 0 no longer the identity) the two cameras of a frame name ONE body
    refined = [se3_mul(se3_inv(_ld(T_i_c_in[0])), _ld(tic[j])) for j in (0, 1)]
    body_from_0 = se3_mul(_ld(poses[0::2]), se3_inv(refined[0])[None])
    body_from_1 = se3_mul(_ld(poses[1::2]), se3_inv(refined[1])[None])
    assert _diff(body_from_0, body_from_1) <= 1e-12
    if k == 0:
        assert _diff(refined[0], ident) > 1e-3
    # the fixed frames keep their body: bit for bit where the held camera is the body frame itself
    assert _diff(body_from_1[:2], cams[[0, 2]]) <= 1e-12
    if k == 1:
        assert np.array_equal(poses[0], cams[0]) and np.array_equal(poses[2], cams[2])
    # the second call -- every frame fixed, no extrinsic free -- left everything as it was
    assert np.array_equal(buf[npz + npt + 14:], buf[:npz + npt + 14])
