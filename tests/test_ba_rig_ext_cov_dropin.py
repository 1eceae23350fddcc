"""visnav::bundle_adjustment_rig_extrinsics_covariance (include/visnav_amd/bundle_adjustment.h) on the mirror-type map of
tests/test_ba_rig_ext_dropin.py: it compiles against the header on the host (CPU test) and -- on the GPU box -- gives what
Context.ba_rig_ext_covariance gives on the same problem (bar 1e-6, as the rig covariance drop-in test: the wrapper
derives T_b_c and the body poses itself), and the same window with ONE fixed frame gives the "not observable" result."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_rig_ref
from pgo_ref import _ld, se3_inv, se3_mul

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/ba_rig_ext_cov_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrapper_compiles_and_links_on_the_host(tmp_path, vsl):
    assert vsl.library_path().exists()
    _compile(tmp_path / "ba_rig_ext_cov_dropin_test")


def _norm(T):
    T = np.asarray(T, np.float64).copy()
    T[..., :4] /= np.linalg.norm(T[..., :4], axis=-1, keepdims=True)
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 0])
def test_wrapper_matches_the_python_call(tmp_path, ctx, vsl, k):
    exe = _compile(tmp_path / "ba_rig_ext_cov_dropin_test")
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    E = ba_rig_ref.extrinsics()
    T_i_c = np.array([E[0], _norm(se3_mul(_ld(E[0]), _ld(E[1])).astype(np.float64))])
    T_b_c = np.array([ident, _norm(se3_mul(se3_inv(_ld(T_i_c[0])), _ld(T_i_c[1])).astype(np.float64))])   # body frame = camera 0
    rp = ba_rig_ref.rig_scene(4, 2, 12, 670 + k, T_b_c=T_b_c)
    cams = _norm(se3_mul(_ld(rp.poses)[rp.cam_body], _ld(T_b_c)[rp.cam_intr]).astype(np.float64))
    frame = np.array([10, 10, 11, 11, 12, 12, 15, 15], np.int32)
    cam_fixed = np.zeros(len(cams), np.int32)
    cam_fixed[[1, 2]] = 1                                                # one camera of frame 10 and of frame 11: both frames fixed
    with open(tmp_path / "rig.bin", "wb") as f:
        f.write(struct.pack("iii", len(cams), len(rp.points), len(rp.obs_lm)))
        for a, t in ((T_i_c, np.float64), (frame, np.int32), (rp.cam_intr, np.int32), (cam_fixed, np.int32), (cams, np.float64),
                     (rp.intr, np.float64), (rp.points, np.float64), (rp.obs_camera, np.int32), (rp.obs_lm, np.int32),
                     (rp.obs_uv, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "rig.bin"), str(tmp_path / "out.bin"), str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    # the same problem through Python: bodies = camera 0 of every frame, frames 10 and 11 fixed
    arr = vsl.BaArrays(np.zeros_like(cams), np.zeros(len(cams), np.uint8), rp.cam_intr, rp.intr, rp.points, rp.obs_camera, rp.obs_lm,
                       rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(cams[[0, 2, 4, 6]], [1, 1, 0, 0], rp.cam_body, np.full((2, 7), np.nan))
    qc = [c for c in range(len(cams)) if rp.cam_body[c] >= 2 or rp.cam_intr[c] == k]
    lms = np.arange(len(rp.points))
    want = ctx.ba_rig_ext_covariance(arr, rig, T_b_c.copy(), ext_free=(k == 0, k == 1), bodies=[2, 3], cams=qc, lms=lms)
    both = np.stack([want["cov_body"], want["cov_body_ext"][:, 0]], axis=1)                # per frame: body, cross
    flat = np.concatenate([[1.0], want["cov_ext"].ravel(), both.ravel(), want["cov_cam"].ravel(), want["cov_point"].ravel()])
    assert len(buf) == len(flat) + 1
    e = float(np.abs(buf[:-1] - flat).max())
    print("camera %d free: wrapper vs python %.3g over %d numbers; one fixed frame: observable %g" % (k, e, len(flat), buf[-1]))
    assert e <= 1e-6
    assert buf[-1] == 0.0                                                # the gauge window: "not observable"
