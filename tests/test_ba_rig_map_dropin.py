"""visnav::global_bundle_adjustment_rig (include/visnav_amd/bundle_adjustment.h) on a mirror-type map: it compiles
against the header on the host (CPU test) and -- on the GPU box -- gives what Context.global_bundle_adjust_rig gives on
the same problem, by the bars of tests/test_ba_rig_dropin.py (poses and points 1e-6; the wrapper builds T_b_c and the
body poses itself).  The map is the ring case of tests/ba_rig_map_cases.py (41 frames, window 5: cyclic band) with the
body frame on camera 0, one frame whose right camera was pulled 3 cm off the calibration, one frame that has its right
camera only, and only ONE camera of the first frame in fixed_cameras."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_rig_ref as ref
from pgo_ref import _ld, se3_exp, se3_inv, se3_mul

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests/cpp/ba_rig_map_dropin_test.cpp"),
           "-o", str(out), "-L", str(ROOT / "visual-slam_amd"), "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_wrapper_compiles_and_links_on_the_host(tmp_path, vsl):
    assert vsl.library_path().exists()
    _compile(tmp_path / "ba_rig_map_dropin_test")


def _norm(T):
    T = np.asarray(T, np.float64).copy()
    T[..., :4] /= np.linalg.norm(T[..., :4], axis=-1, keepdims=True)
    return T


@pytest.mark.gpu
def test_wrapper_matches_the_python_call(tmp_path, ctx, vsl):
    exe = _compile(tmp_path / "ba_rig_map_dropin_test")
    E = ref.extrinsics()
    T_i_c = np.array([E[0], _norm(se3_mul(_ld(E[0]), _ld(E[1])).astype(np.float64))])        # body frame = camera 0
    T_b_c = np.array([[0, 0, 0, 1.0, 0, 0, 0], _norm(se3_mul(se3_inv(_ld(T_i_c[0])), _ld(T_i_c[1])).astype(np.float64))])
    nb = 41
    rp = ref.rig_scene(nb, 1, 40, 602, window=5, cams_of_body=[(0, 1)] * 20 + [(1,)] + [(0, 1)] * 20, T_b_c=T_b_c)
    cams = _norm(rp.cameras().astype(np.float64))
    pulled = 3                                                           # the right camera of frame 1
    assert rp.cam_body[pulled] == 1 and rp.cam_intr[pulled] == 1
    cams[pulled] = _norm(se3_mul(_ld(cams[pulled]), se3_exp(_ld([0.03, 0, 0, 0, 0.01, 0]))).astype(np.float64))
    frame = (10 + 2 * rp.cam_body).astype(np.int32)                      # frame ids with gaps, ascending with the body
    cam_fixed = np.zeros(len(cams), np.int32)
    cam_fixed[1] = 1                                                     # only the right camera of the first frame
    with open(tmp_path / "rig.bin", "wb") as f:
        f.write(struct.pack("iii", len(cams), len(rp.points), len(rp.obs_lm)))
        for a, t in ((T_i_c, np.float64), (frame, np.int32), (rp.cam_intr, np.int32), (cam_fixed, np.int32), (cams, np.float64),
                     (rp.intr, np.float64), (rp.points, np.float64), (rp.obs_camera, np.int32), (rp.obs_lm, np.int32),
                     (rp.obs_uv, np.float64)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "rig.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[:3] == ["layout", "2", "29"], r.stdout       # the cyclic band of the ring case
    buf = np.fromfile(tmp_path / "out.bin", np.float64)
    npz, npt = 7 * len(cams), 3 * len(rp.points)
    assert len(buf) == 2 * (npz + npt)
    poses, points = buf[:npz].reshape(-1, 7), buf[npz:npz + npt].reshape(-1, 3)
    # the same problem through Python: bodies = camera 0 of a frame, or camera 1 * T_b_c[1]^-1 where it is alone
    first = np.array([int(np.flatnonzero(rp.cam_body == b)[0]) for b in range(nb)])
    bodies = cams[first].copy()
    alone = rp.cam_intr[first] == 1
    assert alone.sum() == 1 and alone[20]
    bodies[alone] = _norm(se3_mul(_ld(cams[first[alone]]), se3_inv(_ld(T_b_c[1]))[None]).astype(np.float64))
    arr = vsl.BaArrays(np.zeros_like(cams), np.zeros(len(cams), np.uint8), rp.cam_intr, rp.intr, rp.points, rp.obs_camera, rp.obs_lm,
                       rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(bodies, rp.cam_fixed, rp.cam_body, T_b_c)
    s = ctx.global_bundle_adjust_rig(arr, rig)
    assert ctx.last_ba_layout()[1:] == (2, 29)
    e_p, e_l = np.abs(poses - arr.poses).max(), np.abs(points - arr.points).max()
    print("wrapper vs python: poses %.3g, points %.3g; %d iterations, cost %.6g -> %.6g" % (e_p, e_l, s.iterations, s.initial_cost, s.final_cost))
    assert s.successful_steps >= 1 and e_p <= 1e-6 and e_l <= 1e-6
    # all camera poses are written back ON the calibration, the pulled one included; the first frame is fixed as a whole
    both = np.array([b for b in range(nb) if (rp.cam_body == b).sum() == 2])
    left, right = first[both], first[both] + 1
    want = _norm(se3_mul(_ld(poses[left]), _ld(T_b_c[1])[None]).astype(np.float64))
    assert np.abs(poses[right] - want).max() <= 1e-12
    assert np.abs(poses[0] - cams[0]).max() == 0 and np.abs(poses[1] - cams[1]).max() <= 1e-12
    assert np.abs(poses[2:] - cams[2:]).max() > 1e-4
    # the second call, every frame fixed, left everything as it was
    assert np.array_equal(buf[npz + npt:], buf[:npz + npt])
