"""visnav::relative_pose_covariance (both overloads, include/visnav_amd/bundle_adjustment.h) and
visnav::map_edge_information (include/visnav_amd/loop_closure.h) on a small mirror-type map, driven by
tests/cpp/relative_pose_covariance_test.cpp: on the host the enumeration of the pose-graph edges that the map can answer;
on the GPU both overloads beside the C ABI on the same flattened problem (bit for bit: the program compares the bytes),
and map_edge_information handed to pose_graph_optimization, answering the default for the loop edge."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ba_cov_ref as R

ROOT = Path(__file__).resolve().parents[1]


def _compile(out):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", str(ROOT / "include"),
           str(ROOT / "tests/cpp/relative_pose_covariance_test.cpp"), "-o", str(out), "-L", str(ROOT / "visual-slam_amd"),
           "-lvslam_hip", "-Wl,-rpath," + str(ROOT / "visual-slam_amd")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def _write(path, d, pairs):
    qc = np.asarray(pairs, np.int32).reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("iiiii", len(d["poses"]), len(d["points"]), len(d["obs_cam"]), len(qc), 0))
        for a, t in ((d["poses"], np.float64), (d["cam_fixed"], np.uint8), (d["intr"], np.float64),
                     (d["points"], np.float64), (d["obs_cam"], np.int32), (d["obs_lm"], np.int32),
                     (d["obs_uv"], np.float64), (qc, np.int32)):
            f.write(np.ascontiguousarray(a, t).tobytes())


# cameras 0 and 1 (frame 0) are fixed: a pair with a fixed camera either way round, left-left, left-right, far
PAIRS = [(2, 4), (4, 2), (0, 6), (7, 1), (2, 3), (9, 2), (6, 8), (8, 4)]


def _problem(synth):
    return R.problem(synth, 5, n_free=8, n_lms=60)     # five frames, ten cameras


def test_map_edges_are_enumerated_on_the_host(tmp_path, vsl, synth):
    assert vsl.library_path().exists()
    exe = _compile(tmp_path / "relative_pose_covariance_test")
    _write(tmp_path / "ba.bin", _problem(synth), PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "ba.bin"), "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    # frames 1 .. 4 with the one or two frames before them: 1 + 2 + 2 + 2
    assert r.stdout.startswith("host ok: 7 map edges of 5 keyframes")


@pytest.mark.gpu
def test_overloads_match_the_c_abi_and_the_pose_graph_takes_the_map_information(tmp_path, synth):
    exe = _compile(tmp_path / "relative_pose_covariance_test")
    _write(tmp_path / "ba.bin", _problem(synth), PAIRS)
    r = subprocess.run([str(exe), str(tmp_path / "ba.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.strip().endswith("drop-in ok: 8 pairs on both overloads, 7 map edges, loop edge answered with the default")
