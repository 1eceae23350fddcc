"""The host set-up of the rig bundle adjustment with the extrinsics as unknowns (visual-slam_amd/csrc/ba_rig_plan.h
"EXTRINSICS": the slot of a free extrinsic block, camera -> extrinsic slot, the pose-block table, the (landmark, slot)
groups with their observation index lists and the per-slot group / observation lists), compiled with g++ as plain C++
without HIP headers and driven by tests/cpp/ba_rig_ext_plan_test.cpp.  The literal values are worked out by hand from the
orders stated in the header; the program compares every plan it builds with a brute-force construction (maps and sets,
no shared code) over a sweep of shapes that includes the empty body lists of the no-free-body case.  A second build of
the same program runs under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is loaded
into Python)."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "ba_rig_ext_plan_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I", str(ROOT / "visual-slam_amd" / "csrc"),
                    str(SRC), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ba_rig_ext_plan") / "ba_rig_ext_plan_test")


def _run(exe, *args, stdin=""):
    r = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _fields(lines):
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines}


def _problem(body_fixed, cam_body, cam_intr, n_lms, obs):
    j = lambda v: " ".join(map(str, v))  # noqa: E731
    return "%d\n%s\n%d\n%s\n%s\n%d %d\n%s\n%s\n" % (len(body_fixed), j(body_fixed), len(cam_body), j(cam_body), j(cam_intr), n_lms,
                                                 len(obs), j(o[0] for o in obs), j(o[1] for o in obs))


# the problem of test_ba_rig_plan_cpu.py: three bodies, body 0 fixed; body 2 carries a right camera only.  Sorted
# observations (camera, landmark): 0 (0, 0)  1 (2, 0)  2 (3, 0)  3 (4, 0)  4 (1, 1)  5 (3, 1)  6 (2, 1)
FIXED, CAM_BODY, CAM_INTR = [1, 0, 0], [0, 0, 1, 1, 2], [0, 1, 0, 1, 1]
OBS = [(3, 1), (0, 0), (4, 0), (2, 1), (2, 0), (1, 1), (3, 0)]


def test_plan_by_hand_block_1_free(exe):
    p = _fields(_run(exe, "plan", 0, 1, stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS)))
    assert p["dims"] == [3, 1, 5] and p["ext_slot"] == [-1, 2]
    assert p["cam_eslot"] == [-1, 2, -1, 2, 2] and p["pose_free"] == [-1, 0, 1, -1, 2]
    # per landmark: the body groups in ascending slot, then the extrinsic group; the camera of the FIXED body 0 on block 1
    # (observation 4) is in the extrinsic group of landmark 1
    assert p["lm_grp"] == [0, 3, 5] and p["grp_lm"] == [0, 0, 0, 1, 1] and p["grp_slot"] == [0, 1, 2, 0, 2]
    assert p["grp_first"] == [0, 2, 3, 5, 7, 9] and p["grp_obs"] == [1, 2, 3, 2, 3, 5, 6, 4, 5]
    assert p["sg_start"] == [0, 2, 3, 5] and p["sg_grp"] == [0, 3, 1, 2, 4] and p["sg_lm"] == [0, 1, 0, 0, 1]
    assert p["so_start"] == [0, 4, 5, 9] and p["so_obs"] == [1, 2, 5, 6, 3, 2, 3, 4, 5]


def test_plan_by_hand_both_free_and_no_free_body(exe):
    p = _fields(_run(exe, "plan", 1, 1, stdin=_problem([1, 1, 1], CAM_BODY, CAM_INTR, 2, OBS)))
    # every body fixed: the slots are the two blocks, the body lists are empty.  Sorted order with every body fixed:
    # ties in the caller's order: 0 (0, 0)  1 (4, 0)  2 (2, 0)  3 (3, 0)  4 (3, 1)  5 (2, 1)  6 (1, 1)
    assert p["dims"] == [2, 2, 4] and p["ext_slot"] == [0, 1] and p["pose_free"] == [-1, -1, -1, 0, 1]
    assert p["cam_eslot"] == [0, 1, 0, 1, 1]
    assert p["grp_lm"] == [0, 0, 1, 1] and p["grp_slot"] == [0, 1, 0, 1]
    assert p["grp_first"] == [0, 2, 4, 5, 7] and p["grp_obs"] == [0, 2, 1, 3, 5, 4, 6]
    assert p["sg_start"] == [0, 2, 4] and p["sg_grp"] == [0, 2, 1, 3] and p["so_start"] == [0, 3, 7] and p["so_obs"] == [0, 2, 5, 1, 3, 4, 6]


def test_rules(exe):
    ok = _problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS)
    assert _run(exe, "check", 0, 1, stdin=ok) == ["0 -1"]
    # what the rig plan refuses stays refused: 3 index, 4 cam_body, 5 body without camera, 6 shared intrinsics block
    assert _run(exe, "check", 0, 1, stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS[:3] + [(5, 0)])) == ["3 3"]
    assert _run(exe, "check", 0, 1, stdin=_problem(FIXED, [0, 0, 1, 3, 2], CAM_INTR, 2, OBS)) == ["4 3"]
    assert _run(exe, "check", 1, 0, stdin=_problem([1, 0, 0, 0], CAM_BODY, CAM_INTR, 2, OBS)) == ["5 3"]
    assert _run(exe, "check", 1, 1, stdin=_problem(FIXED, CAM_BODY, [0, 1, 0, 0, 1], 2, OBS)) == ["6 3"]
    # every body fixed is a plan while a block is free; nothing free at all is status 10
    assert _run(exe, "check", 0, 1, stdin=_problem([1, 1, 1], CAM_BODY, CAM_INTR, 2, OBS)) == ["0 -1"]
    assert _run(exe, "check", 0, 0, stdin=_problem([1, 1, 1], CAM_BODY, CAM_INTR, 2, OBS)) == ["10 -1"]
    # 9: a free block that no camera carries (every camera on block 0, block 1 free)
    assert _run(exe, "check", 0, 1, stdin=_problem([1, 0], [0, 1], [0, 0], 2, [(0, 0), (1, 0), (0, 1), (1, 1)])) == ["9 1"]
    assert _run(exe, "check", 1, 0, stdin=_problem([1, 0], [0, 1], [0, 0], 2, [(0, 0), (1, 0), (0, 1), (1, 1)])) == ["0 -1"]


def test_sweep_against_the_brute_force_construction(exe):
    (out,) = _run(exe, "sweep")
    w = out.split()
    assert w[0] == "checked" and int(w[1]) + int(w[7]) == 7 * 4 * 4 * 3 * 3 and int(w[3]) > 1000 and int(w[5]) > 100 and int(w[7]) > 10


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path / "ba_rig_ext_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert _run(san, "sweep")
    assert _run(san, "plan", 0, 1, stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS))
    assert _run(san, "plan", 1, 1, stdin=_problem([1, 1, 1], CAM_BODY, CAM_INTR, 2, OBS))
    assert _run(san, "check", 0, 1, stdin=_problem(FIXED, [0, 0, 1, 3, 2], CAM_INTR, 2, OBS))
