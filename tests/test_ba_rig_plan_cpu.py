"""The host half of the rig-constrained bundle adjustment (visual-slam_amd/csrc/ba_rig_plan.h: validation of a vsl_ba_rig,
free-body numbering, camera -> body slot, observations sorted by landmark with one body's observations adjacent, the
(landmark, body) groups and the body-major gather lists), compiled with g++ as plain C++ without HIP headers and driven
by tests/cpp/ba_rig_plan_test.cpp.  The literal values are worked out by hand from the orders stated in the header; the
program verifies the plan's properties on every plan it prints and over a sweep of shapes.  A second build of the same
program runs under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is loaded into
Python)."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "ba_rig_plan_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I", str(ROOT / "visual-slam_amd" / "csrc"),
                    str(SRC), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ba_rig_plan") / "ba_rig_plan_test")


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


# three bodies, body 0 fixed; body 2 carries a right camera only; landmark 0 is seen by both cameras of body 1
FIXED, CAM_BODY, CAM_INTR = [1, 0, 0], [0, 0, 1, 1, 2], [0, 1, 0, 1, 1]
OBS = [(3, 1), (0, 0), (4, 0), (2, 1), (2, 0), (1, 1), (3, 0)]


def test_plan_by_hand(exe):
    p = _fields(_run(exe, "plan", stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS)))
    assert p["dims"] == [2, 1, 3]
    assert p["body_slot"] == [-1, 0, 1] and p["free_bodies"] == [1, 2] and p["cam_slot"] == [-1, -1, 0, 0, 1]
    # by landmark; fixed bodies first, then by slot; ties in the caller's order
    assert p["perm"] == [1, 4, 6, 2, 5, 0, 3] and p["lm_start"] == [0, 4, 7]
    # the two observations of landmark 0 / 1 from body 1 are ONE group each
    assert p["lm_grp"] == [0, 2, 3] and p["grp_lm"] == [0, 0, 1] and p["grp_slot"] == [0, 1, 0]
    assert p["grp_begin"] == [1, 3, 5] and p["grp_end"] == [3, 4, 7]
    assert p["bg_start"] == [0, 2, 3] and p["bg_grp"] == [0, 2, 1] and p["bg_lm"] == [0, 1, 0]
    assert p["bo_start"] == [0, 4, 5] and p["bo_obs"] == [1, 2, 5, 6, 3]
    assert p["extrinsic_error_below_1e-15"] == [1]


def test_rules(exe):
    ok = _problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS)
    assert _run(exe, "check", stdin=ok) == ["0 -1"]
    # RigPlanStatus: 2 empty, 3 index, 4 cam_body, 5 body without camera, 6 shared intrinsics block, 7 no free body
    assert _run(exe, "check", stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, [])) == ["2 -1"]
    assert _run(exe, "check", stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS[:3] + [(5, 0)])) == ["3 3"]
    assert _run(exe, "check", stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS[:2] + [(0, 2)])) == ["3 2"]
    assert _run(exe, "check", stdin=_problem(FIXED, CAM_BODY, [0, 1, 0, 2, 1], 2, OBS)) == ["3 3"]
    assert _run(exe, "check", stdin=_problem(FIXED, [0, 0, 1, 3, 2], CAM_INTR, 2, OBS)) == ["4 3"]
    assert _run(exe, "check", stdin=_problem(FIXED, [0, 0, 1, -1, 2], CAM_INTR, 2, OBS)) == ["4 3"]
    assert _run(exe, "check", stdin=_problem([1, 0, 0, 0], CAM_BODY, CAM_INTR, 2, OBS)) == ["5 3"]
    assert _run(exe, "check", stdin=_problem(FIXED, CAM_BODY, [0, 1, 0, 0, 1], 2, OBS)) == ["6 3"]
    assert _run(exe, "check", stdin=_problem([1, 1, 1], CAM_BODY, CAM_INTR, 2, OBS)) == ["7 -1"]
    # a body is free or fixed as a whole, whatever the caller's cam_fixed says: no fixed body is a valid plan
    assert _run(exe, "check", stdin=_problem([0, 0, 0], CAM_BODY, CAM_INTR, 2, OBS)) == ["0 -1"]


def test_sweep(exe):
    (out,) = _run(exe, "sweep")
    w = out.split()
    assert w[0] == "checked" and int(w[1]) == 9 * 3 * 4 * 4 and int(w[3]) > 1000 and int(w[5]) > 100


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path / "ba_rig_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert _run(san, "sweep")
    assert _run(san, "plan", stdin=_problem(FIXED, CAM_BODY, CAM_INTR, 2, OBS))
    assert _run(san, "check", stdin=_problem(FIXED, [0, 0, 1, 3, 2], CAM_INTR, 2, OBS))
