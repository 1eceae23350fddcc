"""The host plan of vsl_ba_rig_ext_covariance (visual-slam_amd/csrc/ba_rig_cov_plan.h rxcp_plan: query validation, the
union of slots that need unit columns, the slot -> column map, the pose items with their kinds, the unique landmarks, the
slot pairs), compiled with g++ as plain C++ without HIP headers and checked by tests/cpp/ba_rig_ext_cov_plan_test.cpp
against a brute-force construction over random problems and queries: duplicates, a fixed-body camera of a free block, no
free body, both blocks free, every refusal.  A second build runs under AddressSanitizer and UndefinedBehaviorSanitizer (a
stand-alone program: nothing is loaded into Python)."""
import subprocess

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "ba_rig_ext_cov_plan_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I", str(ROOT / "visual-slam_amd" / "csrc"),
                    str(SRC), "-o", str(exe)], check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    w = r.stdout.split()
    assert w[0] == "checked" and w[2] == "invalid"
    return int(w[1]), int(w[3])


def test_plan_against_brute_force(tmp_path):
    checked, invalid = _run(_build(tmp_path / "ba_rig_ext_cov_plan_test"))
    assert checked >= 450 and invalid >= 60 and checked + invalid == 600


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(_build(tmp_path / "ba_rig_ext_cov_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))
