"""The 6 x 6 steps of ba_relpose_kernel (visual-slam_amd/csrc/relpose_math.h: Cholesky factor, inverse of the factor,
Omega, the 2^-36 pivot rule on Sigma_r and the consumer's rule on Omega), compiled with g++ as plain C++ and driven by
tests/cpp/relpose_math_test.cpp on hand-built matrices: the NaN / singular branches that no bundle-adjustment input
reaches on the device run here, through the very functions the kernel calls.  A second build runs under
AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is loaded into Python)."""
import subprocess

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "relpose_math_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I",
                    str(ROOT / "visual-slam_amd" / "csrc"), str(SRC), "-o", str(exe)], check=True)
    return exe


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def test_factor_invert_and_pivot_rules(tmp_path):
    out = _run(_build(tmp_path / "relpose_math_test"))
    assert out[0] == "exact ok"
    assert out[1] == "boundary ok: last accepted k 17, first refused k 18"
    assert out[2] == "refusals ok"
    w = out[3].split()
    assert w[:3] == ["sweep", "ok:", "accepted"] and int(w[3].rstrip(",")) > 100


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    out = _run(_build(tmp_path / "relpose_math_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))
    assert out[2] == "refusals ok" and out[3].startswith("sweep ok")
