"""The host arithmetic of the selected inversion (visual-slam_amd/csrc/chol_plan.h: chol_fold_plan, chol_selinv_plan),
compiled with g++ as plain C++ without HIP headers and driven by tests/cpp/selinv_plan_test.cpp; the fold is compared
with its restatement in tests/selinv_ref.py.  A second build of the same program runs under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program: nothing is loaded into Python)."""
import subprocess

import numpy as np
import pytest

import selinv_ref as sel
from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "selinv_plan_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", str(ROOT / "visual-slam_amd" / "csrc"), str(SRC),
                    "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("selinv_plan") / "selinv_plan_test")


def _run(exe, *args):
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return r.stdout.splitlines()


@pytest.mark.parametrize("n,bw,folded_bw", [(138, 11, 22), (301, 17, 34), (24, 11, 22), (25, 11, 22), (9, 1, 2), (5, 3, 4), (1, 0, 0)])
def test_fold_matches_the_reference_permutation(exe, n, bw, folded_bw):
    head, pos, ring = _run(exe, "fold", n, bw)
    pbw, band, widest = map(int, head.split())
    rpos, rring = sel.fold(n)
    assert np.array_equal(np.array(pos.split(), int), rpos) and np.array_equal(np.array(ring.split(), int), rring)
    assert pbw == folded_bw and widest <= pbw and band == int(0 <= 2 * bw < n - 1)
    if n > 2 * bw + 1:
        assert widest == 2 * bw


def test_sweep_of_fold_and_plan(exe):
    assert _run(exe, "sweep") == [str(sum(min(n, 40) + 1 for n in range(1, 401)))]


def test_plan_literals(exe):
    # n_panels fused window Linv G scratch_doubles z_elems
    assert _run(exe, "plan", 132, 11, 0) == ["5 1 11 0 5120 %d %d" % (5120 + (11 + 16) * 32 + 16, 132 * 44 + 64)]
    assert _run(exe, "plan", 3000, 41, 0) == ["94 1 41 0 96256 %d %d" % (96256 + 57 * 32 + 16, 3000 * 74 + 64)]
    assert _run(exe, "plan", 3000, 513, 0)[0].split()[1] == "0"     # wider than the single-workgroup kernels: panel by panel
    assert _run(exe, "plan", 3000, 41, 1)[0].split()[1] == "0"      # "chol_no_fused"
    assert _run(exe, "plan", 20, 30, 0) == ["1 1 0 0 1024 %d %d" % (1024 + 16 * 32 + 16, 20 * 63 + 64)]


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path / "selinv_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert _run(san, "sweep")
    assert _run(san, "fold", 301, 17)
