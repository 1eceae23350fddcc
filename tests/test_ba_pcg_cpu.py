"""Host side of the iterative-Schur route: the plain-C++ header of its host-only decisions
(visual-slam_amd/csrc/ba_pcg_plan.h, driven by tests/cpp/ba_pcg_plan_test.cpp -- also as a stand-alone sanitizer build),
the wide-map generator of tests/ba_wide_ref.py, and the premise of the GPU solve test: block-Jacobi PCG on the oracle's S
reaches 1e-12 within 4 n iterations on the seeds tests/test_ba_pcg_gpu.py uses."""
import subprocess

import numpy as np
import pytest

import ba_wide_ref as W
from conftest import ROOT

SHAPES = [(1, 16, 600), (2, 40, 1500)]  # tests/test_ba_pcg_gpu.py SHAPES


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]])
def test_plan_header(tmp_path, flags):
    exe = tmp_path / "ba_pcg_plan_test"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "visual-slam_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "ba_pcg_plan_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stderr)


@pytest.mark.parametrize("seed,n_kf,n_lms", SHAPES)
def test_wide_generator(synth, seed, n_kf, n_lms):
    d = W.wide(synth, seed, n_kf, n_lms)
    nfree = int((d["cam_fixed"] == 0).sum())
    assert nfree == 2 * n_kf - 2 > 21 and 6 * nfree > 128
    assert W.covisible_fraction(d) > 0.95                     # almost every camera pair is covisible
    assert np.bincount(d["obs_lm"]).max() <= 512               # every landmark fits a run of the recompute form
    assert np.all(np.diff(d["obs_lm"]) >= 0)                   # landmark order, as the reference hands it over
    capped = W.wide(synth, seed, n_kf, n_lms, max_obs_per_lm=8)
    assert 2 <= np.bincount(capped["obs_lm"]).min() and np.bincount(capped["obs_lm"]).max() <= 8


@pytest.mark.parametrize("seed,n_kf,n_lms", SHAPES)
def test_block_jacobi_pcg_converges_on_the_oracle_system(orc, synth, seed, n_kf, n_lms):
    d = W.wide(synth, seed, n_kf, n_lms)
    for huber in (True, False):
        S, g, _ = orc.ba_linearize(W.arrays(orc, d), use_huber=huber)
        n = len(g)
        x, it, rel = W.block_jacobi_pcg(S, g, 1e-12, 4 * n)
        assert rel <= 1e-12 and it <= 4 * n, (it, rel)
        x_ref = np.linalg.solve(S, g)
        assert np.linalg.norm(x - x_ref) <= np.linalg.cond(S) * 1e-12 * np.linalg.norm(x_ref)
    x0, it0, rel0 = W.block_jacobi_pcg(S, g, 1e-12, 0)
    assert it0 == 0 and rel0 == 1.0 and not x0.any()
