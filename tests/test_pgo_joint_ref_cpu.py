"""CPU checks of tests/pgo_joint_ref.py, the reference of the joint-covariance and edge-consistency GPU tests: the
four-product formula of Sigma_r against a brute-force first-order propagation of the whole covariance, symmetry, the
zero block of a fixed node, and the long-double chi-square against a plain solve."""
import numpy as np
import pytest

import pgo_joint_ref as jr
import pgo_ref as pg
import spd_ref as ref

pytestmark = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)


@pytest.mark.parametrize("name", ["dense4", "chain30_w2_fixed_middle"])
def test_resid_cov_of_existing_edges_against_the_whole_covariance(name):
    c = jr.case(name)
    g = c.g
    worst = 0.0
    for e in range(0, len(g.edge_a), 3):
        a, b = int(g.edge_a[e]), int(g.edge_b[e])
        if c.free[a] < 0 and c.free[b] < 0:
            continue
        r, S, Ja, Jb, _ = jr.resid_cov(c, a, b, g.edge_meas[e])
        B = jr.resid_cov_brute(c, a, b, g.edge_meas[e])
        scale = float(np.abs(B).max())
        worst = max(worst, float(np.abs(S - B).max()) / scale)
        assert np.array_equal(S, S.T)
        assert np.array_equal(r, pg.residual(pg._ld(g.poses)[a], pg._ld(g.poses)[b], g.edge_meas[e]))
    print("%s: four products vs whole covariance, worst relative difference %.3e" % (name, worst))
    assert worst <= 1e-15   # long double: 2^-63 ~ 1.1e-19 per operation, sums of at most 6 n terms


def test_joint_block_is_symmetric_and_swaps():
    c = jr.case("chain30_w2_fixed_middle")
    for a, b in jr.pairs_of("chain30_w2_fixed_middle"):
        S, T = jr.joint_block(c, a, b), jr.joint_block(c, b, a)
        assert float(np.abs(S - S.T).max()) <= 1e-17 * float(np.abs(S).max())   # Z itself is symmetric to rounding
        assert np.array_equal(S[:6, :6], T[6:, 6:]) and np.array_equal(S[:6, 6:], T[6:, :6])


def test_fixed_node_gives_a_zero_block_and_drops_its_term():
    c = jr.case("chain30_w2_fixed_middle")
    S = jr.joint_block(c, 15, 7)
    assert not S[:6, :].any() and not S[:, :6].any() and S[6:, 6:].any()
    meas = np.zeros(6)
    _, Sr, Ja, Jb, _ = jr.resid_cov(c, 15, 7, meas)
    assert not Ja.any()
    M = Jb @ c.Z[6 * 7:6 * 7 + 6, 6 * 7:6 * 7 + 6] @ Jb.T
    assert np.array_equal(Sr, (M + M.T) / 2)


def test_chi2_by_cholesky():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(6, 6))
    A = B @ B.T + 0.1 * np.eye(6)
    r = rng.normal(size=6)
    want = float(r @ np.linalg.solve(A, r))
    assert abs(jr.chi2_ld(r, A) - want) <= 1e-12 * want
    assert np.isnan(jr.chi2_ld(r, -A))
    assert jr.chi2_ld(np.zeros(6), A) == 0.0
