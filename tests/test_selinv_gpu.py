"""vsl_spd_inverse_band (csrc/chol.hip "SELECTED INVERSION"): the band of S^-1 from the band Cholesky factor, against
the long-double inverse of tests/selinv_ref.py.  Tolerance, the project's covariance rule: max |Z - Z_ref| over the
band <= 64 cond(S) 2^-52 max |Z_ref|, cond and Z_ref from the reference (the fp64 model of the recurrence sits
10^3 - 10^4 below it: test_selinv_ref_cpu.py).  Every case prints its error beside the bound (-s)."""
import numpy as np
import pytest

import selinv_ref as sel
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]

CASES = sel.cases()
BY_NAME = {c["name"]: c for c in CASES}


def _dense(case):
    return case["bw_pass"] >= case["n"] - 1


def _band(case):
    return case["n"] if _dense(case) else case["bw"]


def _check(case, Z, S, Z_ref, tol, bw=None, label=""):
    bw = _band(case) if bw is None else bw
    err = sel.band_error(Z, Z_ref, bw, case["cyclic"])
    print("%s%s: max |Z - Z_ref| %.3e, bound %.3e" % (case["name"], label, err, tol))
    assert np.all(np.isfinite(Z))
    assert err <= tol
    assert np.array_equal(Z, Z.T)
    assert not Z[~sel.band_mask(case["n"], bw, case["cyclic"])].any()


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_band_of_the_inverse(ctx, name):
    case = BY_NAME[name]
    S, Z_ref, tol = sel.reference(case)
    Z = ctx.spd_inverse_band(S, case["bw_pass"], case["cyclic"])
    _check(case, Z, S, Z_ref, tol)
    if _dense(case):
        assert np.abs(Z).min() > 0.0   # the full inverse, not a band of it


def test_dense_route_by_a_negative_bandwidth(ctx):
    case = BY_NAME["n132_bw11"]
    S, Z_ref, tol = sel.reference(case)
    Z = ctx.spd_inverse_band(S, -1)
    err = float(np.abs(Z - Z_ref).max())
    print("n132 dense: max |Z - Z_ref| %.3e, bound %.3e" % (err, tol))
    assert err <= tol and np.array_equal(Z, Z.T)


@pytest.mark.parametrize("name", ["n132_bw11", "ring_n138_bw11"])
def test_entries_outside_the_declared_band_are_ignored(ctx, name):
    case = BY_NAME[name]
    S, _, _ = sel.reference(case)
    Z = ctx.spd_inverse_band(S, case["bw"], case["cyclic"])
    junk = np.where(sel.band_mask(case["n"], case["bw"], case["cyclic"]), S, 1e30)
    junk[np.triu_indices(case["n"], 1)] = np.nan   # the upper triangle is never read
    assert np.array_equal(ctx.spd_inverse_band(junk, case["bw"], case["cyclic"]), Z)


@pytest.mark.parametrize("name", ["n97_bw40", "ring_odd_n301_bw17"])
def test_same_bits_on_a_rerun_and_after_a_solve(ctx, name):
    case = BY_NAME[name]
    S, _, _ = sel.reference(case)
    Z = ctx.spd_inverse_band(S, case["bw"], case["cyclic"])
    assert np.array_equal(ctx.spd_inverse_band(S, case["bw"], case["cyclic"]), Z)
    other = ref.chain_spd(160, 7, 5, 1e-2)
    ctx.spd_solve(other, np.ones(160), 7)
    assert np.array_equal(ctx.spd_inverse_band(S, case["bw"], case["cyclic"]), Z)


@pytest.mark.parametrize("name,wider", [("n132_bw11", 19), ("n200_bw20", 45), ("ring_n138_bw11", 14)])
def test_a_wider_declared_band_gives_the_same_entries(ctx, name, wider):
    case = BY_NAME[name]
    S, Z_ref, tol = sel.reference(case)
    Zw = ctx.spd_inverse_band(S, wider, case["cyclic"])
    _check(case, Zw, S, Z_ref, tol, bw=wider, label=" declared %d" % wider)
    err = sel.band_error(Zw, Z_ref, case["bw"], case["cyclic"])
    assert err <= tol


def test_band_panels_route_matches(ctx):
    # the panel-by-panel launches (what bands wider than 512 take) on a small system, through the diagnostic
    case = BY_NAME["n97_bw40"]
    S, Z_ref, tol = sel.reference(case)
    ctx.set_diagnostic("chol_no_fused", 1)
    try:
        Z = ctx.spd_inverse_band(S, case["bw"])
    finally:
        ctx.set_diagnostic("chol_no_fused", 0)
    _check(case, Z, S, Z_ref, tol, label=" panel by panel")
    assert np.array_equal(Z, ctx.spd_inverse_band(S, case["bw"]))   # the same tiles in the same order


@pytest.mark.parametrize("n,bw,cyclic", [(200, 20, False), (301, 17, True)])
def test_not_positive_definite_is_numeric_and_the_context_survives(ctx, vsl, n, bw, cyclic):
    S = ref.globally_indefinite(n, bw, 7, cyclic)
    with pytest.raises(vsl.VslError) as e:
        ctx.spd_inverse_band(S, bw, cyclic)
    assert e.value.code == -7
    case = BY_NAME["n132_bw11"]
    S, Z_ref, tol = sel.reference(case)
    _check(case, ctx.spd_inverse_band(S, case["bw"]), S, Z_ref, tol, label=" after the failure")


def test_exact_structure_diagonal_and_block_diagonal(ctx):
    d = np.array([0.25, 1.0, 4.0, 16.0] * 10)
    Z = ctx.spd_inverse_band(np.diag(d), 0)
    assert np.array_equal(Z, np.diag(1.0 / d))   # Z S = I exactly: powers of four, whose square roots are exact
    d = np.random.default_rng(4).uniform(0.5, 4.0, 40)
    Z = ctx.spd_inverse_band(np.diag(d), 0)
    assert not Z[~np.eye(40, dtype=bool)].any() and np.abs(np.diag(Z) * d - 1.0).max() <= 8 * 2.0 ** -52
    # block-diagonal S (blocks of 7 inside a declared band of 6): the inverse is block diagonal with the blocks' inverses
    rng = np.random.default_rng(11)
    n, b = 70, 7
    S = np.zeros((n, n))
    for o in range(0, n, b):
        A = rng.standard_normal((b, b))
        S[o:o + b, o:o + b] = A @ A.T + b * np.eye(b)
    Z = ctx.spd_inverse_band(S, b - 1)
    blocks = np.kron(np.eye(n // b), np.ones((b, b))) > 0
    assert not Z[~blocks].any()
    assert np.abs(Z @ S - np.eye(n)).max() < 1e-13


def test_empty_system(ctx):
    assert ctx.spd_inverse_band(np.zeros((0, 0)), 3).shape == (0, 0)
    assert ctx.spd_inverse_band(np.zeros((0, 0)), -1, True).shape == (0, 0)
