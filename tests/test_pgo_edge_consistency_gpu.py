"""vsl_pgo_edge_consistency: residual, residual covariance and chi-square of candidate edges against the long-double
reference of tests/pgo_joint_ref.py.  Bounds (printed beside the measured errors, -s):
  resid      |r - ref| <= pgo_ref.GPU_TOL x max |log(T_a^-1 T_b)|: the relative tolerance of the linearise tests, taken on
             the logarithm (the subtraction of the measurement adds one rounding of at most that size)
  resid_cov  tol_block (|Ja|_inf + |Jb|_inf)^2 + tol_J 2 max|Sigma| (|Ja|_inf + |Jb|_inf), tol_block = the covariance rule
             selinv_ref.tolerance(H, Z), tol_J = GPU_TOL x max |J| (the linearise tests' Jacobian tolerance)
  chi2       relative: 64 cond(Sigma_r + Sigma_m) x (the resid_cov bound / max |Sigma_r|)
A candidate equal to the current relative pose: the measurement fed back is the device's own logarithm, so r and chi2
are EXACTLY zero."""
import numpy as np
import pytest

import pgo_joint_ref as jr
import pgo_ref as pg
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]

LD = pg.LD
# graph -> candidates (a, b): a far pair (solved), an in-band pair (read), the fixed node on either side, one more far pair
CANDS = {
    "dense4": [(1, 3), (3, 2), (0, 2), (1, 0)],
    "chain30_w2_fixed_middle": [(0, 29), (3, 4), (15, 7), (20, 15), (27, 5), (3, 6)],
    "ring26_odd": [(1, 13), (4, 5), (0, 9), (17, 0), (25, 12), (1, 25)],
    "ring26_outliers_huber_on": [(1, 13), (4, 5), (0, 9), (22, 6)],
}


def _norm_inf(J):
    return float(np.abs(J).sum(axis=1).max())


def _reference(c, cands, meas, meas_cov=None):
    """per candidate: r, Sigma_r, bound on Sigma_r, chi2, relative bound on chi2, bound on r"""
    out = []
    P = pg._ld(c.g.poses)
    for q, (a, b) in enumerate(cands):
        r, Sr, Ja, Jb, S = jr.resid_cov(c, a, b, meas[q])
        nj = _norm_inf(Ja) + _norm_inf(Jb)
        tol_j = pg.GPU_TOL * float(max(np.abs(Ja).max(), np.abs(Jb).max()))
        b_cov = c.tol * nj * nj + tol_j * 2 * float(np.abs(S).max()) * nj
        A = Sr if meas_cov is None else Sr + pg._ld(meas_cov[q])
        A64 = np.asarray(A, np.float64)
        cond = float(np.linalg.cond(A64)) if np.all(np.linalg.eigvalsh(A64) > 0) else float("inf")
        b_chi = 64 * cond * b_cov / float(np.abs(Sr).max())
        b_r = pg.GPU_TOL * float(np.abs(pg.residual(P[a], P[b], np.zeros(6))).max())
        out.append((r, Sr, b_cov, jr.chi2_ld(r, A), b_chi, b_r))
    return out


def _meas(c, cands, seed, scale):
    """measurements near the current relative poses: log(T_a^-1 T_b) + scale x N(0, 1)"""
    rng = np.random.default_rng(seed)
    P = pg._ld(c.g.poses)
    return np.stack([(pg.residual(P[a], P[b], np.zeros(6)) + LD(scale) * rng.normal(size=6)).astype(np.float64) for a, b in cands])


def _call(ctx, c, cands, meas, meas_cov=None):
    a, b = [p[0] for p in cands], [p[1] for p in cands]
    return ctx.pgo_edge_consistency(c.g, a, b, meas, meas_cov, use_huber=c.use_huber, huber=c.huber)


def _check(c, cands, got, want, label=""):
    resid, cov, chi2, _ = got
    worst = [0.0, 0.0, 0.0]
    for q, (r, Sr, b_cov, x2, b_chi, b_r) in enumerate(want):
        e_r = float(np.abs(resid[q] - r).max())
        e_c = float(np.abs(cov[q] - Sr).max())
        e_x = abs(float(chi2[q]) - x2) / x2 if x2 > 0 else abs(float(chi2[q]))
        print("%s%s %s: resid %.3e (bound %.3e)  resid_cov %.3e (bound %.3e, ratio %.2e)  chi2 %.6g rel %.3e (bound %.3e, ratio %.2e)"
              % (c.name, label, cands[q], e_r, b_r, e_c, b_cov, e_c / b_cov, x2, e_x, b_chi, e_x / b_chi))
        assert e_r <= b_r and e_c <= b_cov and e_x <= b_chi, cands[q]
        worst = [max(w, v) for w, v in zip(worst, (e_r / b_r, e_c / b_cov, e_x / b_chi))]
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    return worst


@pytest.mark.parametrize("name", list(CANDS))
def test_residual_covariance_and_chi2(ctx, name):
    c = jr.case(name)
    cands = CANDS[name]
    meas = _meas(c, cands, 11, 0.05)
    before = c.g.poses.copy()
    got = _call(ctx, c, cands, meas)
    assert got[3] == c.route
    assert np.array_equal(c.g.poses, before)
    _check(c, cands, got, _reference(c, cands, meas))
    # resid_cov is the propagation of the joint covariance the other call returns, and does not depend on the measurement
    again = _call(ctx, c, cands, meas)
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], again[:3]))
    other = _call(ctx, c, cands, _meas(c, cands, 12, 0.2))
    assert np.array_equal(other[1], got[1])
    # a candidate alone returns the bits it has in company
    for q in range(len(cands)):
        one = _call(ctx, c, cands[q:q + 1], meas[q:q + 1])
        assert all(np.array_equal(one[k][0], got[k][q]) for k in range(3)), cands[q]


@pytest.mark.parametrize("name", ["chain30_w2_fixed_middle", "ring26_odd"])
def test_routes_agree(ctx, name):
    c = jr.case(name)
    cands = CANDS[name]
    meas = _meas(c, cands, 11, 0.05)
    want = _reference(c, cands, meas)
    for knob in ("pgo_cov_no_band_read", "ba_force_dense"):
        ctx.set_diagnostic(knob, 1)
        try:
            got = _call(ctx, c, cands, meas)
        finally:
            ctx.set_diagnostic(knob, 0)
        assert got[3] == (0 if knob == "ba_force_dense" else c.route)
        _check(c, cands, got, want, " " + knob)


@pytest.mark.parametrize("name", ["chain30_w2_fixed_middle", "ring26_odd"])
def test_current_relative_pose_is_exactly_consistent(ctx, name):
    c = jr.case(name)
    cands = CANDS[name]
    log_dev = _call(ctx, c, cands, np.zeros((len(cands), 6)))[0]     # r = log(T_a^-1 T_b) - 0
    resid, cov, chi2, _ = _call(ctx, c, cands, log_dev)
    assert not resid.any() and not chi2.any()       # exactly zero: the same logarithm minus itself
    assert np.all(np.linalg.eigvalsh(cov) > 0)


@pytest.mark.parametrize("name", ["chain30_w2_fixed_middle", "ring26_odd"])
def test_k_sigma_along_a_principal_axis(ctx, name):
    c = jr.case(name)
    cands = CANDS[name]
    P = pg._ld(c.g.poses)
    for k, axis in ((1.0, 0), (3.0, 5), (0.5, 2)):
        meas = []
        for a, b in cands:
            _, Sr, _, _, _ = jr.resid_cov(c, a, b, np.zeros(6))
            lam, V = np.linalg.eigh(np.asarray(Sr, np.float64))
            meas.append((pg.residual(P[a], P[b], np.zeros(6)) - LD(k) * LD(np.sqrt(lam[axis])) * pg._ld(V[:, axis])).astype(np.float64))
        meas = np.stack(meas)
        got = _call(ctx, c, cands, meas)
        want = _reference(c, cands, meas)
        _check(c, cands, got, want, " k = %g axis %d" % (k, axis))
        for q, w in enumerate(want):
            # the reference chi2 itself is k^2 up to the rounding of the measurement to double and of eigh
            assert abs(w[3] - k * k) <= 1e-6 * k * k
            assert abs(got[2][q] - k * k) <= (w[4] + 1e-6) * k * k


def test_measurement_covariance(ctx):
    c = jr.case("ring26_odd")
    cands = CANDS["ring26_odd"]
    n = len(cands)
    meas = _meas(c, cands, 13, 0.05)
    base = _call(ctx, c, cands, meas)
    zeros = _call(ctx, c, cands, meas, np.zeros((n, 6, 6)))
    assert all(np.array_equal(x, y) for x, y in zip(base[:3], zeros[:3]))     # NULL = zeros, bit for bit
    rng = np.random.default_rng(4)
    B = rng.normal(size=(n, 6, 6))
    mc = 1e-3 * (B @ B.transpose(0, 2, 1)) + 1e-4 * np.eye(6)
    got = _call(ctx, c, cands, meas, mc)
    _check(c, cands, got, _reference(c, cands, meas, mc), " with meas_cov")
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
    assert np.all(got[2] < base[2])                                           # more noise allowed: more consistent
    # a negative definite meas_cov on ONE candidate: NaN there, the others keep their bits
    mc2 = mc.copy()
    mc2[2] = -1e3 * np.eye(6)
    bad = _call(ctx, c, cands, meas, mc2)
    assert np.isnan(bad[2][2]) and np.array_equal(np.delete(bad[2], 2), np.delete(got[2], 2))
    assert np.array_equal(bad[0], got[0]) and np.array_equal(bad[1], got[1])


def test_invalid_candidates_and_an_empty_list(ctx, vsl):
    c = jr.case("ring26_odd")
    for a, b in ((3, 3), (-1, 2), (2, 26)):
        with pytest.raises(vsl.VslError) as e:
            ctx.pgo_edge_consistency(c.g, [a], [b], np.zeros((1, 6)))
        assert e.value.code == -1
    resid, cov, chi2, storage = ctx.pgo_edge_consistency(c.g, [], [], np.zeros((0, 6)))
    assert resid.shape == (0, 6) and cov.shape == (0, 6, 6) and chi2.shape == (0,) and storage == 2
    g = pg.loop_graph(40, noise=2e-3, seed=31)   # free gauge
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_edge_consistency(g, [0], [20], np.zeros((1, 6)))
    assert e.value.code == -7
    assert ctx.pgo_edge_consistency(c.g, [1], [13], np.zeros((1, 6)))[3] == 2
