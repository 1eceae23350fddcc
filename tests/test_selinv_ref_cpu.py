"""CPU: pins tests/selinv_ref.py -- the fp64 model of the panel recurrence against the long-double inverse on the case
list of the device test, the fold of a cyclic band, and the ragged-corner trap (the model with the out-of-band rows of
Z_WK dropped before Z_KK is formed must FAIL the tolerance somewhere: otherwise the device test could not tell).  No GPU;
prints what it measures (-s)."""
import numpy as np
import pytest

import selinv_ref as sel
import spd_ref as ref

needs_ld = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)
CASES = sel.cases()


def _model(case, S, zero_ragged=False):
    if case["bw_pass"] >= case["n"] - 1:
        return sel.model(S, case["n"], zero_ragged)   # the band is the whole matrix
    return (sel.model_cyclic if case["cyclic"] else sel.model)(S, case["bw"], zero_ragged)


def _band(case):
    return case["n"] if case["bw_pass"] >= case["n"] - 1 else case["bw"]


@needs_ld
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_model_matches_the_long_double_inverse(name):
    case = next(c for c in CASES if c["name"] == name)
    S, Z_ref, tol = sel.reference(case)
    Z = _model(case, S)
    err = sel.band_error(Z, Z_ref, _band(case), case["cyclic"])
    lap = sel.band_error(np.linalg.inv(S), Z_ref, _band(case), case["cyclic"])
    print("%s: model %.2e, numpy.linalg.inv %.2e, bound %.2e" % (name, err, lap, tol))
    assert err <= tol
    assert np.array_equal(Z, Z.T)
    assert not Z[~sel.band_mask(case["n"], _band(case), case["cyclic"])].any()


@needs_ld
def test_reference_inverse_is_an_inverse():
    case = next(c for c in CASES if c["name"] == "n132_bw11")
    S, Z_ref, _ = sel.reference(case)
    R = np.asarray(S, ref.LD) @ Z_ref - np.eye(case["n"], dtype=ref.LD)
    assert float(np.abs(R).max()) < 1e3 * ref.EPS_LD * sel.cond_of(S, Z_ref)


@pytest.mark.parametrize("n,bw", [(138, 11), (301, 17), (64, 3), (65, 3), (9, 1), (2, 1), (1, 0)])
def test_fold_is_a_permutation_and_at_most_doubles_the_band(n, bw):
    pos, ring = sel.fold(n)
    assert sorted(pos) == list(range(n)) and np.array_equal(pos[ring], np.arange(n))
    widest = 0
    for p in range(n):
        for d in range(1, bw + 1):
            widest = max(widest, abs(int(pos[p]) - int(pos[(p + d) % n])))
    assert widest <= 2 * bw
    if n > 2 * bw + 1:
        assert widest == 2 * bw   # two positions on the same half of the ring


@pytest.mark.parametrize("n,bw", [(138, 11), (301, 17)])
def test_fold_of_a_ring_matrix(n, bw):
    S = ref.chain_spd(n, bw, 3, 1e-4, True)
    A = sel.folded(S)
    assert ref.half_bandwidth(A) == 2 * bw
    pos, _ = sel.fold(n)
    assert np.array_equal(A[np.ix_(pos, pos)], S)


@needs_ld
def test_dropping_the_ragged_corner_is_caught():
    worst = 0.0
    for case in CASES:
        if case["bw"] == 0 or case["bw_pass"] >= case["n"] - 1:
            continue
        S, Z_ref, tol = sel.reference(case)
        err = sel.band_error(_model(case, S, zero_ragged=True), Z_ref, _band(case), case["cyclic"])
        print("%s: ragged rows dropped: error %.2e, bound %.2e" % (case["name"], err, tol))
        worst = max(worst, err / tol)
    assert worst > 1.0
