"""tests/pgo_weighted_ref.py against itself and against tests/pgo_ref.py: no GPU, no package code under test.
  * the fp64 restatement of the whitening and the assembly agrees with the long-double reference over cases(); the
    largest discrepancy is printed (-s) and must not exceed the recorded F64_VS_REF_W, from which the GPU tolerance follows;
  * Omega = I reproduces pgo_ref's unweighted H, g and cost;
  * a block that is not positive definite is rejected, naming the lowest such edge."""
import numpy as np
import pytest

import pgo_ref as pg
import pgo_weighted_ref as wr
import spd_ref as ref

pytestmark = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)


def test_fp64_restatement_agrees_with_the_reference(synth):
    worst, where = 0.0, None
    for key, (g, W, thr, want) in wr.cases(synth).items():
        got = wr.linearize(g, W, key[2], thr, dtype=np.float64)
        eh, eg = pg.rel_errors(got.H, got.g, want.H, want.g)
        ec = pg.cost_error(got.cost, want.cost)
        if max(eh, eg, ec) > worst:
            worst, where = max(eh, eg, ec), (key, eh, eg, ec)
    print("fp64 restatement vs long-double reference: worst %.3e at %s (H %.3e, g %.3e, cost %.3e); recorded %.3e"
          % ((worst,) + where + (wr.F64_VS_REF_W,)))
    assert worst <= wr.F64_VS_REF_W
    assert wr.GPU_TOL_W == 8.0 * wr.F64_VS_REF_W


def test_cases_cover_every_family_and_both_sides_of_the_threshold(synth):
    C = wr.cases(synth)
    assert {k[1] for k in C} == set(wr.FAMILIES) and {k[0] for k in C} >= set(wr.STORAGE_GRAPHS)
    for (name, fam, on), (g, W, thr, lin) in C.items():
        if name not in wr.STORAGE_GRAPHS:
            continue
        assert (lin.norms > thr).any() and (lin.norms < thr).any(), (name, fam)
        if fam != "identity":   # an edge the unweighted norm keeps inside the threshold and the whitened norm puts outside
            assert ((lin.raw_norms < thr) & (lin.norms > thr)).any(), (name, fam)
    lam = np.linalg.eigvalsh(wr.family("random", 40))
    assert abs(lam[0, -1] / lam[0, 0] - 1e6) < 1.0 and (lam[:, -1] / lam[:, 0]).max() <= 1e6 * (1 + 1e-6)
    R = wr.family("random", 40)
    assert np.abs(R[:, :3, 3:]).max() > 0.1        # translation and rotation are correlated


@pytest.mark.parametrize("name", ["dense30", "band120_w3", "tiny65"])
@pytest.mark.parametrize("huber", [True, False])
def test_identity_reproduces_the_unweighted_reference(synth, name, huber):
    g = wr.graphs(synth)[name][0]
    want = pg.linearize(g, huber, 0.5)
    got = wr.linearize(g, wr.family("identity", len(g.edge_a)), huber, 0.5)
    assert np.array_equal(got.H, want.H) and np.array_equal(got.g, want.g) and got.cost == want.cost


def test_cholesky_reproduces_omega_and_symmetrises():
    W = wr.family("random", 25)
    U = wr.cholesky_upper(W)
    assert np.abs(np.asarray(U.transpose(0, 2, 1) @ U, np.float64) - W).max() <= 1e-15 * np.abs(W).max()
    assert not np.tril(np.asarray(U, np.float64), -1).any()
    A = W.copy()
    A[:, 0, 5] += 1e-9
    A[:, 5, 0] -= 1e-9
    assert np.array_equal(wr.cholesky_upper(A), wr.cholesky_upper((A + A.transpose(0, 2, 1)) / 2))
    assert np.array_equal(np.asarray(wr.cholesky_upper(wr.family("four", 3)), np.float64), np.tile(2 * np.eye(6), (3, 1, 1)))


@pytest.mark.parametrize("kind", ["zero", "indefinite", "nan", "pivot_1e-40"])
def test_a_block_that_is_not_positive_definite_is_rejected(kind):
    W = wr.family("random", 9)
    W[6] = wr.bad_blocks()[kind]
    W[3] = wr.bad_blocks()[kind]
    for dtype in (wr.LD, np.float64):
        with pytest.raises(wr.NotPositiveDefinite) as e:
            wr.cholesky_upper(W, dtype)
        assert e.value.edge == 3


def test_minimize_reaches_a_stationary_point(synth):
    g = wr.tiny_graph(64)
    W = wr.family("diag", 64)
    m = wr.minimize(g, W)
    assert m.cost <= wr.total_cost(g, W, False) and m.gmax <= 1e-12 * max(1.0, np.abs(wr.linearize(g, W, False).g).max())
    assert abs(wr.total_cost(g, W, False, poses=m.poses) - m.cost) <= 1e-12 * m.cost + 1e-25
