"""tests/pgo_far_ref.py (the long-double restatement of the far-edge split and of the identity x = y - Y z) pinned
against direct solves with the dense H, for every shape tests/test_pgo_far_gpu.py hands to the hook."""
import numpy as np
import pytest

import pgo_far_ref as fr
import pgo_ref as pg
import spd_ref as ref

pytestmark = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)


@pytest.mark.parametrize("name", list(fr.hook_cases()))
def test_identity_agrees_with_the_dense_solve(name):
    g, W, hub, thr, d_star, k = fr.hook_cases()[name]
    R = fr.hook_reference(name)
    n = g.n_unknowns()
    assert R.k == k and R.W.shape == (n, 6 * k)
    # the split is exact: the same products summed into two matrices instead of one
    assert float(np.abs(R.M + R.W @ R.W.T - R.H_ld).max()) <= 2.0 ** -60 * float(np.abs(R.H_ld).max())
    if W is None:
        lin = pg.linearize(g, hub, thr)
        assert float(np.abs(lin.H - R.lin.H).max()) <= 1e-15 * float(np.abs(lin.H).max())
    for b in (fr.rhs(n), None):
        x, xd = R.x(b), R.x_dense(b)
        b64 = np.asarray(R.g_ld if b is None else b, np.float64)
        x64 = np.linalg.solve(np.asarray(R.H_ld, np.float64), b64)
        scale = float(np.abs(xd).max())
        e_ld, e_64 = float(np.abs(x - xd).max()) / scale, float(np.abs(x64 - xd).max()) / scale
        print("%s: identity vs dense in long double %.3e (bound cond x 2^-60 = %.3e), np.linalg.solve in double %.3e (bound cond x 2^-50 = %.3e)"
              % (name, e_ld, R.cond * 2.0 ** -60, e_64, R.cond * 2.0 ** -50))
        # both long-double solves are refined to the long-double residual: they differ by rounding of 2^-64 amplified by
        # cond (measured: at most 1.2e-14 relative at cond 8.4e6); the double solve by 2^-53 x cond
        assert e_ld <= R.cond * 2.0 ** -60 and e_64 <= R.cond * 2.0 ** -50
        res = float(np.abs(R.H_ld @ x - pg._ld(b64)).max()) / float(np.abs(b64).max())
        assert res <= R.cond * 2.0 ** -60


def test_the_plan_restatement():
    g = fr.hook_cases()["block_boundary44"][0]
    d = fr.distances(g)
    assert d[-1] == 0 and list(d[-4:-1]) == [27, 34, 25]            # (30, 20): fixed endpoint; free indices shift past node 20
    assert fr.choose(g) == 2 and fr.anchored(g, 2)
    two = fr.two_chains()
    assert not fr.anchored(two, 1) and fr.anchored(two, 22) and fr.choose(two) is None
    for name, (h, k, bw) in fr.lm_cases().items():
        assert fr.choose(h) == (bw - 5) // 6 and int(fr.far_mask(h, (bw - 5) // 6).sum()) == k, name
