"""vsl_pgo_joint_covariance: the 12 x 12 joint covariance [[S_aa, S_ab], [S_ba, S_bb]] of pairs of pose-graph nodes on
the three routes (0 dense, 1 linear band, 2 folded ring), against the long-double reference of tests/pgo_joint_ref.py (H
from pgo_ref.linearize, inverted by selinv_ref.inverse_ld).  Tolerance for every block, the project's covariance rule:
max |cov - ref| <= selinv_ref.tolerance(H, Z) = 64 cond(H) 2^-52 max |H^-1|.  Every case prints its error beside the
bound (-s).  The pairs of a graph (pgo_joint_ref.pairs_of) cover: read from the band, the largest in-band node distance
and the one after it, the two ends / opposite sides, free index 5 (unknowns 30..35 across the 32-column panel
boundary), the fixed node on either side, the last free node."""
import numpy as np
import pytest

import pgo_joint_ref as jr
import pgo_ref as pg
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]

BAND = ["chain23", "chain30_w2_fixed_middle", "ring25_even", "ring26_odd", "ring26_outliers_huber_on"]


def _query(ctx, c, pairs):
    return ctx.pgo_joint_covariance(c.g, pairs, use_huber=c.use_huber, huber=c.huber)


def _assert_blocks(c, cov, pairs, label=""):
    want = jr.joint_blocks(c, pairs)
    err = float(np.abs(cov - want).max())
    print("%s%s: %d pairs, max |cov - ref| %.3e, bound %.3e" % (c.name, label, len(pairs), err, c.tol))
    assert np.all(np.isfinite(cov))
    assert err <= c.tol
    assert np.array_equal(cov, cov.transpose(0, 2, 1))


@pytest.mark.parametrize("name", list(jr.GRAPHS))
def test_blocks_route_and_exact_properties(ctx, name):
    c = jr.case(name)
    pairs = jr.pairs_of(name)
    before = c.g.poses.copy()
    cov, storage = _query(ctx, c, pairs)
    assert storage == c.route == ctx.pgo_linearize_stored(c.g, c.use_huber, c.huber)[3]["storage"]
    assert cov.shape == (len(pairs), 12, 12)
    _assert_blocks(c, cov, pairs)
    assert np.array_equal(c.g.poses, before)   # nothing is optimised
    # a fixed node: rows and columns exactly zero
    for q, (a, b) in enumerate(pairs):
        if c.g.node_fixed[a]:
            assert not cov[q, :6, :].any() and not cov[q, :, :6].any()
        if c.g.node_fixed[b]:
            assert not cov[q, 6:, :].any() and not cov[q, :, 6:].any()
    # (b, a): the same bits, blocks swapped and transposed
    swapped, _ = _query(ctx, c, [(b, a) for a, b in pairs])
    perm = np.r_[6:12, 0:6]
    assert np.array_equal(swapped, cov[:, perm][:, :, perm])
    # diagonal blocks: the bits of vsl_pgo_covariance on this route
    free = np.flatnonzero(c.g.node_fixed == 0)
    marg, st2 = ctx.pgo_covariance(c.g, use_huber=c.use_huber, huber=c.huber)
    assert st2 == storage
    for q, (a, b) in enumerate(pairs):
        if not c.g.node_fixed[a]:
            assert np.array_equal(cov[q, :6, :6], marg[np.searchsorted(free, a)]), (a, b)
        if not c.g.node_fixed[b]:
            assert np.array_equal(cov[q, 6:, 6:], marg[np.searchsorted(free, b)]), (a, b)
    # two calls, subsets, duplicates, permutations: the bits of the full query
    assert np.array_equal(_query(ctx, c, pairs)[0], cov)
    rng = np.random.default_rng(7)
    n = len(pairs)
    for sel in (np.arange(0, n, 2), np.arange(n)[::-1], np.array([n - 1, 0, n - 1, 1, 1]), rng.permutation(n)[:3], np.array([1])):
        sub, st3 = _query(ctx, c, [pairs[i] for i in sel])
        assert st3 == storage and np.array_equal(sub, cov[sel]), sel
    for q in range(n):   # every pair alone
        assert np.array_equal(_query(ctx, c, [pairs[q]])[0][0], cov[q]), pairs[q]


@pytest.mark.parametrize("name", BAND)
def test_in_band_pairs_agree_with_the_solve(ctx, name):
    c = jr.case(name)
    pairs = jr.pairs_of(name)
    cov, storage = _query(ctx, c, pairs)
    ctx.set_diagnostic("pgo_cov_no_band_read", 1)
    try:
        solved, st2 = _query(ctx, c, pairs)
    finally:
        ctx.set_diagnostic("pgo_cov_no_band_read", 0)
    assert st2 == storage == c.route
    _assert_blocks(c, solved, pairs, " all pairs solved")
    differ = int((np.abs(solved - cov).max(axis=(1, 2)) > 0).sum())
    print("%s: %d of %d pairs change bits under the diagnostic (the in-band ones may)" % (name, differ, len(pairs)))
    assert float(np.abs(solved - cov).max()) <= 2 * c.tol


@pytest.mark.parametrize("name", BAND)
def test_forced_dense_agrees(ctx, name):
    c = jr.case(name)
    pairs = jr.pairs_of(name)
    cov, storage = _query(ctx, c, pairs)
    assert storage == c.route
    ctx.set_diagnostic("ba_force_dense", 1)
    try:
        dense, st2 = _query(ctx, c, pairs)
        marg, _ = ctx.pgo_covariance(c.g, use_huber=c.use_huber, huber=c.huber)
    finally:
        ctx.set_diagnostic("ba_force_dense", 0)
    assert st2 == 0
    _assert_blocks(c, dense, pairs, " forced dense")
    assert float(np.abs(dense - cov).max()) <= 2 * c.tol
    free = np.flatnonzero(c.g.node_fixed == 0)
    for q, (a, b) in enumerate(pairs):   # the dense route's diagonal rule, bit for bit
        if not c.g.node_fixed[a]:
            assert np.array_equal(dense[q, :6, :6], marg[np.searchsorted(free, a)])


def test_invalid_pairs(ctx, vsl):
    c = jr.case("ring25_even")
    for bad in ([(3, 3)], [(-1, 2)], [(2, 25)], [(1, 2), (4, 99)], [(0, 0)]):
        with pytest.raises(vsl.VslError) as e:
            ctx.pgo_joint_covariance(c.g, bad)
        assert e.value.code == -1, bad
    g = pg.loop_graph(30, window=2, loop=False, fixed=[15, 16], noise=2e-3, seed=23)
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_joint_covariance(g, [(15, 16)])
    assert e.value.code == -1


def test_no_pairs_returns_the_route(ctx):
    for name in ("dense4", "chain30_w2_fixed_middle", "ring26_odd"):
        c = jr.case(name)
        cov, storage = _query(ctx, c, np.zeros((0, 2), np.int32))
        assert cov.shape == (0, 12, 12) and storage == c.route


@pytest.mark.parametrize("n_nodes,route", [(4, 0), (40, 2)])
def test_free_gauge_is_numeric_and_the_context_survives(ctx, vsl, n_nodes, route):
    g = pg.loop_graph(n_nodes, noise=2e-3, seed=31)   # no fixed node
    assert ctx.pgo_linearize_stored(g)[3]["storage"] == route
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_joint_covariance(g, [(0, n_nodes // 2), (1, 2)])
    assert e.value.code == -7
    c = jr.case("ring25_even")
    pairs = jr.pairs_of("ring25_even")
    _assert_blocks(c, _query(ctx, c, pairs)[0], pairs, " after the failure")


def test_a_free_node_without_an_edge_is_numeric(ctx, vsl):
    g = pg.loop_graph(30, window=2, loop=False, fixed=[15], isolated=[7], noise=2e-3, seed=32)
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_joint_covariance(g, [(0, 29), (3, 4)])
    assert e.value.code == -7
    c = jr.case("chain30_w2_fixed_middle")
    pairs = jr.pairs_of(c.name)
    _assert_blocks(c, _query(ctx, c, pairs)[0], pairs, " after the failure")


def test_the_solver_is_not_disturbed(ctx):
    c = jr.case("ring26_odd")
    a, b = c.g.copy(), c.g.copy()
    sa = ctx.pose_graph_optimize(a, max_iters=5)
    _query(ctx, c, jr.pairs_of("ring26_odd"))
    sb = ctx.pose_graph_optimize(b, max_iters=5)
    assert np.array_equal(a.poses, b.poses) and sa.final_cost == sb.final_cost and sa.iterations == sb.iterations
    before, _ = ctx.pgo_covariance(c.g, use_huber=c.use_huber, huber=c.huber)
    _query(ctx, c, jr.pairs_of("ring26_odd"))
    after, _ = ctx.pgo_covariance(c.g, use_huber=c.use_huber, huber=c.huber)
    assert np.array_equal(before, after)
