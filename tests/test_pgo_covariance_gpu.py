"""vsl_pgo_covariance: the 6 x 6 diagonal blocks of H^-1 of a pose graph, on its three routes (0 dense, 1 linear band,
2 folded ring), against the long-double reference: H from tests/pgo_ref.py (linearize), inverted in long double
(tests/selinv_ref.py), the blocks cut out.  Tolerance, the project's covariance rule: max |cov - ref| <=
64 cond(H) 2^-52 max |H^-1|.  Every case asserts the route it took and prints its error beside the bound (-s)."""
import numpy as np
import pytest

import pgo_ref as pg
import selinv_ref as sel
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]


def _ring(n_nodes, **kw):
    """Node 0 fixed, a pendant of node 1; nodes 1 .. n - 1 free and closed into a ring by the edge (n - 1, 1): the fixed
    node does not cut the ring (the solver measures distances in free indices)."""
    return pg.loop_graph(n_nodes, window=1, loop=False, fixed=[0], extra=[(n_nodes - 1, 1)], noise=2e-3, **kw)


# name -> (graph builder, use_huber, huber, expected route)
GRAPHS = {
    "dense4": (lambda: pg.loop_graph(4, fixed=[0], noise=2e-3, seed=21), True, 1.0, 0),
    "chain23_first_band_size": (lambda: pg.loop_graph(23, window=1, loop=False, fixed=[0], noise=2e-3, seed=22), True, 1.0, 1),
    "chain30_w2_fixed_middle": (lambda: pg.loop_graph(30, window=2, loop=False, fixed=[15], noise=2e-3, seed=23), True, 1.0, 1),
    "ring25_even": (lambda: _ring(25, seed=24), True, 1.0, 2),
    "ring26_odd": (lambda: _ring(26, seed=25), True, 1.0, 2),
    "ring26_outliers_huber_on": (lambda: _ring(26, seed=26, outliers=5), True, 0.5, 2),
    "ring26_outliers_huber_off": (lambda: _ring(26, seed=26, outliers=5), False, 0.5, 2),
    "chain30_outliers_huber_on": (lambda: pg.loop_graph(30, window=2, loop=False, fixed=[15], noise=2e-3, seed=27, outliers=5),
                                  True, 0.5, 1),
    "chain30_outliers_huber_off": (lambda: pg.loop_graph(30, window=2, loop=False, fixed=[15], noise=2e-3, seed=27, outliers=5),
                                   False, 0.5, 1),
}
_cache = {}


def _case(name):
    """(graph, use_huber, huber, route, reference blocks [free nodes, 6, 6] long double, tolerance), computed once."""
    if name not in _cache:
        build, on, h, route = GRAPHS[name]
        g = build()
        H = pg.linearize(g, on, h).H
        Z = sel.inverse_ld(H)
        nf = g.n_unknowns() // 6
        blocks = np.stack([Z[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(nf)])
        blocks.setflags(write=False)
        _cache[name] = (g, on, h, route, blocks, sel.tolerance(H, Z))
    return _cache[name]


def _assert_blocks(name, cov, ref_blocks, tol, label=""):
    err = float(np.abs(cov - ref_blocks).max())
    print("%s%s: max |cov - ref| %.3e, bound %.3e" % (name, label, err, tol))
    assert np.all(np.isfinite(cov))
    assert err <= tol
    assert np.array_equal(cov, cov.transpose(0, 2, 1))


@pytest.mark.parametrize("name", list(GRAPHS))
def test_blocks_and_route(ctx, name):
    g, on, h, route, blocks, tol = _case(name)
    before = g.poses.copy()
    cov, storage = ctx.pgo_covariance(g, use_huber=on, huber=h)
    assert storage == route
    assert cov.shape == blocks.shape
    _assert_blocks(name, cov, blocks, tol)
    assert np.array_equal(g.poses, before)   # nothing is optimised
    if "outliers" in name:
        # the outliers really are beyond the Huber threshold: the two settings are different matrices
        other = _case(name.replace("_on", "_off") if on else name.replace("_off", "_on"))[4]
        assert float(np.abs(other - blocks).max()) > 10 * tol


def test_the_same_route_decision_as_the_solver(ctx):
    for name in GRAPHS:
        g, on, h, route, _, _ = _case(name)
        assert ctx.pgo_linearize_stored(g, on, h)[3]["storage"] == route, name


@pytest.mark.parametrize("name", ["ring25_even", "ring26_odd"])
def test_forced_dense_agrees(ctx, name):
    g, on, h, _, blocks, tol = _case(name)
    band, storage = ctx.pgo_covariance(g, use_huber=on, huber=h)
    assert storage == 2
    ctx.set_diagnostic("ba_force_dense", 1)
    try:
        cov, storage = ctx.pgo_covariance(g, use_huber=on, huber=h)
    finally:
        ctx.set_diagnostic("ba_force_dense", 0)
    assert storage == 0
    _assert_blocks(name, cov, blocks, tol, " forced dense")
    assert float(np.abs(cov - band).max()) <= 2 * tol


@pytest.mark.parametrize("name", ["dense4", "chain30_w2_fixed_middle", "ring26_odd"])
def test_subset_duplicate_permuted_and_empty_queries(ctx, name):
    g, on, h, route, _, _ = _case(name)
    free = np.flatnonzero(g.node_fixed == 0)
    full, _ = ctx.pgo_covariance(g, use_huber=on, huber=h)
    again, _ = ctx.pgo_covariance(g, use_huber=on, huber=h)
    assert np.array_equal(full, again)
    rng = np.random.default_rng(5)
    for query in (free[::3], free[::-1], np.array([free[-1], free[0], free[-1], free[0]]), rng.permutation(free)[:5], free[:1]):
        cov, storage = ctx.pgo_covariance(g, nodes=query, use_huber=on, huber=h)
        assert storage == route
        pos = np.searchsorted(free, query)
        assert np.array_equal(cov, full[pos])
    cov, storage = ctx.pgo_covariance(g, nodes=np.zeros(0, np.int32), use_huber=on, huber=h)
    assert cov.shape == (0, 6, 6) and storage == route


def test_invalid_ids_and_a_fixed_node(ctx, vsl):
    g = _case("ring25_even")[0]
    for bad in ([-1], [25], [3, 99], [0], [5, 0]):   # node 0 is fixed
        with pytest.raises(vsl.VslError) as e:
            ctx.pgo_covariance(g, nodes=np.array(bad, np.int32))
        assert e.value.code == -1, bad


@pytest.mark.parametrize("n_nodes,route", [(4, 0), (40, 2)])
def test_free_gauge_is_numeric_and_the_context_survives(ctx, vsl, n_nodes, route):
    g = pg.loop_graph(n_nodes, noise=2e-3, seed=31)   # no fixed node
    assert ctx.pgo_linearize_stored(g)[3]["storage"] == route
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_covariance(g)
    assert e.value.code == -7
    name = "ring25_even"
    g, on, h, _, blocks, tol = _case(name)
    _assert_blocks(name, ctx.pgo_covariance(g, use_huber=on, huber=h)[0], blocks, tol, " after the failure")


def test_a_free_node_without_an_edge_is_numeric(ctx, vsl):
    g = pg.loop_graph(30, window=2, loop=False, fixed=[15], isolated=[7], noise=2e-3, seed=32)
    with pytest.raises(vsl.VslError) as e:
        ctx.pgo_covariance(g)
    assert e.value.code == -7


def test_the_solver_is_not_disturbed(ctx):
    g = _case("ring26_odd")[0]
    a, b = g.copy(), g.copy()
    sa = ctx.pose_graph_optimize(a, max_iters=5)
    ctx.pgo_covariance(g)
    sb = ctx.pose_graph_optimize(b, max_iters=5)
    assert np.array_equal(a.poses, b.poses) and sa.final_cost == sb.final_cost and sa.iterations == sb.iterations
