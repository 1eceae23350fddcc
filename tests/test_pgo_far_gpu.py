"""Pose graph, far-edge route (pgo.hip "FAR EDGES": band factor of the near edges plus a low-rank update for the far
ones) against the long-double restatement of tests/pgo_far_ref.py, the dense device route and the
oracle.
  hook      vsl_pgo_far_solve on the smallest shapes at each boundary: |x - x_ref| <= 64 cond_2(H) 2^-52 max|x_ref|; the
            same bits twice, b -> -b gives -x, b = NULL is b = g of vsl_pgo_linearize_w -- bit for bit
  errors    129 far edges, no admissible split, no fixed node
  LM        switch on: the route is taken, the trajectory is the dense route's and the oracle's; switch on where the
            route does not apply: the bits of the switch-off call
Every measured figure is printed beside its bound (-s)."""
import ctypes as C

import numpy as np
import pytest

import pgo_far_ref as fr
import pgo_ref as pg
import pgo_weighted_ref as wr
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]

f64p = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------------------ 1-4. the hook
@pytest.mark.parametrize("name", ["k1_chain23", "block_boundary44", "weighted60", "k0_chain30"])
def test_hook_matches_the_reference(ctx, name):
    g, W, hub, thr, d_star, k_want = fr.hook_cases()[name]
    R = fr.hook_reference(name)
    n = g.n_unknowns()
    if name == "k1_chain23":
        assert n == 132 and n % 32 != 0
    if name == "weighted60":
        assert (R.lin.norms[R.far] > thr).any() and (R.lin.norms[R.far] < thr).any()
    b = fr.rhs(n)
    x, k, bw = ctx.pgo_far_solve(g, b, d_star, hub, thr, edge_info=W)
    assert (k, bw) == (k_want, 6 * d_star + 5) and k == R.k
    x_ref = R.x(b)
    err, tol = float(np.abs(x - x_ref).max()), R.tol(x_ref)
    e_id = float(np.abs(x_ref - R.x_dense(b)).max())
    print("%s: n %d, k %d, bw %d, cond %.3e: |x - x_ref| %.3e, bar %.3e (max|x| %.3e; identity vs dense solve in long double %.3e)"
          % (name, n, k, bw, R.cond, err, tol, float(np.abs(x_ref).max()), e_id))
    assert err <= tol
    # bit for bit: twice, the sign, and b = NULL
    x2, _, _ = ctx.pgo_far_solve(g, b, d_star, hub, thr, edge_info=W)
    assert np.array_equal(x, x2)
    xm, _, _ = ctx.pgo_far_solve(g, -b, d_star, hub, thr, edge_info=W)
    assert np.array_equal(xm, -x)
    _, grad, _ = ctx.pgo_linearize(g, hub, thr, edge_info=W)
    xg, _, _ = ctx.pgo_far_solve(g, grad, d_star, hub, thr, edge_info=W)
    xn, _, _ = ctx.pgo_far_solve(g, None, d_star, hub, thr, edge_info=W)
    assert np.array_equal(xg, xn) and xn.any()
    xg_ref = R.x(grad)
    eg = float(np.abs(xn - xg_ref).max())
    print("  b = g: |x - x_ref| %.3e, bar %.3e" % (eg, R.tol(xg_ref)))
    assert eg <= R.tol(xg_ref)


def test_hook_takes_the_plans_choice(ctx):
    g, W, hub, thr, d_star, k_want = fr.hook_cases()["block_boundary44"]
    assert fr.choose(g) == d_star
    b = fr.rhs(g.n_unknowns())
    x, k, bw = ctx.pgo_far_solve(g, b, -1, hub, thr)
    x2, _, _ = ctx.pgo_far_solve(g, b, d_star, hub, thr)
    assert (k, bw) == (k_want, 6 * d_star + 5) and np.array_equal(x, x2)


# ------------------------------------------------------------------------------------------------ 5. errors
def _raw_far_solve(ctx, g, max_near):
    st, o = ctx._pgo_struct(g), ctx._ba_opts(True, 1.0, 0, 0)
    x = np.full(max(g.n_unknowns(), 1), 7.0)
    rc = ctx.L.vsl_pgo_far_solve(ctx.h, C.byref(st), None, C.byref(o), None, C.c_int(max_near), x.ctypes.data_as(f64p), None, None)
    return rc, x


def test_errors(ctx, vsl):
    extra = [(40 + (i % 30), 1 + i % 9) for i in range(129)]
    g = pg.loop_graph(80, window=1, loop=False, fixed=[0], extra=extra, noise=fr.NOISE, seed=48)
    assert int(fr.far_mask(g, 1).sum()) == 129
    rc, _ = _raw_far_solve(ctx, g, 1)
    assert rc == -1                                      # VSL_ERR_INVALID: 129 far edges
    rc, _ = _raw_far_solve(ctx, g, 79)
    assert rc == -1                                      # the band is not narrower than the matrix
    two = fr.two_chains()
    assert fr.choose(two) is None
    rc, _ = _raw_far_solve(ctx, two, -1)
    assert rc == -1
    # no fixed node: M is singular
    free = pg.loop_graph(30, window=2, loop=False, fixed=[], extra=[(25, 4)], noise=fr.NOISE, seed=49)
    rc, x = _raw_far_solve(ctx, free, 2)
    print("no fixed node: rc %d, max|x| %.3e" % (rc, float(np.abs(x).max())))
    assert rc == -7 and not x[:free.n_unknowns()].any()  # VSL_ERR_NUMERIC, x = 0
    good, _, _, _, _, _ = fr.hook_cases()["k1_chain23"]
    a, b = good.copy(), good.copy()
    s = ctx.pose_graph_optimize(a, True, 1.0, 20)
    fresh = vsl.Context(0)
    try:
        s2 = fresh.pose_graph_optimize(b, True, 1.0, 20)
    finally:
        fresh.close()
    assert np.array_equal(a.poses, b.poses) and (s.iterations, s.final_cost) == (s2.iterations, s2.final_cost) and s.iterations > 0


# ------------------------------------------------------------------------------------------------ 6-8. the LM loop
def _solve(ctx, g, far, W=None, hub=True, thr=1.0):
    ctx.set_diagnostic("pgo_far_edges", int(far))
    try:
        return ctx.pose_graph_optimize(g, hub, thr, 20, edge_info=W), ctx.last_pgo_far()
    finally:
        ctx.set_diagnostic("pgo_far_edges", 0)


def _counts(s):
    return (s.iterations, s.termination, s.successful_steps)


@pytest.mark.parametrize("name", list(fr.lm_cases()))
def test_lm_route_taken(ctx, orc, name):
    g0, k_want, bw_want = fr.lm_cases()[name]
    assert ctx.pgo_linearize_stored(g0)[3]["storage"] == 0 and g0.n_unknowns() > 128
    assert fr.choose(g0) == (bw_want - 5) // 6
    a, b, c, a2 = g0.copy(), g0.copy(), g0.copy(), g0.copy()
    s, info = _solve(ctx, a, True)
    assert info["taken"] == 1 and (info["far_edges"], info["half_bandwidth"]) == (k_want, bw_want)
    assert info["columns"] == 6 * k_want + 1 and info["solves"] == s.iterations
    sd, info_d = _solve(ctx, b, False)
    assert info_d == dict(taken=0, far_edges=0, half_bandwidth=0, columns=0, solves=0)
    oc = orc.PgoArrays(c.poses, c.node_fixed, c.edge_a, c.edge_b, c.edge_meas)
    so = orc.pose_graph_optimize(oc, True, 1.0, 20)
    e_dense, e_orc = float(np.abs(a.poses - b.poses).max()), float(np.abs(a.poses - oc.poses).max())
    print("%s: counts far %s dense %s oracle %s; poses %.3e from the dense route (bound 1e-8), %.3e from the oracle (bound 1e-7); "
          "final cost %.12e dense %.12e oracle %.12e" % (name, _counts(s), _counts(sd), _counts(so), e_dense, e_orc, s.final_cost,
                                                         sd.final_cost, so.final_cost))
    assert _counts(sd) == _counts(so)
    assert _counts(s) == _counts(sd) and s.iterations > 1 and s.successful_steps > 0
    assert e_dense < 1e-8 and e_orc < 1e-7
    for other in (sd, so):
        assert abs(s.initial_cost - other.initial_cost) <= 1e-9 * max(1.0, other.initial_cost)
        assert abs(s.final_cost - other.final_cost) <= 1e-6 * max(other.final_cost, 1e-12) + 1e-15
    assert s.final_cost < s.initial_cost
    fixed = np.flatnonzero(g0.node_fixed)
    assert np.array_equal(a.poses[fixed], g0.poses[fixed])
    # 8. the same bits twice
    s2, _ = _solve(ctx, a2, True)
    assert np.array_equal(a.poses, a2.poses) and (_counts(s2), s2.final_cost) == (_counts(s), s.final_cost)


def test_lm_route_taken_weighted_and_robustified(ctx):
    g0 = fr.lm_cases()["chain150_w3_far4"][0]
    W = wr.family("random", len(g0.edge_a), seed=6)
    thr = wr.huber_threshold(wr.linearize(g0, W, False, 1.0).norms)
    a, b = g0.copy(), g0.copy()
    s, info = _solve(ctx, a, True, W, True, thr)
    sd, _ = _solve(ctx, b, False, W, True, thr)
    e = float(np.abs(a.poses - b.poses).max())
    print("weighted, Huber %.3g: counts far %s dense %s, poses %.3e apart (bound 1e-8), final cost %.12e / %.12e"
          % (thr, _counts(s), _counts(sd), e, s.final_cost, sd.final_cost))
    assert info["taken"] == 1 and info["far_edges"] == 4
    assert _counts(s) == _counts(sd) and e < 1e-8
    assert abs(s.initial_cost - sd.initial_cost) <= 1e-9 * max(1.0, sd.initial_cost)
    assert abs(s.final_cost - sd.final_cost) <= 1e-6 * max(sd.final_cost, 1e-12) + 1e-15


def test_lm_route_not_taken(ctx, vsl):
    T = pg.topologies()
    graphs = {"ring (cyclic band)": (T["ring44_w2_fixed_middle"][0], 2), "chain (linear band)": (T["chain60_w3"][0], 1),
              "21 free nodes": (T["ring22_21_free"][0], 0), "two chains": (fr.two_chains(), 0)}
    fresh = vsl.Context(0)
    try:
        for label, (g0, storage) in graphs.items():
            assert ctx.pgo_linearize_stored(g0)[3]["storage"] == storage, label
            a, b = g0.copy(), g0.copy()
            s, info = _solve(ctx, a, True)
            s2 = fresh.pose_graph_optimize(b, True, 1.0, 20)
            assert info == dict(taken=0, far_edges=0, half_bandwidth=0, columns=0, solves=0), label
            assert np.array_equal(a.poses, b.poses), label
            assert (_counts(s), s.initial_cost, s.final_cost) == (_counts(s2), s2.initial_cost, s2.final_cost), label
            assert s.iterations > 0
    finally:
        fresh.close()
