"""GPU: pose-graph kernels (visual-slam_amd/csrc/pgo.hip) against the long-double reference tests/pgo_ref.py at the edges
the synthetic loop of test_pgo_gpu.py never reaches: both sides of every branch of the SE3 log, the Huber threshold, the
band and cyclic-band builders as the solver stores them (vsl_pgo_linearize_stored), fixed nodes anywhere, and the
Levenberg-Marquardt exits.  Tolerance: pgo_ref.GPU_TOL = min(8 x the oracle-versus-reference discrepancy measured on the
CPU by test_pgo_ref_cpu.py, 1e-9), relative to max|H| of the block or matrix, to max|g| likewise
(pgo_ref.rel_errors), and to the cost (pgo_ref.cost_error)."""
import functools

import numpy as np
import pytest

import pgo_ref as ref

pytestmark = pytest.mark.gpu

TOL = ref.GPU_TOL
CHUNK = 70          # edges per graph: a full 64-thread linearise block and a partial second one; 480 unknowns


def _arr(orc, g):
    return orc.PgoArrays(g.poses, g.node_fixed, g.edge_a, g.edge_b, g.edge_meas)


@functools.lru_cache(maxsize=None)
def _case(name, jacobi=0):
    """(graph, blocks, reference linearisation) of one of pgo_ref.linearize_cases()."""
    g, use_huber, h, blocks = ref.linearize_cases()[name]
    return g, blocks, ref.linearize(g, use_huber, h, jacobi_scale=bool(jacobi))


@functools.lru_cache(maxsize=None)
def _topologies():
    return ref.topologies()


def _check_blocks(H, grad, cost, R, blocks, what):
    inside = np.zeros(H.shape, bool)
    worst = 0.0
    for e, (form, at, size) in enumerate(blocks):
        s = slice(at, at + size)
        eh, eg = ref.rel_errors(H[s, s], grad[s], R.H[s, s], R.g[s])
        worst = max(worst, eh, eg)
        assert eh <= TOL and eg <= TOL, (what, e, form, eh, eg)
        inside[s, s] = True
    assert not H[~inside].any(), what
    assert ref.cost_error(cost, R.cost) <= TOL, (what, cost, R.cost)
    return worst


# ------------------------------------------------------------------------------------------------ (a) edge geometry
@pytest.mark.parametrize("offset", range(len(ref.FORMS)))
def test_edge_geometry_table_matches_the_reference(ctx, offset):
    # 320 edges (10 angles x 4 axes x both signs of the relative w x 4 translation norms) in graphs of 70 disjoint
    # two-node components; the offset moves the forms (a fixed / b fixed / both free) along the table, so that over the
    # seven cases every edge is linearised in every form
    names = [n for n in ref.linearize_cases() if n.startswith("table/%d/" % offset)]
    assert len(names) == 5 and CHUNK > 64
    worst = 0.0
    for chunk, name in enumerate(names):
        g, blocks, R = _case(name)
        assert g.n_unknowns() == 480 and len(g.edge_a) == CHUNK
        H, grad, cost = ctx.pgo_linearize(g, True, 1.0)
        worst = max(worst, _check_blocks(H, grad, cost, R, blocks, "chunk %d offset %d" % (chunk, offset)))
    print("edge table, offset %d: worst relative error %.3g (tolerance %.3g)" % (offset, worst, TOL))


# ------------------------------------------------------------------------------------------------------- (b) Huber
@pytest.mark.parametrize("use_huber", [True, False])
@pytest.mark.parametrize("h", [1e-3, 0.5])
def test_huber_threshold_edges_match_the_reference(ctx, h, use_huber):
    # |r| = 0 exactly, 0.999 h, 1.001 h, 10 h, 1e3 h (four edges each)
    g, blocks, R = _case("huber/%g/%s" % (h, "on" if use_huber else "off"))
    H, grad, cost = ctx.pgo_linearize(g, use_huber, h)
    worst = _check_blocks(H, grad, cost, R, blocks, "huber %g %s" % (h, use_huber))
    for e in range(4):                      # r == 0: no gradient at all, in either arithmetic
        _, at, size = blocks[e]
        assert not grad[at:at + size].any() and not R.g[at:at + size].any()
    if use_huber:                           # the corrector is active on exactly the edges beyond the threshold
        _, _, Roff = _case("huber/%g/off" % h)
        for e, (_, at, size) in enumerate(blocks):
            same = np.array_equal(R.H[at:at + size, at:at + size], Roff.H[at:at + size, at:at + size])
            assert same == (ref.HUBER_FACTORS[e // 4] < 1.0), e
    print("huber %g %s: worst relative error %.3g (tolerance %.3g)" % (h, use_huber, worst, TOL))


# ----------------------------------------------------------------------------------------------- (c) storage forms
@pytest.mark.parametrize("jacobi", [0, 1])
@pytest.mark.parametrize("name", ["ring22_all_free", "ring22_21_free", "ring44_w2_fixed_middle", "ring44_w2_fixed_first",
                                  "ring44_w2_fixed_pair", "chain60_w3", "ring44_w2_long_edge", "ring48_mixed"])
def test_stored_normal_equations(ctx, name, jacobi):
    g, storage, bw, n = _topologies()[name]
    H, grad, cost, info = ctx.pgo_linearize_stored(g, True, 1.0, jacobi)
    assert (info["storage"], info["half_bandwidth"], 6 * info["n_free"]) == (storage, bw, n), info
    assert info["stray_nonzeros"] == 0
    ctx.set_diagnostic("ba_force_dense", 1)
    try:
        Hd, gd, costd, infod = ctx.pgo_linearize_stored(g, True, 1.0, jacobi)
    finally:
        ctx.set_diagnostic("ba_force_dense", 0)
    assert infod["storage"] == 0 and infod["half_bandwidth"] == 0 and infod["stray_nonzeros"] == 0
    # the same thread code accumulates the same products in the same incidence order in every storage form
    assert np.array_equal(H, Hd) and np.array_equal(grad, gd) and cost == costd
    assert np.array_equal(H, H.T)
    if not jacobi:                            # unit scale: what vsl_pgo_linearize returns
        H0, g0, c0 = ctx.pgo_linearize(g, True, 1.0)
        assert np.array_equal(H, H0) and np.array_equal(grad, g0) and cost == c0
    gc, _, R = _case("topology/" + name, jacobi)
    assert gc is g or np.array_equal(gc.poses, g.poses)
    eh, eg = ref.rel_errors(H, grad, R.H, R.g)
    print("%s jacobi %d: storage %d bw %d, H %.3g g %.3g (tolerance %.3g)" % (name, jacobi, storage, bw, eh, eg, TOL))
    assert eh <= TOL and eg <= TOL
    assert ref.cost_error(cost, R.cost) <= TOL
    # structure: nothing outside the band (cyclic: and its corner) in the band forms
    if storage:
        i, j = np.indices(H.shape)
        d = np.abs(i - j)
        outside = (np.minimum(d, n - d) if storage == 2 else d) > bw
        assert not H[outside].any()
        assert H[np.minimum(d, n - d) == bw].any() if storage == 2 else H[d == bw].any()     # the band's last diagonal is used
    if name == "ring48_mixed":                # node 7 is free (index 7: the fixed nodes come later) and has no edge
        assert not H[42:48].any() and not H[:, 42:48].any() and not grad[42:48].any()
    if name == "ring22_all_free":             # the wrap-around corner comes from the loop edge (21, 0) itself
        assert H[126:, :6].any() and np.array_equal(H[126:, :6], H[:6, 126:].T)


# -------------------------------------------------------------------------------------------------- (d) full solves
@pytest.mark.parametrize("name", ["ring44_w2_fixed_middle", "chain60_w3", "ring44_w2_long_edge"])
def test_full_solves_on_the_storage_forms(ctx, orc, name):
    g, storage, bw, _ = _topologies()[name]          # measurement noise 2e-3, one fixed node in the middle
    assert g.node_fixed.sum() >= 1
    assert ctx.pgo_linearize_stored(g, True, 1.0, 1)[3]["storage"] == storage
    a, b, c = _arr(orc, g), _arr(orc, g), _arr(orc, g)
    s = ctx.pose_graph_optimize(a, True, 1.0, 20)
    os_ = orc.pose_graph_optimize(b, True, 1.0, 20)
    assert (s.iterations, s.termination, s.successful_steps) == (os_.iterations, os_.termination, os_.successful_steps)
    assert np.abs(a.poses - b.poses).max() < 1e-7
    ctx.set_diagnostic("ba_force_dense", 1)
    try:
        sd = ctx.pose_graph_optimize(c, True, 1.0, 20)
    finally:
        ctx.set_diagnostic("ba_force_dense", 0)
    assert (sd.iterations, sd.termination, sd.successful_steps) == (s.iterations, s.termination, s.successful_steps)
    assert np.abs(a.poses - c.poses).max() < 1e-8
    # independent of both: the reference's cost at the input and at the returned poses
    c0, c1 = ref.total_cost(g, True, 1.0), ref.total_cost(g, True, 1.0, poses=a.poses)
    print("%s: %d iterations, cost %.6e -> %.6e, reference %.6e -> %.6e" % (name, s.iterations, s.initial_cost, s.final_cost, c0, c1))
    assert abs(s.initial_cost - c0) <= 1e-12 * c0 and abs(s.final_cost - c1) <= 1e-12 * c1
    assert s.final_cost < s.initial_cost
    fixed = g.node_fixed != 0
    assert np.array_equal(a.poses[fixed], g.poses[fixed]) and np.array_equal(c.poses[fixed], g.poses[fixed])


# ------------------------------------------------------------------------------------------------------ (e) LM paths
def _parity(ctx, orc, g, use_huber=True, huber=1.0, max_iters=20):
    a, b = _arr(orc, g), _arr(orc, g)
    s = ctx.pose_graph_optimize(a, use_huber, huber, max_iters)
    os_ = orc.pose_graph_optimize(b, use_huber, huber, max_iters)
    assert (s.iterations, s.termination, s.successful_steps) == (os_.iterations, os_.termination, os_.successful_steps)
    assert a.poses.shape == b.poses.shape and (a.poses.size == 0 or np.abs(a.poses - b.poses).max() < 1e-7)
    # (1e-24: a start at the optimum costs ~1e-30, which is the squared rounding of the poses and nothing else)
    assert abs(s.initial_cost - os_.initial_cost) <= 1e-9 * os_.initial_cost + 1e-24
    assert abs(s.final_cost - os_.final_cost) <= 1e-6 * max(os_.final_cost, 1e-12) + 1e-15
    return s, a


def test_start_at_the_optimum_takes_the_gradient_exit(ctx, orc):
    g = ref.ground_truth_graph(44, 2, [20])          # cyclic band form: the exit is found one step late and dropped
    assert ctx.pgo_linearize_stored(g, True, 1.0, 1)[3]["storage"] == 2
    s, a = _parity(ctx, orc, g)
    assert (s.iterations, s.termination, s.successful_steps) == (0, 2, 0)
    assert np.array_equal(a.poses, g.poses)
    g = ref.ground_truth_graph(20, 1, [3])            # and in the dense form
    s, a = _parity(ctx, orc, g)
    assert (s.iterations, s.termination, s.successful_steps) == (0, 2, 0) and np.array_equal(a.poses, g.poses)


@pytest.mark.parametrize("max_iters", [0, 1])
def test_iteration_limits(ctx, orc, max_iters):
    g = _topologies()["ring44_w2_fixed_middle"][0]
    s, a = _parity(ctx, orc, g, max_iters=max_iters)
    assert (s.iterations, s.termination) == (max_iters, 0)
    if max_iters == 0:
        assert np.array_equal(a.poses, g.poses) and s.final_cost == s.initial_cost
    else:
        assert s.successful_steps == 1 and s.final_cost < s.initial_cost


def test_rejected_step(ctx, orc):
    # drift 0.5 and four gross outliers (seed picked on the CPU): the oracle rejects a step on the way
    g = ref.loop_graph(30, window=2, fixed=[12], noise=2e-3, drift=0.5, seed=10, outliers=4)
    assert ctx.pgo_linearize_stored(g, True, 1.0, 1)[3]["storage"] == 2
    os_ = orc.pose_graph_optimize(_arr(orc, g), True, 1.0, 30)
    assert os_.termination == 1 and os_.successful_steps < os_.iterations - 1     # (the last, converged step is not counted)
    s, _ = _parity(ctx, orc, g, max_iters=30)
    assert s.successful_steps < s.iterations - 1


@pytest.mark.parametrize("n_nodes", [44, 22])          # cyclic band (258 unknowns) and dense (126)
def test_huber_off_in_a_full_solve(ctx, orc, n_nodes):
    g = ref.loop_graph(n_nodes, window=2, fixed=[9], noise=2e-3, seed=21, outliers=2)
    s, a = _parity(ctx, orc, g, use_huber=False)
    assert s.final_cost < s.initial_cost
    c1 = ref.total_cost(g, False, 1.0, poses=a.poses)
    assert abs(s.final_cost - c1) <= 1e-12 * c1


def test_free_nodes_without_edges(ctx, orc):
    g = ref.Graph(ref.loop_graph(5).poses, [0, 0, 1, 0, 0], [], [], np.zeros((0, 6)))
    H, grad, cost, info = ctx.pgo_linearize_stored(g, True, 1.0, 1)
    assert H.shape == (24, 24) and not H.any() and not grad.any() and cost == 0.0 and info["storage"] == 0
    s, a = _parity(ctx, orc, g)
    assert (s.iterations, s.termination, s.successful_steps) == (0, 2, 0)
    assert np.array_equal(a.poses, g.poses) and s.initial_cost == 0.0 and s.final_cost == 0.0


def test_empty_graph(ctx, orc):
    g = ref.Graph(np.zeros((0, 7)), [], [], [], np.zeros((0, 6)))
    H, grad, cost, info = ctx.pgo_linearize_stored(g, True, 1.0, 0)
    assert H.size == 0 and grad.size == 0 and cost == 0.0 and info["n_free"] == 0 and info["storage"] == 0
    s, _ = _parity(ctx, orc, g)
    assert (s.iterations, s.termination, s.successful_steps) == (0, 2, 0)
