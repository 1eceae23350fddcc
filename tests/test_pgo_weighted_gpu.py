"""Pose graph with per-edge information matrices (the _w entry points of pgo.hip, edge_info= in Python) against the
long-double reference of tests/pgo_weighted_ref.py.  Graphs: the shapes tests/test_pgo_gpu.py uses, one per storage
(dense 30 nodes with long-range edges, 120 nodes window 3, 300 nodes window 12) plus a 120-node window-3 chain for the
linear band (every storage is asserted), and chains of
0 / 1 / 64 / 65 edges (the workgroup boundary of the per-edge kernels).  Weight families: identity, 4 I,
diag(1e2 x 3, 1e4 x 3), random SPD with condition number up to 1e6.
  linearisation   H, g relative to their max, cost relative: GPU_TOL_W = 8 x F64_VS_REF_W (pgo_weighted_ref.py)
  4 I             H, g, cost are 4 x the unweighted ones bit for bit (Huber off)
  NULL            the _w symbols with a null edge_info return the bits of the unweighted symbols
  solve           cost <= reference minimum x (1 + LM_FUNCTION_TOLERANCE x iterations), poses to 1e-7 of the reference
                  minimiser (the parameter tolerance of tests/test_pgo_gpu.py), same bits twice, dense route to 1e-7; the
                  reference run converges by the solver's own stop rules (pgo_weighted_ref.minimize_lm)
  marginals       64 cond(H) 2^-52 max|Sigma| against the inverse of the reference H
  refusals        VSL_ERR_INVALID naming the lowest edge, poses untouched
Every measured figure is printed beside its bound (-s)."""
import ctypes as C

import numpy as np
import pytest

import pgo_joint_ref as jr
import pgo_ref as pg
import pgo_weighted_ref as wr
import spd_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)]

LM_FUNCTION_TOLERANCE = 1e-6      # lm_policy.h
POSE_TOL = 1e-7                   # tests/test_pgo_gpu.py, poses against the oracle
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
ALL = list(wr.STORAGE_GRAPHS) + ["tiny%d" % k for k in wr.TINY_EDGE_COUNTS]


# ------------------------------------------------------------------------------------------------ 1. linearisation
@pytest.mark.parametrize("huber", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_linearisation_matches_the_reference(ctx, synth, name, huber):
    expected_storage = wr.graphs(synth)[name][1]
    for fam in wr.FAMILIES:
        g, W, thr, want = wr.cases(synth)[(name, fam, huber)]
        H, grad, cost = ctx.pgo_linearize(g, huber, thr, edge_info=W)
        eh, eg = pg.rel_errors(H, grad, want.H, want.g)
        ec = pg.cost_error(cost, want.cost)
        Hs, gs, cs, info = ctx.pgo_linearize_stored(g, huber, thr, edge_info=W)
        esh, esg = pg.rel_errors(Hs, gs, want.H, want.g)
        print("%s %s huber %d: H %.3e g %.3e cost %.3e | stored (%d) H %.3e g %.3e cost %.3e | bound %.3e"
              % (name, fam, huber, eh, eg, ec, info["storage"], esh, esg, pg.cost_error(cs, want.cost), wr.GPU_TOL_W))
        assert max(eh, eg, ec) <= wr.GPU_TOL_W, fam
        assert max(esh, esg, pg.cost_error(cs, want.cost)) <= wr.GPU_TOL_W, fam
        assert info["stray_nonzeros"] == 0
        if expected_storage is not None:
            assert info["storage"] == expected_storage
            if huber:
                assert (want.norms > thr).any() and (want.norms < thr).any()
                assert fam == "identity" or ((want.raw_norms < thr) & (want.norms > thr)).any()


# ------------------------------------------------------------------------------------------------ 2. exact scaling
@pytest.mark.parametrize("name", ALL)
def test_four_times_identity_scales_exactly(ctx, synth, name):
    g = wr.graphs(synth)[name][0]
    W = wr.family("four", len(g.edge_a))
    H, grad, cost = ctx.pgo_linearize(g, False, 1.0)
    Hw, gw, cw = ctx.pgo_linearize(g, False, 1.0, edge_info=W)
    assert np.array_equal(Hw, 4.0 * H) and np.array_equal(gw, 4.0 * grad) and cw == 4.0 * cost
    Hs, gs, cs, info = ctx.pgo_linearize_stored(g, False, 1.0)
    Hsw, gsw, csw, infow = ctx.pgo_linearize_stored(g, False, 1.0, edge_info=W)
    assert np.array_equal(Hsw, 4.0 * Hs) and np.array_equal(gsw, 4.0 * gs) and csw == 4.0 * cs and info == infow
    assert len(g.edge_a) == 0 or H.any()


# ------------------------------------------------------------------------------------------------ 3. no weights
def _opts(ctx, huber, iters):
    return ctx._ba_opts(True, huber, iters, 0)


@pytest.mark.parametrize("name", list(wr.STORAGE_GRAPHS) + ["tiny65"])
def test_null_edge_info_is_the_unweighted_call(ctx, synth, name):
    """The _w symbols through ctypes with a NULL pointer, beside the existing symbols (edge_info=None in Python)."""
    g0 = wr.graphs(synth)[name][0]
    L, h = ctx.L, ctx.h
    n = g0.n_unknowns()
    o = _opts(ctx, 0.5, 20)
    # solve
    a, b = g0.copy(), g0.copy()
    sa = ctx.pose_graph_optimize(a, True, 0.5, 20)
    st, sb = ctx._pgo_struct(b), type(sa)()
    assert L.vsl_pose_graph_optimize_w(h, C.byref(st), None, C.byref(o), C.byref(sb)) == 0
    assert np.array_equal(a.poses, b.poses) and (sa.iterations, sa.final_cost, sa.termination) == (sb.iterations, sb.final_cost, sb.termination)
    assert sa.iterations > 0 and not np.array_equal(a.poses, g0.poses)
    # linearise, both hooks
    g = g0.copy()
    st = ctx._pgo_struct(g)
    H, grad, cost = ctx.pgo_linearize(g, True, 0.5)
    Hn, gn, cn, nf = np.zeros(n * n), np.zeros(max(n, 1)), C.c_double(), C.c_int32()
    assert L.vsl_pgo_linearize_w(h, C.byref(st), None, C.byref(o), Hn.ctypes.data_as(f64p), gn.ctypes.data_as(f64p), C.byref(cn), C.byref(nf)) == 0
    assert np.array_equal(Hn.reshape(n, n), H) and np.array_equal(gn[:n], grad) and cn.value == cost
    for scale in (0, 1):
        Hs, gs, cs, info = ctx.pgo_linearize_stored(g, True, 0.5, jacobi_scale=bool(scale))
        Hn[:] = 0
        sto, bw, stray = C.c_int32(), C.c_int32(), C.c_int32()
        assert L.vsl_pgo_linearize_stored_w(h, C.byref(st), None, C.byref(o), scale, Hn.ctypes.data_as(f64p), gn.ctypes.data_as(f64p),
                                            C.byref(cn), C.byref(nf), C.byref(sto), C.byref(bw), C.byref(stray)) == 0
        assert np.array_equal(Hn.reshape(n, n), Hs) and np.array_equal(gn[:n], gs) and cn.value == cs
        assert (sto.value, bw.value, stray.value) == (info["storage"], info["half_bandwidth"], info["stray_nonzeros"])
    # marginals
    free = np.flatnonzero(g.node_fixed == 0).astype(np.int32)
    nodes = np.ascontiguousarray(free[[0, len(free) // 2, -1]])
    cov, route = ctx.pgo_covariance(g, nodes, True, 0.5)
    covn, rt = np.zeros_like(cov), C.c_int(-1)
    assert L.vsl_pgo_covariance_w(h, C.byref(st), None, C.byref(o), nodes.ctypes.data_as(i32p), len(nodes), covn.ctypes.data_as(f64p), C.byref(rt)) == 0
    assert np.array_equal(cov, covn) and rt.value == route and cov.any()
    pa, pb = np.ascontiguousarray(nodes[:2]), np.ascontiguousarray(nodes[1:])
    joint, _ = ctx.pgo_joint_covariance(g, np.stack([pa, pb], axis=1), True, 0.5)
    jn = np.zeros_like(joint)
    assert L.vsl_pgo_joint_covariance_w(h, C.byref(st), None, C.byref(o), pa.ctypes.data_as(i32p), pb.ctypes.data_as(i32p), 2,
                                        jn.ctypes.data_as(f64p), C.byref(rt)) == 0
    assert np.array_equal(joint, jn) and joint.any()
    meas = np.full((2, 6), 0.01)
    mc = np.tile(1e-3 * np.eye(6), (2, 1, 1))
    r, rc, x2, _ = ctx.pgo_edge_consistency(g, pa, pb, meas, mc, True, 0.5)
    rn, rcn, x2n = np.zeros_like(r), np.zeros_like(rc), np.zeros_like(x2)
    assert L.vsl_pgo_edge_consistency_w(h, C.byref(st), None, C.byref(o), pa.ctypes.data_as(i32p), pb.ctypes.data_as(i32p),
                                        meas.ctypes.data_as(f64p), mc.ctypes.data_as(f64p), 2, rn.ctypes.data_as(f64p),
                                        rcn.ctypes.data_as(f64p), x2n.ctypes.data_as(f64p), C.byref(rt)) == 0
    assert np.array_equal(r, rn) and np.array_equal(rc, rcn) and np.array_equal(x2, x2n) and x2.all()


# ------------------------------------------------------------------------------------------------ 4. solve
NOISE, LOOP_OFFSET = 0.002, 0.3
_SOLVE = {}


def _solve_case(synth, name, loop_weight):
    """Noisy odometry, the last edge (synth.pose_graph: the loop constraint, fixed node n - 1 -> node 0; the chain: its
    last window edge) moved by 0.3 in translation; every edge diag(1e2 x 3, 1e4 x 3), that edge loop_weight x I.
    Returns (graph, Omega, reference minimum)."""
    key = (name, loop_weight)
    if key not in _SOLVE:
        if wr.STORAGE_GRAPHS[name][0] is None:
            g = wr.chain120(NOISE)
        else:
            g = wr.graph_of(synth.pose_graph(**dict(wr.STORAGE_GRAPHS[name][0], meas_noise=NOISE, outlier_edges=0)), name)
            assert (g.edge_a[-1], g.edge_b[-1]) == (len(g.poses) - 1, 0)
        g.edge_meas[-1, :3] += LOOP_OFFSET
        W = wr.family("diag", len(g.edge_a))
        W[-1] = loop_weight * np.eye(6)
        _SOLVE[key] = (g, W, wr.minimize(g, W, use_huber=False))
    return _SOLVE[key]


_LM = {}


def _lm_case(synth, name, loop_weight):
    key = (name, loop_weight)
    if key not in _LM:
        g, W, _ = _solve_case(synth, name, loop_weight)
        _LM[key] = wr.minimize_lm(g, W, use_huber=False)
    return _LM[key]


def _solve(ctx, g, W, dense=False):
    ctx.set_diagnostic("ba_force_dense", int(dense))
    try:
        return ctx.pose_graph_optimize(g, False, 1.0, 50, edge_info=W)
    finally:
        ctx.set_diagnostic("ba_force_dense", 0)


@pytest.mark.parametrize("name", list(wr.STORAGE_GRAPHS))
def test_weighted_solve_reaches_the_reference_minimum(ctx, synth, name):
    """The reference minimum is pgo_weighted_ref.minimize_lm: the damped Gauss-Newton run in long double with the damping
    and the stop rules of lm_policy.h, so that "converged" means for the reference what it means for the solver (the
    oracle of tests/test_pgo_gpu.py is built the same way).  Same trajectory (iterations, termination, successful
    steps), cost within reference x (1 + LM_FUNCTION_TOLERANCE x iterations) -- of that reference AND of the minimum a
    Gauss-Newton run to a step of 1e-13 reaches (minimize) --, poses within 1e-7, same bits twice, the dense route within
    1e-7.  The distance to the tightly converged minimiser is printed: a stop on a relative cost change of 1e-6 leaves
    more than 1e-7 there."""
    closing = []
    for w in (1e4, 1e-2):
        g0, W, tight = _solve_case(synth, name, w)
        m = _lm_case(synth, name, w)
        a, b, c = g0.copy(), g0.copy(), g0.copy()
        s = _solve(ctx, a, W)
        err = float(np.abs(a.poses - m.poses).max())
        print("%s loop weight %g: (%d, %d, %d) iterations / termination / successful steps, reference (%d, %d, %d); cost %.12e, "
              "reference %.12e, tightly converged %.12e; poses %.3e from the reference (bound %.1e), %.3e from the tightly converged minimiser"
              % (name, w, s.iterations, s.termination, s.successful_steps, m.iterations, m.termination, m.successful_steps, s.final_cost,
                 m.cost, tight.cost, err, POSE_TOL, float(np.abs(a.poses - tight.poses).max())))
        assert (s.iterations, s.termination, s.successful_steps) == (m.iterations, m.termination, m.successful_steps)
        assert abs(s.initial_cost - m.initial_cost) <= 1e-9 * m.initial_cost
        assert s.final_cost <= m.cost * (1 + LM_FUNCTION_TOLERANCE * s.iterations)
        assert s.final_cost <= tight.cost * (1 + LM_FUNCTION_TOLERANCE * s.iterations) and s.final_cost < s.initial_cost
        assert abs(wr.total_cost(g0, W, False, poses=a.poses) - s.final_cost) <= 1e-9 * s.final_cost
        assert err < POSE_TOL
        fixed = np.flatnonzero(g0.node_fixed)
        assert np.array_equal(a.poses[fixed], g0.poses[fixed])
        s2 = _solve(ctx, b, W)
        assert np.array_equal(a.poses, b.poses) and (s2.iterations, s2.final_cost) == (s.iterations, s.final_cost)
        sd = _solve(ctx, c, W, dense=True)
        errd = float(np.abs(a.poses - c.poses).max())
        print("  dense route: poses %.3e from the stored route's (bound %.1e)" % (errd, POSE_TOL))
        assert errd < POSE_TOL and (sd.iterations, sd.termination, sd.successful_steps) == (s.iterations, s.termination, s.successful_steps)
        end = g0.edge_b[-1] if g0.node_fixed[g0.edge_a[-1]] else g0.edge_a[-1]
        closing.append(a.poses[end, 4:].copy())
    moved = float(np.linalg.norm(closing[0] - closing[1]))
    print("%s: the closing pose moves by %.3f between the two loop weights (noise %g)" % (name, moved, NOISE))
    assert moved > 10 * NOISE


# ------------------------------------------------------------------------------------------------ 5. marginals
def _queries(g):
    free = np.flatnonzero(g.node_fixed == 0)
    nodes = [int(free[0]), int(free[5]), int(free[len(free) // 2]), int(free[-1])]
    fixed = int(np.flatnonzero(g.node_fixed)[0])
    pairs = [(nodes[0], nodes[1]), (nodes[2], nodes[0]), (nodes[3], nodes[1]), (fixed, nodes[2]), (nodes[1], nodes[0])]
    return nodes, pairs


def _sigma(g, lin, nodes):
    """(columns of the reference H^-1 of the queried nodes: node -> [n, 6] long double, the covariance bound)"""
    free = g.free_index()
    cols = np.concatenate([np.arange(6 * free[v], 6 * free[v] + 6) for v in nodes])
    X = wr.columns_of_inverse(lin.H_ld, cols)
    return {v: X[:, 6 * k:6 * k + 6] for k, v in enumerate(nodes)}, wr.cov_tolerance(lin.H_ld, float(np.abs(X).max()))


def _joint(g, X, a, b):
    free = g.free_index()
    out = np.zeros((12, 12), wr.LD)
    for x, nx in enumerate((a, b)):
        for y, ny in enumerate((a, b)):
            if free[nx] >= 0 and free[ny] >= 0:
                out[6 * x:6 * x + 6, 6 * y:6 * y + 6] = X[ny][6 * free[nx]:6 * free[nx] + 6]
    return out


@pytest.mark.parametrize("fam", ["diag", "random"])
@pytest.mark.parametrize("name", list(wr.STORAGE_GRAPHS))
def test_weighted_marginals_match_the_inverse_of_the_reference(ctx, synth, name, fam):
    g, W, thr, lin = wr.cases(synth)[(name, fam, True)]
    nodes, pairs = _queries(g)
    X, tol = _sigma(g, lin, nodes)
    free = g.free_index()
    cov, route = ctx.pgo_covariance(g, nodes, True, thr, edge_info=W)
    assert route == wr.graphs(synth)[name][1]
    err = max(float(np.abs(cov[k] - X[v][6 * free[v]:6 * free[v] + 6]).max()) for k, v in enumerate(nodes))
    joint, _ = ctx.pgo_joint_covariance(g, pairs, True, thr, edge_info=W)
    want = np.stack([_joint(g, X, a, b) for a, b in pairs])
    errj = float(np.abs(joint - want).max())
    print("%s %s: covariance %.3e, joint %.3e, bound %.3e (route %d)" % (name, fam, err, errj, tol, route))
    assert err <= tol and errj <= tol
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(joint, joint.transpose(0, 2, 1))
    # a subset query returns the same bits; (b, a) is (a, b) with the blocks swapped; the diagonal blocks are pgo_covariance's
    sub, _ = ctx.pgo_covariance(g, nodes[1:3], True, thr, edge_info=W)
    assert np.array_equal(sub, cov[1:3])
    one, _ = ctx.pgo_joint_covariance(g, pairs[2:3], True, thr, edge_info=W)
    assert np.array_equal(one[0], joint[2])
    perm = np.r_[6:12, 0:6]
    assert np.array_equal(joint[4], joint[0][perm][:, perm])
    assert np.array_equal(joint[0][:6, :6], cov[0]) and np.array_equal(joint[0][6:, 6:], cov[1])
    # chi-square of a candidate gated with Sigma_m against the weighted graph: the residual stays unwhitened
    rng = np.random.default_rng(3)
    P = pg._ld(g.poses)
    cands = pairs[:4]
    meas = np.stack([(pg.residual(P[a], P[b], np.zeros(6)) + wr.LD(0.05) * rng.normal(size=6)).astype(np.float64) for a, b in cands])
    B = rng.normal(size=(len(cands), 6, 6))
    mc = 1e-3 * (B @ B.transpose(0, 2, 1)) + 1e-4 * np.eye(6)
    resid, rcov, chi2, _ = ctx.pgo_edge_consistency(g, [p[0] for p in cands], [p[1] for p in cands], meas, mc, True, thr, edge_info=W)
    for q, (a, b) in enumerate(cands):
        r, Ja, Jb, _ = pg.residual_jacobian(P[a], P[b], meas[q])
        Ja, Jb = (Ja if free[a] >= 0 else 0 * Ja), (Jb if free[b] >= 0 else 0 * Jb)
        S, J = want[q], np.concatenate([Ja, Jb], axis=1)
        M = J @ S @ J.T
        Sr = (M + M.T) / 2
        nj = float(np.abs(Ja).sum(axis=1).max() + np.abs(Jb).sum(axis=1).max())
        b_cov = tol * nj * nj + pg.GPU_TOL * float(max(np.abs(Ja).max(), np.abs(Jb).max())) * 2 * float(np.abs(S).max()) * nj
        A = Sr + pg._ld(mc[q])
        x2 = jr.chi2_ld(r, A)
        b_x = 64 * float(np.linalg.cond(np.asarray(A, np.float64))) * b_cov / float(np.abs(Sr).max())
        b_r = pg.GPU_TOL * float(np.abs(pg.residual(P[a], P[b], np.zeros(6))).max())
        e_r, e_c, e_x = float(np.abs(resid[q] - r).max()), float(np.abs(rcov[q] - Sr).max()), abs(float(chi2[q]) - x2) / x2
        print("  candidate %s: resid %.3e (bound %.3e) resid_cov %.3e (bound %.3e) chi2 %.6g rel %.3e (bound %.3e)"
              % ((a, b), e_r, b_r, e_c, b_cov, x2, e_x, b_x))
        assert e_r <= b_r and e_c <= b_cov and e_x <= b_x


@pytest.mark.parametrize("name", list(wr.STORAGE_GRAPHS))
def test_four_times_identity_quarters_the_covariance(ctx, synth, name):
    """Sigma(4 I) = Sigma(I) / 4; each side is within its own bound of the exact value, the weighted bound being a
    quarter of the unweighted one (cond is the same, max|Sigma| a quarter): the two differ by at most twice the former."""
    g, W, _, lin = wr.cases(synth)[(name, "four", False)]
    nodes, pairs = _queries(g)
    X, tol = _sigma(g, lin, nodes)
    cov, _ = ctx.pgo_covariance(g, nodes, False, 1.0)
    covw, _ = ctx.pgo_covariance(g, nodes, False, 1.0, edge_info=W)
    joint, _ = ctx.pgo_joint_covariance(g, pairs, False, 1.0)
    jointw, _ = ctx.pgo_joint_covariance(g, pairs, False, 1.0, edge_info=W)
    e1, e2 = float(np.abs(covw - cov / 4).max()), float(np.abs(jointw - joint / 4).max())
    print("%s: |Sigma(4 I) - Sigma / 4| %.3e, joint %.3e, bound %.3e" % (name, e1, e2, 2 * tol))
    assert e1 <= 2 * tol and e2 <= 2 * tol and covw.any()


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("kind", ["zero", "indefinite", "nan", "pivot_1e-40"])
def test_a_bad_block_is_refused_naming_the_lowest_edge(ctx, vsl, synth, kind):
    g = wr.graphs(synth)["tiny65"][0].copy()
    bad = wr.bad_blocks()
    other = bad["nan" if kind != "nan" else "zero"]
    for low, high in ((10, 64), (64, None), (0, 63)):      # edge 64 is the second workgroup's only thread
        W = wr.family("random", 65)
        W[low] = bad[kind]
        if high is not None:
            W[high] = other
        before = g.poses.tobytes()
        calls = (lambda: ctx.pose_graph_optimize(g, True, 1.0, 20, edge_info=W), lambda: ctx.pgo_linearize(g, edge_info=W),
                 lambda: ctx.pgo_linearize_stored(g, edge_info=W), lambda: ctx.pgo_covariance(g, [3], edge_info=W),
                 lambda: ctx.pgo_joint_covariance(g, [(3, 9)], edge_info=W),
                 lambda: ctx.pgo_edge_consistency(g, [3], [9], np.zeros((1, 6)), edge_info=W))
        for call in calls:
            with pytest.raises(vsl.VslError) as e:
                call()
            assert e.value.code == -1 and "edge %d " % low in str(e.value), str(e.value)
            assert g.poses.tobytes() == before
    s = ctx.pose_graph_optimize(g, True, 1.0, 20, edge_info=wr.family("random", 65))      # the context is still usable
    assert s.final_cost < s.initial_cost


def test_asymmetry_within_rounding_is_averaged(ctx, synth):
    g = wr.graphs(synth)["tiny65"][0]
    W = wr.family("random", 65)
    A = W.copy()
    A[:, 0, 5] *= 1 + 1e-12
    A[:, 3, 1] *= 1 - 1e-12
    A[:, 2, 4] += 1e-13
    assert not np.array_equal(A, A.transpose(0, 2, 1))
    S = 0.5 * (A + A.transpose(0, 2, 1))
    x, y = ctx.pgo_linearize(g, True, 0.5, edge_info=A), ctx.pgo_linearize(g, True, 0.5, edge_info=S)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    a, b = g.copy(), g.copy()
    ctx.pose_graph_optimize(a, True, 0.5, 20, edge_info=A)
    ctx.pose_graph_optimize(b, True, 0.5, 20, edge_info=S)
    assert np.array_equal(a.poses, b.poses)


def test_wrong_shape_or_dtype_is_a_value_error(ctx, synth):
    g = wr.graphs(synth)["tiny65"][0].copy()
    before = g.poses.copy()
    for W in (np.zeros((64, 6, 6)), np.zeros((65, 36)), np.zeros((65, 6, 6), np.float32), [[np.eye(6)] * 65], np.zeros((65, 6, 7))):
        for call in (lambda: ctx.pose_graph_optimize(g, edge_info=W), lambda: ctx.pgo_linearize(g, edge_info=W),
                     lambda: ctx.pgo_linearize_stored(g, edge_info=W), lambda: ctx.pgo_covariance(g, [3], edge_info=W),
                     lambda: ctx.pgo_joint_covariance(g, [(3, 9)], edge_info=W),
                     lambda: ctx.pgo_edge_consistency(g, [3], [9], np.zeros((1, 6)), edge_info=W)):
            with pytest.raises(ValueError):
                call()
    assert np.array_equal(g.poses, before)
