"""CPU: pins tests/pgo_ref.py (the long-double reference of the pose-graph normal equations) and measures the oracle
(oracle/orc_pgo.cpp) against it on every case the GPU tests of test_pgo_edges_gpu.py use.  The largest discrepancy is
printed (`pytest -s`) and must not exceed pgo_ref.ORACLE_VS_REF, the constant the GPU tolerance is 8 x of."""
import ctypes

import numpy as np

import pgo_ref as ref

LD = np.longdouble


def _arr(orc, g):
    return orc.PgoArrays(g.poses, g.node_fixed, g.edge_a, g.edge_b, g.edge_meas)


def test_long_double_is_wider_than_double():
    # the reference's error estimates assume the x87 80-bit format (or better)
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_log_inverts_exp_over_the_angle_table():
    rng = np.random.default_rng(0)
    worst = 0.0
    for angle in ref.ANGLES:
        for tn in ref.TRANSLATIONS:
            for ax in range(4):
                axis = rng.normal(size=3) if ax == 0 else np.eye(3)[ax - 1]
                axis = axis / np.linalg.norm(axis)
                t = rng.normal(size=3)
                xi = np.concatenate([LD(tn) * t / np.linalg.norm(t), LD(angle) * LD(1) * axis]).astype(LD)
                back = ref.se3_log(ref.se3_exp(xi))
                if not np.any(xi):
                    assert not np.any(back)
                    continue
                worst = max(worst, float(np.abs(back - xi).max() / np.abs(xi).max()))
    print("log(exp(xi)) - xi, relative: %.3g" % worst)
    assert worst < 1e-16


def test_c_series_meets_the_closed_form():
    # the two evaluations of c(theta) agree where they change over (0.25) and the series' first term is 1 / 12
    th = LD(0.25)
    closed = (1 - th * np.cos(th / 2) / (2 * np.sin(th / 2))) / (th * th)
    assert abs(ref._series(ref._C_SERIES, th * th) - closed) < 1e-17
    assert ref._series(ref._C_SERIES, LD(0)) == LD(1) / LD(12)
    closed_b = (th - np.sin(th)) / th ** 3
    assert abs(ref._series(ref._B_SERIES, th * th) - closed_b) < 1e-17


def test_edge_table_stays_a_step_away_from_the_cut():
    edges = ref.edge_table()
    assert len(edges) == 320
    Ta, Tb = np.array([e[0] for e in edges]), np.array([e[1] for e in edges])
    om = ref.se3_log(ref.se3_mul(ref.se3_inv(Ta.astype(LD)), Tb.astype(LD)))[:, 3:]
    theta = np.sqrt(np.sum(om * om, axis=1)).astype(np.float64)
    # both endpoints are perturbed by at most FD_STEP (one at a time); the nearest angle is 1e-3 from pi
    assert theta.max() + 4 * ref.FD_STEP < np.pi
    # every angle of the table is present, on the intended side of the kernel's thresholds
    for a in ref.ANGLES:
        assert np.any(np.abs(theta - a) <= 1e-15 + 1e-9 * a), a
    q = ref.q_mul(ref.q_conj(Ta[:, :4].astype(LD)), Tb[:, :4].astype(LD))
    sq_n = np.sum(q[:, :3] ** 2, axis=1).astype(np.float64)
    assert (sq_n == 0).sum() == 32 and ((sq_n > 0) & (sq_n < 1e-20)).sum() == 32 and ((sq_n > 1e-20) & (sq_n < 1e-19)).sum() == 32
    assert ((theta > 1e-7) & (theta < 1e-6)).sum() == 32 and ((theta > 1e-6) & (theta < 1e-5)).sum() == 32
    assert (q[:, 3] < 0).sum() == 160


def test_jacobian_step_halving_disagreement_is_below_the_gpu_bound():
    edges = ref.edge_table()
    Ta, Tb, m = (np.array([e[k] for e in edges]) for k in range(3))
    _, Ja, Jb, dis = ref.residual_jacobian(Ta, Tb, m)
    print("finite differences, step halving: max %.3g (GPU bound %.3g)" % (dis.max(), ref.GPU_TOL))
    assert dis.max() < ref.GPU_TOL
    # and against an independent analytic value: at identical poses and zero residual J_b = I, J_a = -I
    P = np.array([0.1, -0.2, 0.3, 0.9, 1.0, 2.0, 3.0])
    P[:4] /= np.linalg.norm(P[:4])
    _, Ja, Jb, _ = ref.residual_jacobian(P, P, np.zeros(6))
    assert np.abs(Jb - np.eye(6)).max() < 1e-13 and np.abs(Ja + np.eye(6)).max() < 1e-13


def _storage_decision(vsl, g):
    """The storage rule vsl_pose_graph_optimize documents (pgo.hip pgo_storage), restated from the free indices of the
    edges.  A restatement proves nothing about pgo_setup: the check that a topology takes the storage it names is the GPU
    test's assertion on what vsl_pgo_linearize_stored reports.  This only keeps the fixtures' expected values consistent
    with the documented rule and the host-side ring layout without a GPU."""
    free = g.free_index()
    nf = int((free >= 0).sum())
    n = 6 * nf
    fa, fb = free[g.edge_a], free[g.edge_b]
    d = np.abs(fa - fb)[(fa >= 0) & (fb >= 0)]
    lin = int(d.max()) if len(d) else 0
    cyc = int(np.minimum(d, nf - d).max()) if len(d) else 0
    bw_lin, bw_cyc = 6 * lin + 5, 6 * cyc + 5
    B, nb = ctypes.c_int(), ctypes.c_int()
    if n <= 128:
        return 0, 0, n
    if 2 * bw_cyc < bw_lin and vsl.load().vsl_bcr_cyclic_layout(n, bw_cyc, ctypes.byref(B), ctypes.byref(nb)):
        return 2, bw_cyc, n
    if (bw_lin + 33) * 2 < n:
        return 1, bw_lin, n
    return 0, 0, n


def test_topologies_take_the_storage_they_name(vsl):
    T = ref.topologies()
    for name, (g, storage, bw, n) in T.items():
        assert _storage_decision(vsl, g) == (storage, bw, n), name
        assert n < 500
    # 22 free nodes are the smallest ring that is kept cyclic: one fewer is 126 <= 128 unknowns (dense)
    B, nb = ctypes.c_int(), ctypes.c_int()
    assert vsl.load().vsl_bcr_cyclic_layout(132, 11, ctypes.byref(B), ctypes.byref(nb)) == 1
    g = T["ring48_mixed"][0]
    pairs = list(zip(g.edge_a.tolist(), g.edge_b.tolist()))
    assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
    assert sum(1 for p in pairs if set(p) == {12, 13}) == 2 and sum(1 for p in pairs if set(p) == {30, 31}) == 1
    assert g.node_fixed[30] and g.node_fixed[31] and not g.node_fixed[7] and all(7 not in p for p in pairs)
    # the loop edge itself makes the wrap-around corner of the all-free ring
    g = T["ring22_all_free"][0]
    assert (21, 0) in list(zip(g.edge_a.tolist(), g.edge_b.tolist())) and not g.node_fixed.any()


def test_oracle_agrees_with_the_reference(orc):
    worst, worst_at, worst_fd, by_angle = 0.0, "", 0.0, {}
    for name, (g, use_huber, h, blocks) in ref.linearize_cases().items():
        R = ref.linearize(g, use_huber, h)
        worst_fd = max(worst_fd, R.fd_disagreement)
        H, grad, cost = orc.pgo_linearize(_arr(orc, g), use_huber, h)
        errs = [ref.cost_error(cost, R.cost)]
        if blocks is None:
            errs += list(ref.rel_errors(H, grad, R.H, R.g))
        else:
            inside = np.zeros(H.shape, bool)
            for e, (_, at, size) in enumerate(blocks):
                s = slice(at, at + size)
                eh, eg = ref.rel_errors(H[s, s], grad[s], R.H[s, s], R.g[s])
                errs += [eh, eg]
                inside[s, s] = True
                if name.startswith("table/"):           # 32 consecutive table edges share an angle
                    a = ref.ANGLES[((70 * int(name.split("/")[2]) + e) % 320) // 32]
                    by_angle[a] = max(by_angle.get(a, 0.0), eh, eg)
            assert not H[~inside].any() and not R.H[~inside].any()
        if max(errs) > worst:
            worst, worst_at = max(errs), name
    print("oracle vs long-double reference: max relative discrepancy %.3g (at %s); finite-difference step halving %.3g"
          % (worst, worst_at, worst_fd))
    print("  by relative rotation of the table: " + ", ".join("%g: %.3g" % kv for kv in sorted(by_angle.items())))
    assert worst_fd < ref.GPU_TOL
    assert worst <= ref.ORACLE_VS_REF
    assert ref.GPU_TOL == min(8 * ref.ORACLE_VS_REF, 1e-9) and worst < 1e-9


def test_oracle_edge_jacobians_agree_with_the_reference(orc):
    edges = ref.edge_table()
    Ta, Tb, m = (np.array([e[k] for e in edges]) for k in range(3))
    r, Ja, Jb, _ = ref.residual_jacobian(Ta, Tb, m)
    worst = 0.0
    for e in range(len(edges)):
        orr, oJa, oJb = orc.pgo_residual_jacobian(Ta[e], Tb[e], m[e])
        scale = max(np.abs(Ja[e]).max(), np.abs(Jb[e]).max())
        worst = max(worst, float(max(np.abs(oJa - Ja[e]).max(), np.abs(oJb - Jb[e]).max()) / scale),
                    float(np.abs(orr - r[e]).max() / max(1.0, np.abs(r[e]).max())))
    print("oracle edge residuals / Jacobians vs reference: %.3g" % worst)
    assert worst <= ref.ORACLE_VS_REF


def test_jacobi_scale_of_the_reference():
    g = ref.topologies()["ring22_all_free"][0]
    A, B = ref.linearize(g), ref.linearize(g, jacobi_scale=True)
    s = 1 / (1 + np.sqrt(np.diag(A.H)))
    assert np.allclose(B.H, s[:, None] * A.H * s[None, :], rtol=1e-14, atol=0) and np.allclose(B.g, s * A.g, rtol=1e-14, atol=1e-300)
    assert abs(ref.total_cost(g) - A.cost) <= 1e-15 * A.cost
