"""TEST INFRASTRUCTURE: reference of the pose-graph entry points with per-edge information matrices (the _w calls of
pgo.hip), on top of tests/pgo_ref.py.  numpy only; imports neither the package nor the oracle.

  Omega       [E, 6, 6]; the two mirror entries of a block are averaged; Omega = L L^T by a hand-written 6 x 6 Cholesky
              (numpy's linalg has no long double), U = L^T.  A pivot d with d <= 2^-36 Omega_jj, or one that is not finite,
              raises NotPositiveDefinite with the lowest such edge: the rule of the kernel.
  whitening   r_w = U r, Ja_w = U Ja, Jb_w = U Jb
  Huber       pgo_ref.huber_correct on the whitened quantities: rho on r^T Omega r
  assembly    H = sum J_w^T J_w, g = sum J_w^T r_w, cost = sum rho / 2, edge by edge as pgo_ref.linearize
  minimum     damped Gauss-Newton: residuals, Jacobians, cost and gradient in long double; the step solves
              (H + lambda diag H) d = -g with H rounded to double (an inexact Newton step: the fixed point, g = 0 in long
              double, does not depend on how exactly the step is solved).  Stops when the step is below 1e-13 (relative to
              1 + max|pose|) or the cost stops decreasing at lambda = 1e8.
Every function takes a dtype: np.longdouble is the reference, np.float64 the "plain fp64 restatement": r in double by
the closed formulas of the logarithm, J in double by the complex-step derivative (h = 1e-30 along T exp(delta) to first
order: exact up to the rounding of the evaluation, no subtraction), then the same Cholesky, whitening, corrector and
assembly in double.  F64_VS_REF_W is the largest discrepancy of the two over cases().
"""
import numpy as np

import pgo_ref as pg

LD = pg.LD

# Largest fp64-restatement-versus-reference discrepancy of H, g (relative to max|H|, max|g| of the matrix) and the cost
# (relative) over cases(): measured by tests/test_pgo_weighted_ref_cpu.py::test_fp64_restatement_agrees_with_the_reference
# (x86-64, 80-bit long double), which prints it and asserts that it does not exceed this constant.  The GPU tests allow
# GPU_TOL_W = 8 x this -- the rule of pgo_ref.GPU_TOL -- since there is no oracle for the weighted problem.
# The fp64 side evaluates r and J in double as well (as the oracle does for pgo_ref.ORACLE_VS_REF): a first version that
# started from the reference's r and J rounded to double measured 5.5e-16 -- the rounding of the whitening and the sums
# alone, not what any double evaluation of the logarithm and its derivatives can reach.
# Measured 3.07e-14 (g of the dense 30-node graph under the random family with Huber on; H there 2.3e-14).  Recorded
# rounded up.
F64_VS_REF_W = 3.1e-14
GPU_TOL_W = 8.0 * F64_VS_REF_W

FAMILIES = ("identity", "four", "diag", "random")
DIAG = np.array([1e2, 1e2, 1e2, 1e4, 1e4, 1e4])


class NotPositiveDefinite(ValueError):
    def __init__(self, edge):
        ValueError.__init__(self, "edge_info of edge %d is not positive definite" % edge)
        self.edge = edge


def family(name, E, seed=0):
    """[E, 6, 6] float64.  random: SPD, condition number 10^c with c uniform in [0, 6] (the first edge has 1e6 exactly),
    eigenvectors random: translation and rotation are correlated."""
    if name == "identity":
        return np.tile(np.eye(6), (E, 1, 1))
    if name == "four":
        return np.tile(4.0 * np.eye(6), (E, 1, 1))
    if name == "diag":
        return np.tile(np.diag(DIAG), (E, 1, 1))
    assert name == "random"
    rng = np.random.default_rng(1000 + seed)
    out = np.zeros((E, 6, 6))
    for e in range(E):
        c = 6.0 if e == 0 else rng.uniform(0, 6)
        lam = 10.0 ** np.concatenate([[-c / 2, c / 2], rng.uniform(-c / 2, c / 2, 4)])
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        W = (Q * lam) @ Q.T
        out[e] = (W + W.T) / 2
    return out


def bad_blocks():
    """name -> a 6 x 6 block the rule refuses"""
    tiny = np.eye(6)
    tiny[4, 5] = tiny[5, 4] = 2.0 ** -47
    tiny[5, 5] = 2.0 ** -94 + 1e-40      # pivot 1e-40 under Omega_55 = 5e-29: far below 2^-36 Omega_55
    return {"zero": np.zeros((6, 6)), "indefinite": np.diag([1.0, 1, 1, -1, 1, 1]), "nan": np.full((6, 6), np.nan),
            "pivot_1e-40": tiny}


def cholesky_upper(info, dtype=LD):
    """U [E, 6, 6] (upper triangular, Omega = U^T U) in `dtype`."""
    W = np.asarray(info, dtype).reshape(-1, 6, 6)
    W = (W + W.transpose(0, 2, 1)) / 2
    E = len(W)
    L = np.zeros((E, 6, 6), dtype)
    bad = np.zeros(E, bool)
    thr = dtype(2.0) ** -36
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(6):
            d = W[:, j, j] - np.sum(L[:, j, :j] * L[:, j, :j], axis=-1)
            bad |= ~np.isfinite(d) | ~(d > thr * W[:, j, j])
            l = np.sqrt(np.where(bad, dtype(1), d))
            L[:, j, j] = l
            for i in range(j + 1, 6):
                L[:, i, j] = (W[:, i, j] - np.sum(L[:, i, :j] * L[:, j, :j], axis=-1)) / l
    if bad.any():
        raise NotPositiveDefinite(int(np.flatnonzero(bad)[0]))
    return L.transpose(0, 2, 1).copy()


_RAW = {}


def raw_terms(g):
    """r, Ja, Jb of the graph's edges at its poses in long double, unweighted and without corrector (cached per graph
    object: the Jacobians are the expensive part and do not depend on the weights)."""
    key = id(g)
    if key not in _RAW or _RAW[key][0] is not g:
        P = pg._ld(g.poses)
        r, Ja, Jb, dis = pg.residual_jacobian(P[g.edge_a], P[g.edge_b], g.edge_meas) if len(g.edge_a) else \
            (np.zeros((0, 6), LD), np.zeros((0, 6, 6), LD), np.zeros((0, 6, 6), LD), np.zeros(0, LD))
        _RAW[key] = (g, r, Ja, Jb)
    return _RAW[key][1:]


def _log64(q, t):
    """se3 logarithm in the dtype of the arguments (float64 or complex128): the closed formulas, atan(n / w)"""
    v, w = q[..., :3], q[..., 3:4]
    n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
    ns = np.where(n == 0, 1.0, n)
    om = np.where(n == 0, 2.0 / w, 2.0 * np.arctan(ns / w) / ns) * v
    th = np.sqrt(np.sum(om * om, axis=-1, keepdims=True))
    small = np.abs(th) < 1e-6
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0, (1.0 - ths * np.cos(ths / 2) / (2.0 * np.sin(ths / 2))) / (ths * ths))
    a = pg._cross(om, t)
    return np.concatenate([t - a / 2 + c * pg._cross(om, a), om], axis=-1)


def _residual64(Ta, Tb, meas):
    qi = pg.q_conj(Ta[..., :4])
    return _log64(pg.q_mul(qi, Tb[..., :4]), pg.q_rot(qi, Tb[..., 4:] - Ta[..., 4:])) - meas


_RAW64 = {}


def raw_terms_f64(g):
    """r, Ja, Jb in double arithmetic: J by the complex step (T exp(i h e_k) to first order: q (x) (i h e / 2, 1),
    t + R i h e)."""
    key = id(g)
    if key not in _RAW64 or _RAW64[key][0] is not g:
        E, h = len(g.edge_a), 1e-30
        Ta, Tb, meas = g.poses[g.edge_a].astype(np.complex128), g.poses[g.edge_b].astype(np.complex128), g.edge_meas
        r = _residual64(Ta.real, Tb.real, meas) if E else np.zeros((0, 6))
        J = np.zeros((E, 6, 12))
        for side in range(2):
            for k in range(6):
                T = (Ta, Tb)[side]
                P = T.copy()
                if k < 3:
                    P[..., 4:] = T[..., 4:] + pg.q_rot(T[..., :4], 1j * h * np.eye(3)[k])
                else:
                    dq = np.concatenate([0.5j * h * np.eye(3)[k - 3], [1.0]]).astype(np.complex128)
                    P[..., :4] = pg.q_mul(T[..., :4], np.broadcast_to(dq, T[..., :4].shape))
                if E:
                    J[:, :, 6 * side + k] = _residual64(P if side == 0 else Ta, P if side == 1 else Tb, meas).imag / h
        _RAW64[key] = (g, r, J[..., :6].copy(), J[..., 6:].copy())
    return _RAW64[key][1:]


def whiten(U, r, Ja, Jb):
    return np.einsum("eij,ej->ei", U, r), np.einsum("eij,ejk->eik", U, Ja), np.einsum("eij,ejk->eik", U, Jb)


def weighted_huber(U, r, Ja, Jb, use_huber, huber):
    """(k r_w, k Ja_w, k Jb_w, rho(r^T Omega r) / 2, |r_w|) per edge, in the dtype of the arguments."""
    rw, Jaw, Jbw = whiten(U, r, Ja, Jb)
    norm = np.sqrt(np.sum(rw * rw, axis=-1))
    dt = rw.dtype.type
    s = np.sum(rw * rw, axis=-1)
    a = dt(huber)
    out = bool(use_huber) & (s > a * a)
    rt = np.sqrt(np.where(out, s, dt(1)))
    k = np.sqrt(np.where(out, a / rt, dt(1)))
    rho = np.where(out, 2 * a * rt - a * a, s)
    return k[..., None] * rw, k[..., None, None] * Jaw, k[..., None, None] * Jbw, rho / 2, norm


def assemble(g, r, Ja, Jb):
    """H, grad over the free nodes in node order, edge by edge, in the dtype of the arguments."""
    n = g.n_unknowns()
    H, grad = np.zeros((n, n), r.dtype), np.zeros(n, r.dtype)
    free = g.free_index()
    JaT, JbT = Ja.transpose(0, 2, 1), Jb.transpose(0, 2, 1)
    ga, gb = np.einsum("eij,ej->ei", JaT, r), np.einsum("eij,ej->ei", JbT, r)
    Haa, Hab, Hbb = JaT @ Ja, JaT @ Jb, JbT @ Jb
    for e in range(len(g.edge_a)):
        a, b = 6 * free[g.edge_a[e]], 6 * free[g.edge_b[e]]
        if a >= 0:
            grad[a:a + 6] += ga[e]
            H[a:a + 6, a:a + 6] += Haa[e]
        if b >= 0:
            grad[b:b + 6] += gb[e]
            H[b:b + 6, b:b + 6] += Hbb[e]
        if a >= 0 and b >= 0:
            H[a:a + 6, b:b + 6] += Hab[e]
            H[b:b + 6, a:a + 6] += Hab[e].T
    return H, grad


class Lin:
    """H, g (float64), cost, H_ld, g_ld, norms (|r_w| per edge, float64)"""


def linearize(g, info, use_huber=True, huber=1.0, dtype=LD):
    """The weighted normal equations at the graph's poses.  dtype = np.float64: the fp64 restatement (r and J evaluated
    in double, then Cholesky, whitening, corrector and assembly in double)."""
    r, Ja, Jb = raw_terms(g) if dtype is LD else raw_terms_f64(g)
    U = cholesky_upper(info, dtype) if len(g.edge_a) else np.zeros((0, 6, 6), dtype)
    rw, Jaw, Jbw, cost, norm = weighted_huber(U, r, Ja, Jb, use_huber, huber)
    out = Lin()
    out.H_ld, out.g_ld = assemble(g, rw, Jaw, Jbw)
    out.H, out.g = out.H_ld.astype(np.float64), out.g_ld.astype(np.float64)
    out.cost = float(np.sum(cost))
    out.norms = norm.astype(np.float64)
    out.raw_norms = np.sqrt(np.sum(r * r, axis=-1)).astype(np.float64)
    return out


def total_cost(g, info, use_huber=True, huber=1.0, poses=None):
    if len(g.edge_a) == 0:
        return 0.0
    P = pg._ld(g.poses if poses is None else poses)
    r = pg.residual(P[g.edge_a], P[g.edge_b], g.edge_meas)
    z = np.zeros(r.shape + (6,), LD)
    return float(np.sum(weighted_huber(cholesky_upper(info), r, z, z, use_huber, huber)[3]))


def _jacobians(Ta, Tb, meas, h=pg.FD_STEP):
    D1, D2 = pg._central(Ta, Tb, h), pg._central(Ta, Tb, h / 2)
    J = (4 * D2 - D1) / 3
    return pg.residual(Ta, Tb, meas), J[..., :6], J[..., 6:]


class Minimum:
    """poses [N, 7] float64 (rounded from long double), cost, iterations, step (the last accepted step's size)"""


def minimize(g, info, use_huber=False, huber=1.0, max_iterations=60):
    P = pg._ld(g.poses).copy()
    U = cholesky_upper(info)
    free = g.free_index()
    nodes = np.flatnonzero(free >= 0)

    def lin(Q):
        r, Ja, Jb = _jacobians(Q[g.edge_a], Q[g.edge_b], g.edge_meas)
        rw, Jaw, Jbw, cost, _ = weighted_huber(U, r, Ja, Jb, use_huber, huber)
        H, grad = assemble(g, rw, Jaw, Jbw)
        return np.sum(cost), H, grad

    def cost_at(Q):
        r = pg.residual(Q[g.edge_a], Q[g.edge_b], g.edge_meas)
        z = np.zeros(r.shape + (6,), LD)
        return np.sum(weighted_huber(U, r, z, z, use_huber, huber)[3])

    out = Minimum()
    cost, H, grad = lin(P)
    lam, out.iterations, out.step = 1e-4, 0, float("inf")
    while out.iterations < max_iterations:
        H64, step_taken = H.astype(np.float64), False
        while lam <= 1e8:
            d = np.linalg.solve(H64 + lam * np.diag(np.diag(H64)), -grad.astype(np.float64))
            Q = P.copy()
            Q[nodes] = pg.se3_mul(P[nodes], pg.se3_exp(pg._ld(d).reshape(-1, 6)))
            c = cost_at(Q)
            if c < cost:
                P, out.step, step_taken = Q, float(np.abs(d).max()), True
                lam = max(lam / 10, 1e-12)
                break
            lam *= 10
        out.iterations += 1
        if not step_taken:
            break
        cost, H, grad = lin(P)
        if out.step <= 1e-13 * (1 + float(np.abs(P).max())):
            break
    P[:, :4] /= np.sqrt(np.sum(P[:, :4] * P[:, :4], axis=-1, keepdims=True))
    out.poses, out.cost, out.gmax = P.astype(np.float64), float(cost), float(np.abs(grad).max())
    return out


def minimize_lm(g, info, use_huber=False, huber=1.0, max_iterations=50):
    """The damped Gauss-Newton run with the damping and the stop rules of the library's step policy (lm_policy.h: Ceres'
    Levenberg-Marquardt defaults -- radius 1e4, function / gradient / parameter tolerance 1e-6 / 1e-10 / 1e-8) and the
    loop of pgo.hip around them, restated in long double: Jacobi scale 1 / (1 + sqrt(diag H)) of the first linearisation,
    (H_s + diag(clamp(diag H_s, 1e-6, 1e32)) / radius) d = -g_s, model change -d (g_s + H_s d / 2), candidate
    T exp(scale d), the gradient tolerance read one step late.  The step is solved in double and refined once on the
    long-double residual.  Returns a Minimum with iterations, termination and successful_steps as vsl_ba_summary counts
    them: converged means what the solver means by it."""
    P = pg._ld(g.poses).copy()
    U = cholesky_upper(info)
    free = g.free_index()
    nodes = np.flatnonzero(free >= 0)

    def lin(Q):
        r, Ja, Jb = _jacobians(Q[g.edge_a], Q[g.edge_b], g.edge_meas)
        rw, Jaw, Jbw, cost, _ = weighted_huber(U, r, Ja, Jb, use_huber, huber)
        H, grad = assemble(g, rw, Jaw, Jbw)
        return np.sum(cost), H, grad

    def cost_at(Q):
        r = pg.residual(Q[g.edge_a], Q[g.edge_b], g.edge_meas)
        z = np.zeros(r.shape + (6,), LD)
        return np.sum(weighted_huber(U, r, z, z, use_huber, huber)[3])

    out = Minimum()
    cost, H, grad = lin(P)
    out.initial_cost = float(cost)
    scale = 1 / (1 + np.sqrt(np.diag(H)))
    radius, decrease, invalid = LD(1e4), LD(2), 0
    it, ok_steps, term, gmax, need_gmax = 0, 0, 0, np.inf, True
    while True:
        if it >= max_iterations:
            term = 0
            break
        if not need_gmax and gmax <= 1e-10:
            term = 2
            break
        if radius <= 1e-32:
            term = 4
            break
        if len(nodes) == 0:
            term = 2
            break
        Hs, gs = scale[:, None] * H * scale[None, :], scale * grad
        A = Hs + np.diag(np.clip(np.diag(Hs), LD(1e-6), LD(1e32)) / radius)
        pending = need_gmax
        if need_gmax:
            gmax_new, need_gmax = float(np.abs(grad).max()), False
        it += 1
        A64 = A.astype(np.float64)
        d = pg._ld(np.linalg.solve(A64, -gs.astype(np.float64)))
        d = d + pg._ld(np.linalg.solve(A64, (-gs - A @ d).astype(np.float64)))
        model = np.sum(-d * (gs + (Hs @ d) / 2))
        step = scale * d
        Q = P.copy()
        Q[nodes] = pg.se3_mul(P[nodes], pg.se3_exp(step.reshape(-1, 6)))
        Q[:, :4] /= np.sqrt(np.sum(Q[:, :4] * Q[:, :4], axis=-1, keepdims=True))
        cand = cost_at(Q)
        if pending:
            gmax = gmax_new
            if gmax <= 1e-10:
                it -= 1
                term = 2
                break
        step_norm, x_norm = np.sqrt(np.sum(step * step)), np.sqrt(np.sum(P[nodes] * P[nodes]))
        if not (np.all(np.isfinite(d)) and model > 0):
            invalid += 1
            if invalid >= 5:
                term = 4
                break
            radius = radius / 2
            continue
        invalid = 0
        change = cost - cand
        if step_norm <= 1e-8 * (x_norm + 1e-8):
            term = 3
            break
        if abs(change) <= 1e-6 * cost:
            term = 1
            break
        rel = change / model
        if rel > 1e-3:
            radius = min(LD(1e16), radius / max(LD(1) / 3, 1 - (2 * rel - 1) ** 3))
            decrease = LD(2)
            P = Q
            cost, H, grad = lin(P)
            need_gmax = True
            ok_steps += 1
        else:
            radius = radius / decrease
            decrease = decrease * 2
    out.poses, out.cost, out.gmax = P.astype(np.float64), float(cost), float(np.abs(grad).max())
    out.iterations, out.termination, out.successful_steps = it, term, ok_steps
    return out


def columns_of_inverse(H_ld, cols):
    """Columns `cols` of H^-1 in long double: double LU solves, refined on the long-double residual (four rounds: each
    gains a factor cond(H) x 2^-52)."""
    H64 = np.asarray(H_ld, np.float64)
    E = np.zeros((len(H_ld), len(cols)), LD)
    E[cols, np.arange(len(cols))] = 1
    X = pg._ld(np.linalg.solve(H64, E.astype(np.float64)))
    for _ in range(4):
        X = X + pg._ld(np.linalg.solve(H64, (E - H_ld @ X).astype(np.float64)))
    return X


def cov_tolerance(H_ld, zmax):
    """The project's covariance rule 64 cond(H) 2^-52 max|Sigma|; cond from the eigenvalues of H rounded to double."""
    lam = np.linalg.eigvalsh(np.asarray(H_ld, np.float64))
    return 64.0 * float(lam[-1] / lam[0]) * 2.0 ** -52 * zmax


# ------------------------------------------------------------------------------------------------------ cases
def graph_of(d, name=""):
    """pgo_ref.Graph of a synth.pose_graph dict"""
    return pg.Graph(d["poses"], d["node_fixed"], d["edge_a"], d["edge_b"], d["edge_meas"], name)


# name -> (arguments of synth.pose_graph, expected storage): the shapes tests/test_pgo_gpu.py uses.  synth.pose_graph
# always closes the loop, so both band graphs from it are cyclic; the linear band is covered by a fourth graph, the same
# size and window without the closing edges (pgo_ref.loop_graph).
STORAGE_GRAPHS = {
    "dense30": (dict(seed=21, n_nodes=30, n_loop_edges=10, meas_noise=0.2, drift=0.02, outlier_edges=2), 0),
    "band120_w3": (dict(seed=33, n_nodes=120, n_loop_edges=0, meas_noise=0.2, drift=0.02, window=3), 2),
    "ring300_w12": (dict(seed=34, n_nodes=300, n_loop_edges=0, meas_noise=0.2, drift=0.02, window=12), 2),
    "chain120_w3": (None, 1),
}


def chain120(noise=0.2):
    return pg.loop_graph(120, window=3, loop=False, fixed=[0], noise=noise, drift=0.02, seed=35, name="chain120_w3")
TINY_EDGE_COUNTS = (0, 1, 64, 65)

_GRAPHS = {}


def tiny_graph(n_edges, seed=7):
    """A chain of n_edges + 1 nodes (node 0 fixed): exactly n_edges edges; 0 edges: two nodes, nothing between them."""
    if n_edges == 0:
        g = pg.loop_graph(2, loop=False, fixed=[0], seed=seed)
        return pg.Graph(g.poses, g.node_fixed, [], [], np.zeros((0, 6)), "tiny0")
    g = pg.loop_graph(n_edges + 1, window=1, loop=False, fixed=[0], noise=0.1, seed=seed, name="tiny%d" % n_edges)
    assert len(g.edge_a) == n_edges
    return g


def graphs(synth):
    """name -> (graph, expected storage or None): the three storage graphs (synth.pose_graph) and the tiny ones."""
    if not _GRAPHS:
        for name, (kw, storage) in STORAGE_GRAPHS.items():
            _GRAPHS[name] = (chain120() if kw is None else graph_of(synth.pose_graph(**kw), name), storage)
        for k in TINY_EDGE_COUNTS:
            _GRAPHS["tiny%d" % k] = (tiny_graph(k), None)
    return _GRAPHS


def huber_threshold(norms):
    """Half-way between the two middle whitened norms: some edges on each side, none within rounding of it."""
    s = np.sort(norms)
    if len(s) < 2:
        return 1.0
    return float(0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]))


_CASES = None


def cases(synth):
    """(graph name, family, use_huber) -> (graph, Omega, huber threshold, reference Lin), everything the linearise tests
    run: both test files take their cases from here, so the constant is measured on what the GPU tests run."""
    global _CASES
    if _CASES is None:
        C = {}
        for gi, (name, (g, _)) in enumerate(graphs(synth).items()):
            for fam in FAMILIES:
                W = family(fam, len(g.edge_a), seed=gi)
                off = linearize(g, W, False, 1.0)
                thr = huber_threshold(off.norms)
                C[(name, fam, False)] = (g, W, thr, off)
                C[(name, fam, True)] = (g, W, thr, linearize(g, W, True, thr))
        _CASES = C
    return _CASES
