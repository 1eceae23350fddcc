"""TEST INFRASTRUCTURE: plain high-precision numpy reference of the pose-graph normal equations (pgo.hip, orc_pgo.cpp),
in the style of ba_cov_ref.py.  numpy only, np.longdouble throughout; imports neither the package nor the oracle.

  pose      [..., 7] qx qy qz qw tx ty tz (T_w_c); all functions broadcast over leading axes
  log       atan2 everywhere, no series branch in the rotation (only the exact n == 0); the coefficient c of
            V^-1 = I - Om / 2 + c Om^2 by its Taylor series sum |B_2k| theta^(2k-2) / (2k)! below 0.25 (9 terms: the
            next one is below 1e-22) and in closed form above, where 1 - (theta/2) cot(theta/2) >= 5e-3 loses no digits
  residual  r = log(T_a^-1 T_b) - meas                                    (pgo_device.h edge_residual's argument order)
  Jacobians d r / d delta along T * exp(delta), both blocks, by central differences D(h) in long double, Richardson
            extrapolated: J(h) = (4 D(h/2) - D(h)) / 3.  With h = 1e-4: truncation ~ h^4 f^(5) / 480 ~ 1e-18 |f|,
            rounding ~ a few tens of eps |f| / h ~ 1e-14 |f| (eps = 2^-63), both far below 1e-11 max|J|.  The function
            repeats itself at half the step and reports max|J(h) - J(h/2)| / max|J| (measured: at most 5e-14, which is
            mostly the four times larger rounding noise of the half step).
  Huber     the Ceres corrector with rho'' <= 0: r and J scaled by sqrt(rho'), cost = rho(s) / 2
  assembly  dense H = sum_e J_e^T J_e, g = sum_e J_e^T r_e over the free nodes in node order, edge by edge (J_e: the 6 x n
            row block with the edge's one or two 6 x 6 blocks), optionally scaled on both sides by 1 / (1 + sqrt(diag H))
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble

# Largest oracle-versus-reference discrepancy of H (relative to max|H| of the 12 x 12 block or of the matrix), g (relative
# to max|g| likewise) and the cost (relative) over linearize_cases() -- the edge table, the Huber table and every
# topology below: measured by tests/test_pgo_ref_cpu.py::test_oracle_agrees_with_the_reference (x86-64, 80-bit long
# double), which prints it and asserts that it does not exceed this constant.  The GPU tests allow
# GPU_TOL = min(8 x this, 1e-9).
# Measured 1.60e-10 (g of a table edge with relative rotation 2e-6 and translation 1e3; H of such an edge: 8.36e-11): just
# above |theta| = 1e-6 the closed form of c cancels ~12 digits in fp64 and its derivative more.  Every other angle of the
# table stays below 1.5e-11 (g: the rounding of r, ~1e-16 x a
# translation of 1e3, over |r| = 0.1).  Recorded rounded up.
ORACLE_VS_REF = 1.7e-10
GPU_TOL = min(8.0 * ORACLE_VS_REF, 1e-9)

ANGLES = (0.0, 1e-10, 4e-10, 5e-7, 2e-6, 1e-3, 0.3, 1.5, 3.0, float(np.pi) - 1e-3)
TRANSLATIONS = (0.0, 1e-3, 1.0, 1e3)
FD_STEP = 1e-4

_BERNOULLI_ABS = (Fraction(1, 6), Fraction(1, 30), Fraction(1, 42), Fraction(1, 30), Fraction(5, 66), Fraction(691, 2730),
                  Fraction(7, 6), Fraction(3617, 510), Fraction(43867, 798))


def _frac(f):
    return LD(f.numerator) / LD(f.denominator)


def _factorial(k):
    out = 1
    for i in range(2, k + 1):
        out *= i
    return out


_C_SERIES = [_frac(b / _factorial(2 * (k + 1))) for k, b in enumerate(_BERNOULLI_ABS)]      # c = sum_k C_k theta^(2k)
_B_SERIES = [_frac(Fraction((-1) ** k, _factorial(2 * k + 3))) for k in range(10)]          # (th - sin th) / th^3


def _ld(x):
    return np.asarray(x, dtype=LD)


def _series(coef, x2):
    out = np.zeros_like(x2)
    for c in reversed(coef):
        out = out * x2 + c
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def q_mul(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:4], b[..., :3], b[..., 3:4]
    return np.concatenate([aw * bv + bw * av + _cross(av, bv), aw * bw - np.sum(av * bv, axis=-1, keepdims=True)], axis=-1)


def q_rot(q, p):
    uv = 2 * _cross(q[..., :3], p)
    return p + q[..., 3:4] * uv + _cross(q[..., :3], uv)


def q_conj(q):
    return np.concatenate([-q[..., :3], q[..., 3:4]], axis=-1)


def se3_inv(T):
    qi = q_conj(T[..., :4])
    return np.concatenate([qi, -q_rot(qi, T[..., 4:])], axis=-1)


def se3_mul(A, B):
    return np.concatenate([q_mul(A[..., :4], B[..., :4]), A[..., 4:] + q_rot(A[..., :4], B[..., 4:])], axis=-1)


def se3_exp(xi):
    xi = _ld(xi)
    ups, om = xi[..., :3], xi[..., 3:]
    th2 = np.sum(om * om, axis=-1, keepdims=True)
    th = np.sqrt(th2)
    safe = np.where(th > 0, th, LD(1))
    imag = np.where(th > 0, np.sin(th / 2) / safe, LD(0.5))
    A = np.where(th > 0, 2 * (np.sin(th / 2) / safe) ** 2, LD(0.5))          # (1 - cos th) / th^2 without the cancellation
    B = np.where(th < 0.25, _series(_B_SERIES, th2), (th - np.sin(th)) / (safe * safe * safe))
    a = _cross(om, ups)
    return np.concatenate([imag * om, np.cos(th / 2), ups + A * a + B * _cross(om, a)], axis=-1)


def se3_log(T):
    """(upsilon, omega) of T = (q, t); q need not have unit norm exactly (omega does not depend on its scale)."""
    T = _ld(T)
    v, w, t = T[..., :3], T[..., 3:4], T[..., 4:]
    n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
    half = np.where(w < 0, np.arctan2(-n, -w), np.arctan2(n, w))              # atan(n / w), continuous through w = 0
    om = np.where(n > 0, 2 * half / np.where(n > 0, n, LD(1)), LD(0)) * v    # n == 0 exactly: no rotation
    th2 = np.sum(om * om, axis=-1, keepdims=True)
    th = np.sqrt(th2)
    big = np.where(th < 0.25, LD(1), th)
    c = np.where(th < 0.25, _series(_C_SERIES, th2), (1 - big * np.cos(big / 2) / (2 * np.sin(big / 2))) / (big * big))
    a = _cross(om, t)
    return np.concatenate([t - a / 2 + c * _cross(om, a), om], axis=-1)


def residual(Ta, Tb, meas):
    return se3_log(se3_mul(se3_inv(_ld(Ta)), _ld(Tb))) - _ld(meas)


def _central(Ta, Tb, h):
    """D(h): [..., 6, 12], columns 0..5 delta_a, 6..11 delta_b (the measurement is a constant: left out of the
    difference, where a large one would only add rounding noise)."""
    cols, zero = [], np.zeros(6, LD)
    for side in range(2):
        for k in range(6):
            d = np.zeros(6, LD)
            d[k] = LD(h)
            if side == 0:
                rp = residual(se3_mul(Ta, se3_exp(d)), Tb, zero)
                rm = residual(se3_mul(Ta, se3_exp(-d)), Tb, zero)
            else:
                rp = residual(Ta, se3_mul(Tb, se3_exp(d)), zero)
                rm = residual(Ta, se3_mul(Tb, se3_exp(-d)), zero)
            cols.append((rp - rm) / (2 * LD(h)))
    return np.stack(cols, axis=-1)


def residual_jacobian(Ta, Tb, meas, h=FD_STEP):
    """r [..., 6], Ja, Jb [..., 6, 6] and the step-halving disagreement max|J(h) - J(h/2)| / max|J| per edge [...]."""
    Ta, Tb, meas = _ld(Ta), _ld(Tb), _ld(meas)
    D1, D2, D4 = _central(Ta, Tb, h), _central(Ta, Tb, h / 2), _central(Ta, Tb, h / 4)
    J, Jhalf = (4 * D2 - D1) / 3, (4 * D4 - D2) / 3
    dis = np.abs(J - Jhalf).max(axis=(-1, -2)) / np.abs(J).max(axis=(-1, -2))
    return residual(Ta, Tb, meas), J[..., :6], J[..., 6:], dis


def huber_correct(r, Ja, Jb, use_huber, huber):
    """Ceres corrector, rho'' <= 0: (k r, k Ja, k Jb, rho(s) / 2 per edge) with k = sqrt(rho')."""
    s = np.sum(r * r, axis=-1)
    a = LD(huber)
    out = bool(use_huber) & (s > a * a)
    rt = np.sqrt(np.where(out, s, LD(1)))
    k = np.sqrt(np.where(out, a / rt, LD(1)))
    rho = np.where(out, 2 * a * rt - a * a, s)
    return k[..., None] * r, k[..., None, None] * Ja, k[..., None, None] * Jb, rho / 2


class Graph:
    """The numpy fields of vsl_pgo_problem (what Context._pgo_struct and orc.PgoArrays take)."""

    def __init__(self, poses, node_fixed, edge_a, edge_b, edge_meas, name=""):
        self.poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7).copy()
        self.node_fixed = np.ascontiguousarray(node_fixed, np.uint8).copy()
        self.edge_a = np.ascontiguousarray(edge_a, np.int32).reshape(-1).copy()
        self.edge_b = np.ascontiguousarray(edge_b, np.int32).reshape(-1).copy()
        self.edge_meas = np.ascontiguousarray(edge_meas, np.float64).reshape(-1, 6).copy()
        self.name = name

    def copy(self):
        return Graph(self.poses, self.node_fixed, self.edge_a, self.edge_b, self.edge_meas, self.name)

    def free_index(self):
        free = np.cumsum(self.node_fixed == 0) - 1
        free[self.node_fixed != 0] = -1
        return free

    def n_unknowns(self):
        return 6 * int((self.node_fixed == 0).sum())


class Lin:
    """H, g (float64, rounded from long double), cost, the Jacobi scale used (or None) and the largest finite-difference
    step-halving disagreement of the graph's edges."""


def total_cost(g, use_huber=True, huber=1.0, poses=None):
    """Cost of the graph at `poses` (default: its own), float."""
    if len(g.edge_a) == 0:
        return 0.0
    P = _ld(g.poses if poses is None else poses)
    r = residual(P[g.edge_a], P[g.edge_b], g.edge_meas)
    return float(np.sum(huber_correct(r, np.zeros(r.shape + (6,), LD), np.zeros(r.shape + (6,), LD), use_huber, huber)[3]))


def linearize(g, use_huber=True, huber=1.0, jacobi_scale=False):
    n, E = g.n_unknowns(), len(g.edge_a)
    out = Lin()
    H, grad = np.zeros((n, n), LD), np.zeros(n, LD)
    out.cost, out.fd_disagreement = 0.0, 0.0
    if E:
        P = _ld(g.poses)
        r, Ja, Jb, dis = residual_jacobian(P[g.edge_a], P[g.edge_b], g.edge_meas)
        r, Ja, Jb, cost = huber_correct(r, Ja, Jb, use_huber, huber)
        out.cost, out.fd_disagreement = float(np.sum(cost)), float(dis.max())
        free = g.free_index()
        for e in range(E):                       # edge by edge: the 6 x n row block J_e has at most two 6 x 6 blocks
            ends = [(6 * free[node], Jx) for node, Jx in ((g.edge_a[e], Ja[e]), (g.edge_b[e], Jb[e])) if free[node] >= 0]
            for x, Jx in ends:
                grad[x:x + 6] += Jx.T @ r[e]
                for y, Jy in ends:
                    H[x:x + 6, y:y + 6] += Jx.T @ Jy
    out.scale = None
    if jacobi_scale:
        s = 1 / (1 + np.sqrt(np.diag(H)))
        H, grad = s[:, None] * H * s[None, :], s * grad
        out.scale = s.astype(np.float64)
    out.H, out.g = H.astype(np.float64), grad.astype(np.float64)
    return out


def rel_errors(H, g, Href, gref):
    """(max|H - Href| / max|Href|, max|g - gref| / max|gref|) of a block or a matrix.  A reference that is zero
    throughout (no edge; r exactly zero on an edge) leaves no scale: the absolute error is returned for it, so that any
    tolerance below one ulp of anything asks for zero there as well."""
    if Href.size == 0:
        return 0.0, 0.0
    hs, gs = float(np.abs(Href).max()), float(np.abs(gref).max())
    return float(np.abs(H - Href).max()) / (hs if hs > 0 else 1.0), float(np.abs(g - gref).max()) / (gs if gs > 0 else 1.0)


def cost_error(cost, cost_ref):
    """Relative error of a total cost (absolute when the reference cost is zero)."""
    return abs(cost - cost_ref) / (cost_ref if cost_ref > 0 else 1.0)


# ------------------------------------------------------------------------------------------------------ fixtures
def axis_angle_pose(axis, angle, t=(0, 0, 0)):
    axis = _ld(axis)
    axis = axis / np.sqrt(np.sum(axis * axis))
    return np.concatenate([np.sin(LD(angle) / 2) * axis, [np.cos(LD(angle) / 2)], _ld(t)])


def _unit(rng, k=3):
    v = rng.normal(size=k)
    return v / np.linalg.norm(v)


def _random_pose(rng):
    return np.concatenate([_unit(rng, 4), rng.uniform(-3, 3, 3)])


# q^-1 (x) q has a vector part of exactly zero in double arithmetic for these (for a general unit quaternion the products
# cancel only to ~1e-17): identity, half a turn about x, quarter turns about y and z
EXACT_QUATERNIONS = ((0, 0, 0, 1), (1, 0, 0, 0), (0, np.sqrt(0.5), 0, np.sqrt(0.5)), (0, 0, np.sqrt(0.5), np.sqrt(0.5)))


def edge_table(seed=1):
    """Every angle of ANGLES x (a random axis, x, y, z) x (as built, the second endpoint's quaternion negated: relative
    w < 0) x every norm of TRANSLATIONS (random direction): a list of (T_a, T_b, meas) in float64, T_b = T_a * Rel rounded
    to double, meas = the relative pose's log plus a residual of norm ~0.1 -- 320 edges.  The double rounding moves the
    relative quaternion's vector part by ~1e-16: far less than the distance of 1e-10 / 4e-10 / 5e-7 / 2e-6 from the
    kernel's thresholds (|vec|^2 = 1e-20, |theta| = 1e-6).  Angle 0: the two quaternions are equal bit for bit."""
    rng = np.random.default_rng(seed)
    out = []
    for angle in ANGLES:
        for ax in range(4):
            axis = _unit(rng) if ax == 0 else np.eye(3)[ax - 1]
            for flip in (False, True):
                for tn in TRANSLATIONS:
                    Ta = _random_pose(rng)
                    rel = axis_angle_pose(axis, angle, tn * _unit(rng))
                    Tb = Ta.copy() if (angle == 0.0 and tn == 0.0) else se3_mul(_ld(Ta), rel).astype(np.float64)
                    if angle == 0.0:
                        if ax > 0:
                            Ta[:4] = EXACT_QUATERNIONS[ax]      # |vec|^2 == 0 bit for bit (random axis row: ~1e-34)
                            Tb[4:] = se3_mul(_ld(Ta), rel).astype(np.float64)[4:]
                        Tb[:4] = Ta[:4]
                    if flip:
                        Tb[:4] = -Tb[:4]
                    meas = (residual(Ta, Tb, np.zeros(6)) + _ld(0.1 * _unit(rng, 6))).astype(np.float64)
                    out.append((Ta, Tb, meas))
    return out


FORMS = ("a_fixed", "b_fixed", "a_fixed", "b_fixed", "a_fixed", "b_fixed", "both_free")


def disjoint_graph(edges, offset=0, name=""):
    """One two-node component per edge (nodes 2e, 2e + 1): H is block diagonal.  Edge e takes FORMS[(e + offset) % 7]:
    70 edges are 10 x 12 + 60 x 6 = 480 unknowns.  Returns the graph and, per edge, (form, first unknown, block size)."""
    poses, fixed, blocks, at = [], [], [], 0
    for e, (Ta, Tb, _) in enumerate(edges):
        form = FORMS[(e + offset) % len(FORMS)]
        poses += [Ta, Tb]
        fixed += [int(form == "a_fixed"), int(form == "b_fixed")]
        size = 12 if form == "both_free" else 6
        blocks.append((form, at, size))
        at += size
    E = len(edges)
    return Graph(poses, fixed, 2 * np.arange(E), 2 * np.arange(E) + 1, [m for _, _, m in edges], name), blocks


HUBER_FACTORS = (0.0, 0.999, 1.001, 10.0, 1e3)


def huber_edges(h, seed=2, per_factor=4):
    """Edges whose residual norm is f * h for f in HUBER_FACTORS (meas = log(T_a^-1 T_b) - r computed in long double; the
    double rounding moves |r| by ~1e-16, the nearest factors are 1e-3 h from the threshold).  f = 0: identical poses and a
    zero measurement, so r is exactly zero in any arithmetic."""
    rng = np.random.default_rng(seed)
    out = []
    for f in HUBER_FACTORS:
        for _ in range(per_factor):
            Ta = _random_pose(rng)
            if f == 0.0:
                Ta[:4] = EXACT_QUATERNIONS[len(out) % 4]
                out.append((Ta, Ta.copy(), np.zeros(6)))
                continue
            Tb = se3_mul(_ld(Ta), axis_angle_pose(_unit(rng), rng.uniform(0.1, 2.5), rng.uniform(-2, 2, 3))).astype(np.float64)
            r = LD(f) * LD(h) * _ld(_unit(rng, 6))
            out.append((Ta, Tb, (residual(Ta, Tb, np.zeros(6)) - r).astype(np.float64)))
    return out


def loop_graph(n_nodes, window=1, loop=True, fixed=(), extra=(), noise=0.0, drift=0.02, seed=0, both_orientations=False,
               isolated=(), outliers=0, name=""):
    """Keyframes on a 3 m circle in time order.  Edges (newer, older) between nodes at most `window` apart -- around the
    seam too when `loop` (window = 1: the odometry edges and the loop edge) --, then `extra` pairs.  `isolated` nodes take
    no edge at all (their neighbours are joined directly instead).  both_orientations: every third edge is listed as
    (older, newer).  meas = log(T_a^-1 T_b) of the ground truth + noise (+ N(0, 2) on the translation of `outliers` random
    edges); poses = ground truth * exp(drift * N(0, 1))."""
    rng = np.random.default_rng(seed)
    th = 2 * np.pi * np.arange(n_nodes) / n_nodes
    gt = np.stack([axis_angle_pose([0.1 * np.sin(t), 1.0, 0.1 * np.cos(2 * t)], t + 0.5 * np.pi,
                                   [3 * np.cos(t), 0.3 * np.sin(3 * t), 3 * np.sin(t)]) for t in th])
    live = [k for k in range(n_nodes) if k not in set(isolated)]
    ea, eb = [], []
    for j in range(1, window + 1):
        for i, k in enumerate(live):
            if i + j < len(live):
                ea.append(live[i + j]), eb.append(k)
            elif loop and (i + j) % len(live) != i:
                ea.append(k), eb.append(live[(i + j) % len(live)])         # across the seam: the newer keyframe first
    for a, b in extra:
        ea.append(a), eb.append(b)
    if both_orientations:
        for e in range(0, len(ea), 3):
            ea[e], eb[e] = eb[e], ea[e]
    ea, eb = np.array(ea, np.int64).reshape(-1), np.array(eb, np.int64).reshape(-1)
    meas = np.zeros((0, 6))
    if len(ea):
        meas = residual(gt[ea], gt[eb], np.zeros(6)).astype(np.float64) + noise * rng.normal(size=(len(ea), 6))
        for k in rng.choice(len(ea), outliers, replace=False) if outliers else []:
            meas[k, :3] += rng.normal(0, 2.0, 3)
    poses = se3_mul(gt, se3_exp(drift * rng.normal(size=(n_nodes, 6)))).astype(np.float64)
    node_fixed = np.zeros(n_nodes, np.uint8)
    node_fixed[list(fixed)] = 1
    return Graph(poses, node_fixed, ea, eb, meas, name)


def ground_truth_graph(n_nodes, window, fixed, seed=0):
    """loop_graph at its exact optimum: no noise, no drift (cost ~ 1e-30: only the rounding of the poses to double)."""
    return loop_graph(n_nodes, window=window, fixed=fixed, noise=0.0, drift=0.0, seed=seed, name="optimum")


# name -> (builder, expected storage 0 dense / 1 band / 2 cyclic band, expected half bandwidth (0 when dense), unknowns)
def topologies(noise=2e-3):
    T = {}
    T["ring22_all_free"] = (loop_graph(22, noise=noise, seed=11), 2, 11, 132)
    T["ring22_21_free"] = (loop_graph(22, fixed=[9], noise=noise, seed=12), 0, 0, 126)
    T["ring44_w2_fixed_middle"] = (loop_graph(44, window=2, fixed=[20], noise=noise, seed=13), 2, 17, 258)
    T["ring44_w2_fixed_first"] = (loop_graph(44, window=2, fixed=[0], noise=noise, seed=14), 2, 17, 258)
    T["ring44_w2_fixed_pair"] = (loop_graph(44, window=2, fixed=[20, 21], noise=noise, seed=15), 2, 17, 252)
    T["chain60_w3"] = (loop_graph(60, window=3, loop=False, fixed=[30], noise=noise, seed=16), 1, 23, 354)
    T["ring44_w2_long_edge"] = (loop_graph(44, window=2, fixed=[20], extra=[(33, 5)], noise=noise, seed=17), 0, 0, 258)
    # edges in both orientations, the pair (13, 12) twice, the edge (31, 30) between two fixed nodes, node 7 isolated and
    # free (its neighbours 5, 6 | 8, 9 are joined across it: free indices up to 3 apart, half bandwidth 6 * 3 + 5)
    T["ring48_mixed"] = (loop_graph(48, window=2, fixed=[30, 31], extra=[(13, 12)], isolated=[7], noise=noise, seed=18,
                                    both_orientations=True), 2, 23, 276)
    for name, (g, _, _, _) in T.items():
        g.name = name
    return T


_CASES = None


def linearize_cases():
    """Everything the tests linearise, once: name -> (graph, use_huber, huber, blocks of disjoint_graph or None).
      table/<offset>/<chunk>   70 edges of the 320-edge table from 70 * chunk on (wrapping round), forms moved by offset
      huber/<h>/<on|off>       huber_edges(h)
      topology/<name>          topologies()
    Both test files take their cases from here, so the constant is measured on what the GPU tests run."""
    global _CASES
    if _CASES is None:
        C, table = {}, edge_table()
        for off in range(len(FORMS)):
            for chunk in range(-(-len(table) // 70)):
                name = "table/%d/%d" % (off, chunk)
                g, blocks = disjoint_graph((table[70 * chunk:] + table)[:70], off, name)
                C[name] = (g, True, 1.0, blocks)
        for h in (1e-3, 0.5):
            for on in (True, False):
                name = "huber/%g/%s" % (h, "on" if on else "off")
                g, blocks = disjoint_graph(huber_edges(h), 0, name)
                C[name] = (g, on, h, blocks)
        for name, (g, _, _, _) in topologies().items():
            C["topology/" + name] = (g, True, 1.0, None)
        _CASES = C
    return _CASES
