"""TEST INFRASTRUCTURE: long-double reference of vsl_pgo_joint_covariance and vsl_pgo_edge_consistency.  H comes from
pgo_ref.linearize, its inverse from selinv_ref.inverse_ld; residuals and Jacobians of a candidate edge from
pgo_ref.residual_jacobian (no Huber corrector on the candidate).  numpy only.

  joint block   [[S_aa, S_ab], [S_ba, S_bb]] of S = H^-1, rows and columns of a fixed node exactly zero
  Sigma_r       Ja S_aa Ja^T + Ja S_ab Jb^T + Jb S_ba Ja^T + Jb S_bb Jb^T (a fixed node's terms dropped), symmetrised
  chi2          r^T (Sigma_r + Sigma_m)^-1 r by a long-double Cholesky; NaN when a pivot is not positive
"""
import functools

import numpy as np

import pgo_ref as pg
import selinv_ref as sel

LD = pg.LD


class Case:
    """g, use_huber, huber, H (float64), Z = H^-1 (long double, read-only), tol = selinv_ref.tolerance(H, Z)."""


def make_case(g, use_huber=True, huber=1.0):
    c = Case()
    c.g, c.use_huber, c.huber = g, use_huber, huber
    c.H = pg.linearize(g, use_huber, huber).H
    c.Z = sel.inverse_ld(c.H)
    c.Z.setflags(write=False)
    c.tol = sel.tolerance(c.H, c.Z)
    c.free = g.free_index()
    return c


def _idx(c, node):
    f = c.free[node]
    return None if f < 0 else slice(6 * f, 6 * f + 6)


def joint_block(c, a, b):
    """12 x 12 long double, order (a, b)."""
    out = np.zeros((12, 12), LD)
    for x, nx in enumerate((a, b)):
        for y, ny in enumerate((a, b)):
            ix, iy = _idx(c, nx), _idx(c, ny)
            if ix is not None and iy is not None:
                out[6 * x:6 * x + 6, 6 * y:6 * y + 6] = c.Z[ix, iy]
    return out


def joint_blocks(c, pairs):
    return np.stack([joint_block(c, a, b) for a, b in pairs]) if len(pairs) else np.zeros((0, 12, 12), LD)


def edge_terms(c, a, b, meas):
    """r [6], Ja, Jb [6, 6] in long double at the graph's poses; no corrector."""
    P = pg._ld(c.g.poses)
    r, Ja, Jb, _ = pg.residual_jacobian(P[a], P[b], meas)
    return r, Ja, Jb


def resid_cov(c, a, b, meas):
    """(r, Sigma_r, Ja, Jb, joint block), long double.  The Jacobian of a fixed node is replaced by zero."""
    r, Ja, Jb = edge_terms(c, a, b, meas)
    if c.free[a] < 0:
        Ja = np.zeros_like(Ja)
    if c.free[b] < 0:
        Jb = np.zeros_like(Jb)
    S = joint_block(c, a, b)
    J = np.concatenate([Ja, Jb], axis=1)
    M = J @ S @ J.T
    return r, (M + M.T) / 2, Ja, Jb, S


def resid_cov_brute(c, a, b, meas):
    """First-order propagation of the WHOLE covariance: J_full (6 x n) with the edge's blocks at its free nodes."""
    r, Ja, Jb = edge_terms(c, a, b, meas)
    Jf = np.zeros((6, len(c.Z)), LD)
    for node, J in ((a, Ja), (b, Jb)):
        ix = _idx(c, node)
        if ix is not None:
            Jf[:, ix] = J
    return Jf @ c.Z @ Jf.T


def chi2_ld(r, A):
    """r^T A^-1 r in long double by Cholesky; NaN when a pivot is not positive."""
    A = np.array(A, LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    y = np.zeros(n, LD)
    for j in range(n):
        d = A[j, j] - np.sum(L[j, :j] * L[j, :j])
        if not d > 0:
            return float("nan")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
        y[j] = (r[j] - np.sum(L[j, :j] * y[:j])) / L[j, j]
    return float(np.sum(y * y))


def _ring(n_nodes, **kw):
    """Node 0 fixed, a pendant of node 1; nodes 1 .. n - 1 free and closed into a ring by the edge (n - 1, 1)."""
    return pg.loop_graph(n_nodes, window=1, loop=False, fixed=[0], extra=[(n_nodes - 1, 1)], noise=2e-3, **kw)


# name -> (graph builder, use_huber, huber, expected route): the graphs of the marginal-covariance tests
GRAPHS = {
    "dense4": (lambda: pg.loop_graph(4, fixed=[0], noise=2e-3, seed=21), True, 1.0, 0),
    "chain23": (lambda: pg.loop_graph(23, window=1, loop=False, fixed=[0], noise=2e-3, seed=22), True, 1.0, 1),
    "chain30_w2_fixed_middle": (lambda: pg.loop_graph(30, window=2, loop=False, fixed=[15], noise=2e-3, seed=23), True, 1.0, 1),
    "ring25_even": (lambda: _ring(25, seed=24), True, 1.0, 2),
    "ring26_odd": (lambda: _ring(26, seed=25), True, 1.0, 2),
    "ring26_outliers_huber_on": (lambda: _ring(26, seed=26, outliers=5), True, 0.5, 2),
}


@functools.lru_cache(maxsize=None)
def case(name):
    build, on, h, route = GRAPHS[name]
    c = make_case(build(), on, h)
    c.route = route
    c.name = name
    return c


def pairs_of(name):
    """The queried pairs of a graph (node ids): adjacent nodes; the two ends / opposite sides; a pair with free index 5
    (unknowns 30..35 straddle the 32-column panel boundary); pairs with the fixed node, either way round; the last free
    node; on the window-2 chain (half bandwidth 17) the node distances 2 (6 d + 5 = 17: read) and 3 (partly inside the
    band: solved)."""
    c = case(name)
    free = [int(x) for x in np.flatnonzero(c.g.node_fixed == 0)]
    fixed = int(np.flatnonzero(c.g.node_fixed)[0])
    nf = len(free)
    if nf < 6:
        return [(free[0], free[1]), (free[2], free[0]), (fixed, free[1]), (free[2], fixed), (free[-1], free[1])]
    out = [(free[1], free[2]), (free[0], free[-1]), (free[0], free[nf // 2]), (free[5], free[-2]), (free[nf // 2 + 3], free[5]),
           (fixed, free[1]), (free[nf // 2], fixed), (free[-1], free[nf // 3]), (free[-2], free[-1])]
    if name == "chain30_w2_fixed_middle":
        out += [(3, 5), (3, 6), (14, 17), (14, 18), (29, 26)]   # 14 | 17, 18: free indices 14 | 16, 17 across the fixed node
    return out
