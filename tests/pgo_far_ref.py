"""TEST INFRASTRUCTURE: long-double restatement of the pose graph's far-edge route (pgo.hip "FAR EDGES", DESIGN.md
section 25) on the normal equations of pgo_weighted_ref.linearize (pgo_ref.linearize's H when the weights are identity).
numpy only; imports neither the package nor the oracle.

  split     d_e = |f_a - f_b| in free indices (0 with one endpoint fixed, -1 with both); far = d_e > d*
  identity  H = M + W W^T with M the near edges' J^T J and W six columns per far edge (the rows of [Ja Jb] of the
            whitened, robustified edge at its endpoints' unknowns);  y = M^-1 b, Y = M^-1 W, C = I + W^T Y,
            C z = W^T y, x = y - Y z
  solves    double LU refined on the long-double residual (pgo_weighted_ref.columns_of_inverse's scheme)
  bar       64 cond_2(H) 2^-52 max|x|, cond_2 from the eigenvalues of the long-double H rounded to double
"""
import numpy as np

import pgo_ref as pg
import pgo_weighted_ref as wr

LD = pg.LD
MAX_FAR = 128


def ld_solve(A_ld, B_ld, rounds=4):
    """A^-1 B in long double: double LU solves refined on the long-double residual."""
    A64 = np.asarray(A_ld, np.float64)
    B_ld = pg._ld(B_ld)
    X = pg._ld(np.linalg.solve(A64, B_ld.astype(np.float64)))
    for _ in range(rounds):
        X = X + pg._ld(np.linalg.solve(A64, (B_ld - A_ld @ X).astype(np.float64)))
    return X


def distances(g):
    free = g.free_index()
    fa, fb = free[g.edge_a], free[g.edge_b]
    return np.where((fa < 0) & (fb < 0), -1, np.where((fa < 0) | (fb < 0), 0, np.abs(fa - fb)))


def far_mask(g, d_star):
    return distances(g) > d_star


def model_flops(n, bw, m):
    return float(n) * bw * bw + 4.0 * n * bw * (m + 1.0) + 24.0 * m * m + float(m) ** 3 / 3.0


def anchored(g, d_star):
    """Every component of the near graph over the free nodes has a node with an edge to a fixed node."""
    free, d = g.free_index(), distances(g)
    nf = int((g.node_fixed == 0).sum())
    comp = list(range(nf))

    def find(x):
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x
    for e in range(len(g.edge_a)):
        a, b = free[g.edge_a[e]], free[g.edge_b[e]]
        if a >= 0 and b >= 0 and d[e] <= d_star:
            comp[find(a)] = find(b)
    ok = set()
    for e in range(len(g.edge_a)):
        a, b = free[g.edge_a[e]], free[g.edge_b[e]]
        if (a < 0) != (b < 0):
            ok.add(find(max(a, b)))
    return all(find(f) in ok for f in range(nf))


def choose(g):
    """The plan's d* (None: no admissible candidate): least model cost, ties to the smaller d*."""
    d, n = distances(g), g.n_unknowns()
    best = None
    for c in sorted(set(int(x) for x in d if x >= 0)):
        k, bw = int((d > c).sum()), 6 * c + 5
        if not (1 <= k <= MAX_FAR and (bw + 33) * 2 < n and anchored(g, c)):
            continue
        cost = model_flops(n, bw, 6 * k)
        if best is None or cost < best[0]:
            best = (cost, c)
    return None if best is None else best[1]


class Ref:
    """H_ld, g_ld, far (mask), k, bw, M, W (long double), cond, x(b) by the identity, x_dense(b) by a solve with H"""

    def tol(self, x_ref):
        return 64.0 * self.cond * 2.0 ** -52 * float(np.abs(x_ref).max())

    def x(self, b=None):
        b = self.g_ld if b is None else pg._ld(b)
        if self.k == 0:
            return ld_solve(self.M, b)
        Y = ld_solve(self.M, np.concatenate([b[:, None], self.W], axis=1))
        y, YW = Y[:, 0], Y[:, 1:]
        C = np.eye(6 * self.k, dtype=LD) + self.W.T @ YW
        z = ld_solve(C, self.W.T @ y)
        return y - YW @ z

    def x_dense(self, b=None):
        return ld_solve(self.H_ld, self.g_ld if b is None else pg._ld(b))


def reference(g, d_star, info=None, use_huber=True, huber=1.0):
    E = len(g.edge_a)
    info = wr.family("identity", E) if info is None else info
    lin = wr.linearize(g, info, use_huber, huber)
    r, Ja, Jb = wr.raw_terms(g)
    U = wr.cholesky_upper(info)
    _, Jaw, Jbw, _, _ = wr.weighted_huber(U, r, Ja, Jb, use_huber, huber)
    out = Ref()
    out.lin, out.H_ld, out.g_ld = lin, lin.H_ld, lin.g_ld
    out.far = far_mask(g, d_star)
    out.k, out.bw = int(out.far.sum()), 6 * d_star + 5
    n, free = g.n_unknowns(), g.free_index()
    near = np.flatnonzero(~out.far)
    sub = pg.Graph(g.poses, g.node_fixed, g.edge_a[near], g.edge_b[near], g.edge_meas[near])
    out.M, _ = wr.assemble(sub, np.zeros((len(near), 6), LD), Jaw[near], Jbw[near])
    out.W = np.zeros((n, 6 * out.k), LD)
    for q, e in enumerate(np.flatnonzero(out.far)):
        a, b = 6 * free[g.edge_a[e]], 6 * free[g.edge_b[e]]
        out.W[a:a + 6, 6 * q:6 * q + 6] = Jaw[e].T
        out.W[b:b + 6, 6 * q:6 * q + 6] = Jbw[e].T
    lam = np.linalg.eigvalsh(np.asarray(out.H_ld, np.float64))
    out.cond = float(lam[-1] / lam[0])
    return out


# ------------------------------------------------------------------------------------------------------ shapes
NOISE = 2e-3
TWO_CHAINS_EXTRA = [(35, 5), (30, 8), (39, 1)]      # free distances 30, 22, 38: a band that holds one of them is not narrow


def two_chains():
    """Two window-1 chains of 20 nodes (0 .. 19 with node 0 fixed, 20 .. 39 all free) joined only by extra edges: at
    every d* below the extras' distances the second chain has no fixed neighbour."""
    a = pg.loop_graph(40, window=1, loop=False, fixed=[0], extra=TWO_CHAINS_EXTRA, noise=NOISE, seed=47, name="two_chains")
    keep = ~((a.edge_a == 20) & (a.edge_b == 19))
    return pg.Graph(a.poses, a.node_fixed, a.edge_a[keep], a.edge_b[keep], a.edge_meas[keep], "two_chains")


_HOOK = None


def hook_cases():
    """name -> (graph, edge_info or None, use_huber, huber, max_near_distance, expected far edges): the shapes of the hook
    tests of tests/test_pgo_far_gpu.py, built once."""
    global _HOOK
    if _HOOK is None:
        C = {}
        C["k1_chain23"] = (pg.loop_graph(23, window=2, loop=False, fixed=[0], extra=[(20, 3)], noise=NOISE, seed=41,
                                         name="k1_chain23"), None, True, 1.0, 2, 1)
        # (30, 20): one endpoint fixed -- near at every d*
        C["block_boundary44"] = (pg.loop_graph(44, window=2, loop=False, fixed=[20], extra=[(33, 5), (40, 5), (12, 38), (30, 20)],
                                               noise=NOISE, seed=42, name="block_boundary44"), None, True, 1.0, 2, 3)
        g = pg.loop_graph(60, window=2, loop=False, fixed=[0], extra=[(50, 4), (33, 9), (58, 20), (41, 2), (27, 12)], noise=NOISE,
                          seed=43, outliers=2, name="weighted60")
        W = wr.family("random", len(g.edge_a), seed=5)
        thr = wr.huber_threshold(wr.linearize(g, W, False, 1.0).norms)
        C["weighted60"] = (g, W, True, thr, 2, 5)
        C["k0_chain30"] = (pg.loop_graph(30, window=3, loop=False, fixed=[0], noise=NOISE, seed=44, name="k0_chain30"),
                           None, True, 1.0, 3, 0)
        _HOOK = C
    return _HOOK


def rhs(n, seed=3):
    return np.random.default_rng(seed).normal(size=n)


_REFS = {}


def hook_reference(name):
    if name not in _REFS:
        g, W, hub, thr, d, _ = hook_cases()[name]
        _REFS[name] = reference(g, d, W, hub, thr)
    return _REFS[name]


# LM cases (the switch): name -> (graph, expected far edges, expected half bandwidth).  Seeds: see DESIGN.md section 25.
_LM = None


def _spread_extra(n_nodes, count, seed):
    """`count` far pairs (a, b), a - b >= n_nodes / 4, both away from the ends"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        b = int(rng.integers(2, n_nodes // 2))
        a = int(rng.integers(b + n_nodes // 4, n_nodes - 2))
        out.append((a, b))
    return out


def lm_cases():
    global _LM
    if _LM is None:
        C = {}
        # the three edges across the seam and the long edge (33, 5) are far at d* = 2
        C["ring44_w2_long_edge"] = (pg.topologies()["ring44_w2_long_edge"][0], 4, 17)
        C["chain150_w3_far4"] = (pg.loop_graph(150, window=3, loop=False, fixed=[0], extra=_spread_extra(150, 4, 1), noise=NOISE,
                                               seed=45, name="chain150_w3_far4"), 4, 23)
        C["chain400_w2_far12"] = (pg.loop_graph(400, window=2, loop=False, fixed=[0], extra=_spread_extra(400, 12, 2), noise=NOISE,
                                                seed=46, name="chain400_w2_far12"), 12, 17)
        _LM = C
    return _LM
