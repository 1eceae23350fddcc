"""TEST INFRASTRUCTURE: long-double reference of the matrix-free PCG on the reduced camera system (ba_pcg.h, driven from
ba_session.hip), in the style of ba_ref.py, on which it builds (Problem, scene_problem, reference, ratio, the per-observation
blocks and the Huber corrector).  numpy only, np.longdouble throughout; imports neither the package nor the oracle.

  system(name, inv_radius)   S, g and the entrywise magnitudes A_S, A_g (ba_ref.py "reduction") of the plain system
              (inv_radius None) or of the Jacobi-scaled, damped one in ba_ref's "fused form" variables.  For the cases of
              ba_ref's own table this IS ba_ref.reference(); the new cases are reduced landmark by landmark without the
              dense H of ba_ref.linearize (3300 landmarks would be a 10^7-entry matrix); test_ba_pcg_ref_cpu.py holds the
              two against each other on a case both can do.
  the session's rule   read in ba_session.hip / ba_large.h: sess_scale_kernel sets D = 1 / (1 + sqrt(diag H)) from the
              UNSCALED column norms of cameras (diag of the blocks H_c) and landmarks (n2l); bal_prep_kernel damps a
              landmark block by clamp(diag P, 1e-6, 1e32) / radius on the SCALED P; sess_damp_kernel keeps
              clamp(diag H_c, 1e-6, 1e32) of the SCALED camera blocks and the product / the preconditioner add it times
              1 / radius (bpcg_q_of, bpcg_precond_kernel).  That is ba_ref's fused form term by term (scale from the plain
              diagonal, clamp on the scaled one, cameras and landmarks alike), so nothing is re-implemented differently.
  x_ref, cond, blocks   x_ref = S^-1 b by long-double Cholesky; cond_2(S); the blocks M_c = S[6c:6c+6, 6c:6c+6] with M_c^-1
              (long double) and cond_2(M_c).  The blocks are computed in square-root form (sqrt_blocks: no P_l inverted,
              nothing subtracted), because cut out of the normal-equations S they are noise exactly where their condition
              number matters: at 1 / radius = 0 the pair1mm blocks came out with a smallest eigenvalue of +-1e-10,
              negative for three camera models and positive for the fourth.  test_ba_pcg_ref_cpu.py holds the two forms
              against each other.
  pcg(S, b, tol, max_it)   the algorithm of ba_pcg.h in long double: block-Jacobi preconditioner from the true diagonal
              blocks, recurrence residual, the record's stopping rule in its order (||r||^2 <= tol^2 ||b||^2, then the cap,
              then rho > 0; p.Sp > 0 before the division).  Returns every iterate.
  components  many/1040 is a block-diagonal union of independent windows: each is linearised on its own and the System
              applies / solves component by component -- no dense matrix of the whole problem exists.

Cases beyond ba_ref's table (what each reaches: DESIGN.md section 22, "edge table"):
  seg/one_free, seg/empty, seg/boundaries, runs/cut, many/1040 -- see their builders below.
"""
import numpy as np

import ba_ref as ref
from ba_ref import LD, U, Problem, _cholesky_solve, _inv3, huber_correct, scene_problem
from pgo_ref import _ld

# the host plan's rule for the segments of a camera's observation list (ba.hip, ba_setup): clamp(O / nfree / 512, 1, 32)
BL_THREADS, BL_LMW = 512, 256


def nseg_rule(prob):
    return int(max(1, min(32, len(prob.obs_cam) // max(1, prob.n_free) // 512)))


def run_cuts(prob):
    """wg_lm by the rule of ba_host_plan.h: a run closes before the landmark that would take it past BL_THREADS
    observations, or at BL_LMW landmarks.  -> (cuts, why) with why[k] in {"threads", "landmarks", "both", "end"}."""
    cnt = np.bincount(prob.obs_lm, minlength=len(prob.points))
    start = np.concatenate([[0], np.cumsum(cnt)])
    cuts, why, a = [0], [], 0
    for l in range(len(cnt)):
        t, m = start[l + 1] - start[a] > BL_THREADS, l - a == BL_LMW
        if t or m:
            cuts.append(l)
            why.append("both" if t and m else ("threads" if t else "landmarks"))
            a = l
    cuts.append(len(cnt))
    why.append("end")
    return cuts, why


# ----------------------------------------------------------------------------------------------------------- cases
def _keep(p, mask):
    return ref._drop(p, mask)


def _seg_one_free():
    """2 fixed + 1 free camera, 1100 landmarks seen by all three: 3300 observations over ONE free camera, 6 segments;
    the preconditioner block is S itself."""
    return scene_problem(3, 2, 1100, 900)


def _seg_empty():
    """30 fixed cameras see all 1100 landmarks, the two free cameras 40 each (landmarks 0 .. 39 and 20 .. 59): the host plan
    takes 32 segments from the TOTAL observation count, and a free camera's 40 observations all fall into segment 0."""
    p = scene_problem(32, 30, 1100, 901)
    lo = np.where(p.obs_cam == 31, 20, 0)
    return _keep(p, (p.obs_cam < 30) | ((p.obs_lm >= lo) & (p.obs_lm < lo + 40)))


SEG_BOUNDARY_COUNTS = (255, 256, 257, 511, 512, 513)


def _seg_boundaries():
    """8 fixed cameras see all 520 landmarks; free camera j sees the first SEG_BOUNDARY_COUNTS[j]: two segments, strides of
    256 threads -- counts on both sides of one trip, of the second segment's end and of the second trip."""
    p = scene_problem(14, 8, 520, 902)
    cnt = np.concatenate([np.full(8, 520), SEG_BOUNDARY_COUNTS])
    return _keep(p, p.obs_lm < cnt[p.obs_cam])


RUNS_UNOBSERVED = (100, 255)


def _runs_cut():
    """32 cameras (2 fixed).  Landmarks 0 .. 255: 254 with two observations and two with none -- 508 observations, so the
    run closes at BL_LMW landmarks and NOT at BL_THREADS; 256 .. 301: 46 more with two observations; 302 .. 321: 20 landmarks
    seen by 30 cameras -- the second run takes 14 of them (92 + 420 = 512 observations exactly) and closes at BL_THREADS."""
    L = 322
    p = scene_problem(32, 2, L, 903)
    c, l = p.obs_cam, p.obs_lm
    a = 2 + l % 30                                      # a light landmark: free camera a and the one 8 further on
    light = (c == a) | (c == 2 + (l % 30 + 8) % 30)
    heavy = c <= 29                                     # a heavy landmark: 30 cameras, the two fixed ones among them
    keep = np.where(l >= 302, heavy, light) & ~np.isin(l, RUNS_UNOBSERVED)
    return _keep(p, keep)


MANY_SIZES = (4,) + (8,) * 129 + (4,)      # free cameras per window: 1040 in all, a window straddles free index 1024


def _many():
    """131 different windows (seeds 1000 ..), 2 fixed cameras each, everything sees its window's 12 landmarks; camera, landmark
    and observation arrays concatenated.  p.components = [(Problem, first free index, first camera, first landmark)]."""
    comps, off_f, off_c, off_l = [], 0, 0, 0
    for k, nf in enumerate(MANY_SIZES):
        q = scene_problem(nf + 2, 2, 12, 1000 + k, name="many/1040[%d]" % k)
        comps.append((q, off_f, off_c, off_l))
        off_f, off_c, off_l = off_f + nf, off_c + nf + 2, off_l + 12
    cat = lambda f: np.concatenate([f(q, oc, ol) for q, _, oc, ol in comps])
    p = Problem(cat(lambda q, oc, ol: q.poses), cat(lambda q, oc, ol: q.cam_fixed), cat(lambda q, oc, ol: q.cam_intr), comps[0][0].intr,
                cat(lambda q, oc, ol: q.points), cat(lambda q, oc, ol: q.obs_cam + oc), cat(lambda q, oc, ol: q.obs_lm + ol),
                cat(lambda q, oc, ol: q.obs_uv), comps[0][0].cam_model)
    p.components = comps
    return p


NEW = {"seg/one_free": _seg_one_free, "seg/empty": _seg_empty, "seg/boundaries": _seg_boundaries, "runs/cut": _runs_cut,
       "many/1040": _many}
# the cases of ba_ref's table: every one with 0 < 6 n_free <= 126, and structure/n22
TABLE = sorted(n for n, p in ref.cases().items() if 0 < 6 * p.n_free <= 126) + ["structure/n22"]
NAMES = TABLE + list(NEW)
# solvable undamped (64 cond(S) 2^-52 < 1e-3): the windows with two fixed cameras -- the rest leave the scale free
# (test_ba_edges_gpu.py DC_UNDAMPED, plus structure/cams65, structure/n22 and the new cases: at least two fixed cameras each)
SOLVABLE_UNDAMPED = ("structure/cams64", "structure/cams65", "structure/fixed_only_and_unobserved", "structure/n1", "structure/n8", "structure/n16",
                     "structure/n21", "structure/n22") + tuple(NEW)

_CASES = None


def cases():
    """name -> ba_ref.Problem, built once."""
    global _CASES
    if _CASES is None:
        C = {n: ref.cases()[n] for n in TABLE}
        for n, f in NEW.items():
            C[n] = f()
            C[n].name = n
        _CASES = C
    return _CASES


# ----------------------------------------------------------------------------------- reduction without a dense H
def reduce_sparse(prob, inv_radius=None):
    """ba_ref.linearize's S, g, A_S, A_g, D (cameras), cost for a problem of any size: camera blocks and landmark blocks
    summed from the observations, the landmarks eliminated one by one on the rows of the cameras that see them."""
    out = ref.Lin()
    nf, L = prob.n_free, len(prob.points)
    nc = 6 * nf
    out.r, out.F, out.E, _ = prob.blocks()
    r, F, E, cost, _ = huber_correct(out.r, out.F, out.E, prob.use_huber, prob.huber)
    out.cost = float(np.sum(cost))
    fc = prob.free_index()[prob.obs_cam]
    lm = prob.obs_lm
    isf = fc >= 0
    hc, hl = np.zeros((nf, 6), LD), np.zeros((L, 3), LD)
    np.add.at(hc, fc[isf], np.sum(F[isf] ** 2, axis=1))
    np.add.at(hl, lm, np.sum(E ** 2, axis=1))
    Pplain = np.zeros((L, 3, 3), LD)
    np.add.at(Pplain, lm, np.einsum("oia,oib->oab", E, E))
    Dc, Dl = np.ones((nf, 6), LD), np.ones((L, 3), LD)
    damp_c, damp_l = np.zeros((nf, 6), LD), np.zeros((L, 3), LD)
    if inv_radius is not None:
        Dc, Dl = 1 / (1 + np.sqrt(hc)), 1 / (1 + np.sqrt(hl))
        damp_c = np.clip(Dc * hc * Dc, LD(1e-6), LD(1e32)) * LD(inv_radius)
        damp_l = np.clip(Dl * hl * Dl, LD(1e-6), LD(1e32)) * LD(inv_radius)
    Fs = F * Dc[np.where(isf, fc, 0)][:, None, :] * isf[:, None, None]
    Es = E * Dl[lm][:, None, :]
    S, A_S, g, A_g = np.zeros((nc, nc), LD), np.zeros((nc, nc), LD), np.zeros(nc, LD), np.zeros(nc, LD)
    Hb, Ab = np.zeros((nf, 6, 6), LD), np.zeros((nf, 6, 6), LD)
    gb, ab = np.zeros((nf, 6), LD), np.zeros((nf, 6), LD)
    np.add.at(Hb, fc[isf], np.einsum("oia,oib->oab", Fs[isf], Fs[isf]))
    np.add.at(Ab, fc[isf], np.einsum("oia,oib->oab", np.abs(Fs[isf]), np.abs(Fs[isf])))
    np.add.at(gb, fc[isf], np.einsum("oia,oi->oa", Fs[isf], r[isf]))
    np.add.at(ab, fc[isf], np.einsum("oia,oi->oa", np.abs(Fs[isf]), np.abs(r[isf])))
    for c in range(nf):
        s = slice(6 * c, 6 * c + 6)
        S[s, s], A_S[s, s], g[s], A_g[s] = Hb[c] + np.diag(damp_c[c]), Ab[c] + np.diag(damp_c[c]), gb[c], ab[c]
    P = np.zeros((L, 3, 3), LD)
    np.add.at(P, lm, np.einsum("oia,oib->oab", Es, Es))
    bl = np.zeros((L, 3), LD)
    np.add.at(bl, lm, np.einsum("oia,oi->oa", Es, r))
    W = np.einsum("oia,oib->oab", Fs, Es)                 # [O, 6, 3], zero for a fixed camera's observation
    order = np.argsort(lm, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(lm, minlength=L))])
    out.kappa = np.zeros(L)
    for l in range(L):
        idx = order[start[l]:start[l + 1]]
        Pl = P[l] + np.diag(damp_l[l])
        if len(idx) == 0 and not np.any(Pl):
            continue
        idx = idx[isf[idx]]
        if len(idx) == 0:
            continue
        Pi = _inv3(Pl)
        cams = np.unique(fc[idx])
        Wk = np.zeros((len(cams), 6, 3), LD)
        np.add.at(Wk, np.searchsorted(cams, fc[idx]), W[idx])
        Wk = Wk.reshape(-1, 3)
        if not np.any(Wk):
            continue
        rows = (6 * cams[:, None] + np.arange(6)[None, :]).reshape(-1)
        k = out.kappa[l] = np.linalg.cond(Pplain[l].astype(np.float64))
        ix = np.ix_(rows, rows)
        S[ix] -= Wk @ Pi @ Wk.T
        g[rows] -= Wk @ Pi @ bl[l]
        A_S[ix] += LD(k) * (np.abs(Wk) @ np.abs(Pi) @ np.abs(Wk).T)
        A_g[rows] += LD(k) * (np.abs(Wk) @ np.abs(Pi) @ np.abs(bl[l]))
    out.S, out.g, out.A_S, out.A_g, out.D = S, g, A_S, A_g, Dc.reshape(-1)
    return out


def _orthonormal(A):
    """Orthonormal basis of the columns of A [m, 3] (modified Gram-Schmidt, every projection twice); a column that
    vanishes against the earlier ones is dropped."""
    Q = []
    for j in range(A.shape[1]):
        v = A[:, j].copy()
        n0 = np.sqrt(v @ v)
        for _ in range(2):
            for q in Q:
                v = v - (q @ v) * q
        nv = np.sqrt(v @ v)
        if nv > 0 and nv > LD(2.0) ** -60 * n0:
            Q.append(v / nv)
    return Q


def sqrt_blocks(prob, lin, inv_radius=None):
    """The diagonal blocks M_c of S [n_free, 6, 6] in SQUARE-ROOT form, from the raw blocks lin.r / F / E:
      M_c = D_c + sum over the landmarks l camera c sees of G^T G,   G = (I - Q Q^T) F_l^c,
    Q an orthonormal basis of the landmark's stacked E blocks (all its observations, plus the rows sqrt(damping) I) and
    F_l^c camera c's F blocks in the same rows.  That IS H_c - W P^-1 W^T restricted to the block (F^T (I - A (A^T A)^-1 A^T) F),
    but no P_l is inverted and nothing is subtracted from H_c: the error is sqrt(cond P_l) 2^-63 relative to |F| in G, where
    the normal-equations form of ba_ref.linearize loses cond(P_l) 2^-63 of |W P^-1 W^T| -- for cameras 1 mm apart seeing
    points 1e3 away (cond P_l ~ 1e12, the pair1mm cases) that is 1e-7 of terms of size 1 against a smallest eigenvalue of
    M_c of 1e-10.  A sum of Gram matrices: positive semi-definite by construction."""
    nf, L = prob.n_free, len(prob.points)
    r, F, E, _, _ = huber_correct(lin.r, lin.F, lin.E, prob.use_huber, prob.huber)
    fc = prob.free_index()[prob.obs_cam]
    lm = prob.obs_lm
    isf = fc >= 0
    hc, hl = np.zeros((nf, 6), LD), np.zeros((L, 3), LD)
    np.add.at(hc, fc[isf], np.sum(F[isf] ** 2, axis=1))
    np.add.at(hl, lm, np.sum(E ** 2, axis=1))
    Dc, Dl = np.ones((nf, 6), LD), np.ones((L, 3), LD)
    damp_c, damp_l = np.zeros((nf, 6), LD), np.zeros((L, 3), LD)
    if inv_radius is not None:
        Dc, Dl = 1 / (1 + np.sqrt(hc)), 1 / (1 + np.sqrt(hl))
        damp_c = np.clip(Dc * hc * Dc, LD(1e-6), LD(1e32)) * LD(inv_radius)
        damp_l = np.clip(Dl * hl * Dl, LD(1e-6), LD(1e32)) * LD(inv_radius)
    Fs = F * Dc[np.where(isf, fc, 0)][:, None, :]
    Es = E * Dl[lm][:, None, :]
    M = np.stack([np.diag(damp_c[c]) for c in range(nf)]) if nf else np.zeros((0, 6, 6), LD)
    order = np.argsort(lm, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(lm, minlength=L))])
    for l in range(L):
        idx = order[start[l]:start[l + 1]]
        if not isf[idx].any():
            continue
        k = len(idx)
        A = np.concatenate([Es[idx].reshape(2 * k, 3), np.diag(np.sqrt(damp_l[l]))])
        Q = _orthonormal(A)
        for c in np.unique(fc[idx][isf[idx]]):
            G = np.zeros((2 * k + 3, 6), LD)
            for j in np.flatnonzero(fc[idx] == c):
                G[2 * j:2 * j + 2] = Fs[idx[j]]
            for _ in range(2):
                for q in Q:
                    G = G - np.outer(q, q @ G)
            M[c] += G.T @ G
    return M


# ------------------------------------------------------------------------------------------------------- the system
class Component:
    def __init__(self, lin, n, off, prob=None, inv_radius=None):
        self.S, self.g, self.A_S, self.A_g = lin.S, lin.g, lin.A_S, lin.A_g
        self.D, self.cost, self.n, self.off = lin.D[:n], lin.cost, n, off
        self._lin, self._prob, self._ir, self._M = lin, prob, inv_radius, None

    def M(self):
        """The diagonal blocks: square-root form where the problem is known, else cut out of S."""
        if self._M is None:
            if self._prob is not None:
                self._M = sqrt_blocks(self._prob, self._lin, self._ir)
            else:
                self._M = np.stack([self.S[k:k + 6, k:k + 6] for k in range(0, self.n, 6)])
        return self._M


class System:
    """The reduced camera system of a case as a list of independent components (one, but for many/1040).  Vectors are
    long double of length n; nothing dense of size n x n is formed unless there is one component (then .S is it)."""

    def __init__(self, comps):
        self.comps = comps
        self.n = sum(c.n for c in comps)
        self.cost = sum(c.cost for c in comps)
        self._cache = {}

    def _each(self, f, *vecs):
        out = np.zeros(self.n, LD)
        for c in self.comps:
            s = slice(c.off, c.off + c.n)
            out[s] = f(c, *[_ld(v)[s] for v in vecs])
        return out

    @property
    def S(self):
        assert len(self.comps) == 1
        return self.comps[0].S

    @property
    def g(self):
        return self._each(lambda c: c.g)

    @property
    def A_g(self):
        return self._each(lambda c: c.A_g)

    @property
    def D(self):
        return self._each(lambda c: c.D)

    def apply(self, x):
        return self._each(lambda c, v: c.S @ v, x)

    def abs_apply(self, x):
        """A_S |x|: the magnitude the product's rounding is measured in."""
        return self._each(lambda c, v: c.A_S @ np.abs(v), x)

    def row_nnz(self):
        """m_i: non-zeros in row i of S."""
        return self._each(lambda c: np.count_nonzero(c.S, axis=1).astype(LD)).astype(np.float64)

    def solve(self, b):
        """S^-1 b by long-double Cholesky, component by component; None where S is not positive definite."""
        parts = [_cholesky_solve(c.S, _ld(b)[c.off:c.off + c.n]) for c in self.comps]
        return None if any(p is None for p in parts) else np.concatenate(parts)

    def cond(self):
        """cond_2(S) (float64 singular values of each component)."""
        if "cond" not in self._cache:
            sv = np.concatenate([np.linalg.svd(c.S.astype(np.float64), compute_uv=False) for c in self.comps])
            self._cache["cond"] = float(sv.max() / sv.min()) if sv.min() > 0 else float("inf")
        return self._cache["cond"]

    def blocks(self):
        """M [n/6, 6, 6] (sqrt_blocks: the square-root form), M^-1 (long double), cond_2(M) [n/6]; a block that is not
        positive definite in long double (a camera whose own six unknowns are not determined without damping) has
        M^-1 = NaN and cond = inf."""
        if "blocks" not in self._cache:
            M = np.concatenate([c.M() for c in self.comps])
            Mi = np.stack([inv_spd(m) for m in M])
            kM = np.array([np.linalg.cond(m.astype(np.float64)) if np.isfinite(mi).all() else np.inf for m, mi in zip(M, Mi)])
            self._cache["blocks"] = (M, Mi, kM)
        return self._cache["blocks"]

    def minv(self, r):
        Mi = self.blocks()[1]
        return np.einsum("cab,cb->ca", Mi, _ld(r).reshape(-1, 6)).reshape(-1)


def inv_spd(M):
    """M^-1 in long double by Cholesky solves of the unit vectors."""
    n = len(M)
    cols = [_cholesky_solve(M, np.eye(n, dtype=LD)[j]) for j in range(n)]
    if any(c is None for c in cols):
        return np.full((n, n), np.nan, LD)
    X = np.stack(cols, axis=1)
    return (X + X.T) / 2


_SYS = {}


def system(name, inv_radius=None):
    """The System of a case: plain (inv_radius None) or scaled and damped (a number; 0 = scaled, no damping term).
    Computed once and shared: treat it as read-only."""
    key = (name, inv_radius)
    if key not in _SYS:
        p = cases()[name]
        if name in TABLE:
            comps = [Component(ref.reference(name, inv_radius), 6 * p.n_free, 0, p, inv_radius)]
        elif hasattr(p, "components"):
            comps = [Component(ref.linearize(q, inv_radius), 6 * q.n_free, 6 * off_f, q, inv_radius) for q, off_f, _, _ in p.components]
        else:
            comps = [Component(reduce_sparse(p, inv_radius), 6 * p.n_free, 0, p, inv_radius)]
        _SYS[key] = System(comps)
    return _SYS[key]


# ------------------------------------------------------------------------------------------------------- the solver
RUNNING, CONVERGED, NUMERIC, CAP = 0, 1, 2, 3


class _Dense:
    def __init__(self, S):
        S = _ld(S)
        self.sys = System([Component(_as_lin(S), len(S), 0)])

    def __getattr__(self, k):
        return getattr(self.sys, k)


def _as_lin(S):
    lin = ref.Lin()
    lin.S, lin.g, lin.A_S, lin.A_g, lin.D, lin.cost = S, np.zeros(len(S), LD), np.abs(S), np.zeros(len(S), LD), np.ones(len(S), LD), 0.0
    return lin


def pcg(S, b, tol, max_it):
    """ba_pcg.h in long double.  S: a System or a dense matrix.  Returns a dict: xs (the iterates x_1 ..), alphas, betas,
    rels (||r_k|| / ||b|| of the recurrence), iterations, status, x (the last iterate, zeros at iteration 0)."""
    A = S if hasattr(S, "apply") else _Dense(S)
    b = _ld(b)
    tol2 = LD(tol) * LD(tol)
    x, r = np.zeros(len(b), LD), b.copy()
    z = A.minv(r)
    p = z.copy()
    rho, bb = r @ z, b @ b
    out = dict(xs=[], alphas=[], betas=[], rels=[], iterations=0, status=RUNNING, x=x)
    if bb <= tol2 * bb:
        out["status"] = CONVERGED
    elif max_it <= 0:
        out["status"] = CAP
    elif not rho > 0:
        out["status"] = NUMERIC
    it = 0
    while out["status"] == RUNNING:
        q = A.apply(p)
        pq = p @ q
        if not pq > 0:
            out["status"] = NUMERIC
            break
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        z = A.minv(r)
        rz, rr = r @ z, r @ r
        beta = rz / rho
        p = z + beta * p
        rho = rz
        it += 1
        out["xs"].append(x)
        out["alphas"].append(alpha)
        out["betas"].append(beta)
        out["rels"].append(float(np.sqrt(rr / bb)))
        if rr <= tol2 * bb:
            out["status"] = CONVERGED
        elif it >= max_it:
            out["status"] = CAP
        elif not rz > 0:
            out["status"] = NUMERIC
    out["iterations"], out["x"] = it, x
    return out


# ------------------------------------------------------------------------------------------- bars of the second iterate
def second_iterate_bars(A, b):
    """The bars of the SECOND iterate, first order, every factor from the long-double reference (norms are 2-norms, e_M,
    e_P, c_b, c_p, bar_alpha as in test_ba_pcg_edges_gpu.py test_first_iterate; p_0 = z_0 = M^-1 b, rho_0 = b . z_0).  What the device carries
    into iteration 2, each an ABSOLUTE error:
      d_r1  = (bar_alpha + e_M + e_Pn) ||alpha_1 S z_0|| + 4 U ||b||     r_1 = b - alpha_1 (S z_0): the errors of alpha_1, of z_0 and
                                                                         of the product (e_Pn = ||(K_GPU + m) U A_S |z_0||| / ||S z_0||)
                                                                         are errors of the subtrahend
      d_z1  = ||M^-1|| d_r1 + e_M ||z_1||                                z_1 = M^-1 r_1, ||M^-1|| = max_c ||M_c^-1||_2
      d_rho = d_r1 ||z_1|| + ||r_1|| d_z1                                rho_1 = r_1 . z_1
      e_beta = d_rho / rho_1 + c_b e_M + 8 U                             beta_1 = rho_1 / rho_0, relative
      d_p1  = d_z1 + beta_1 (e_beta + e_M) ||p_0||                       p_1 = z_1 + beta_1 p_0
      d_q1  = ||S|| d_p1 + ||(K_GPU + m) U A_S |p_1|||                   q_1 = S p_1: the product of a perturbed vector, plus
                                                                         the product bound itself (the propagation)
      d_pq  = d_p1 ||q_1|| + ||p_1|| d_q1                                p_1 . q_1
    and the bars, relative:
      bar_alpha2 = d_rho / rho_1 + d_pq / (p_1 . q_1) + 8 U              alpha_2 = rho_1 / (p_1 . q_1)
      bar_x2     = ((bar_alpha + e_M) ||x_1|| + bar_alpha2 alpha_2 ||p_1|| + alpha_2 d_p1) / ||x_2||      x_2 = x_1 + alpha_2 p_1
    These are worst-case bounds: the rule e_M = 64 cond(M) U enters through z_0 into alpha_1 and r_1 and is amplified once
    more by ||M^-1|| on the way to z_1, so they come out at 64 c_p cond(M)^2 U ~ 1e-4 .. 1e-1 where the device's error is
    ~1e-12.  What they must still do is tell the recurrence from a wrong one, so their reach is measured, in the reference,
    against the nearest wrong recurrence: beta_1 = 0 (p_1 = z_1, the steepest-descent step), which moves alpha_2 by sens_alpha
    and x_2 by sens_x relative.  The bars are applied where each is below a tenth of that sensitivity (a dropped or
    mis-scaled beta then misses by ten bars) and below 0.1 (first-order analysis).
    Returns None where the reference itself does not run two iterations."""
    P = pcg(A, b, 0.0, 2)
    if P["status"] != CAP or P["iterations"] != 2 or not np.isfinite(A.cond()):
        return None
    nrm = lambda v: float(np.sqrt(np.sum(LD(1) * v * v)))
    bl = LD(1) * b
    M, Mi, kM = A.blocks()
    z0 = A.minv(bl)
    Sz0 = A.apply(z0)
    e_M = 64 * kM.max() * U
    w = (ref.K_GPU + A.row_nnz()) * U
    e_P = float(np.abs(z0) @ (w * A.abs_apply(z0)) / (z0 @ Sz0))
    c_b, c_p = nrm(bl) * nrm(z0) / float(bl @ z0), nrm(z0) * nrm(Sz0) / float(z0 @ Sz0)
    bar_a = (c_b + 2 * c_p) * e_M + e_P + 8 * U
    e_Pn = nrm(w * A.abs_apply(z0)) / nrm(Sz0)
    a1, b1, a2 = P["alphas"][0], P["betas"][0], P["alphas"][1]
    r1 = bl - a1 * Sz0
    z1 = A.minv(r1)
    rho1 = float(r1 @ z1)
    p1 = z1 + b1 * z0
    q1 = A.apply(p1)
    norm_Mi = max(float(np.linalg.norm(m.astype(np.float64), 2)) for m in Mi)
    norm_S = max(float(np.linalg.norm(c.S.astype(np.float64), 2)) for c in A.comps)
    d_r1 = (bar_a + e_M + e_Pn) * nrm(a1 * Sz0) + 4 * U * nrm(bl)
    d_z1 = norm_Mi * d_r1 + e_M * nrm(z1)
    d_rho = d_r1 * nrm(z1) + nrm(r1) * d_z1
    e_beta = d_rho / rho1 + c_b * e_M + 8 * U
    d_p1 = d_z1 + float(b1) * (e_beta + e_M) * nrm(z0)
    d_q1 = norm_S * d_p1 + nrm(w * A.abs_apply(p1))
    d_pq = d_p1 * nrm(q1) + nrm(p1) * d_q1
    bar_a2 = d_rho / rho1 + d_pq / float(p1 @ q1) + 8 * U
    bar_x2 = ((bar_a + e_M) * nrm(P["xs"][0]) + bar_a2 * float(a2) * nrm(p1) + float(a2) * d_p1) / nrm(P["xs"][1])
    a2w = rho1 / float(z1 @ A.apply(z1))                       # the wrong recurrence: beta_1 = 0
    sens_a = abs(a2w - float(a2)) / float(a2)
    sens_x = nrm(P["xs"][0] + a2w * z1 - P["xs"][1]) / nrm(P["xs"][1])
    applies = bar_a2 < min(0.1 * sens_a, 0.1) and bar_x2 < min(0.1 * sens_x, 0.1)
    return dict(P=P, bar_alpha2=bar_a2, bar_x2=bar_x2, e_P=e_P, sens_alpha=sens_a, sens_x=sens_x, applies=applies)


# the cases at which the bars of second_iterate_bars apply at 1 / radius 0 or 1e-4 (computed: second_iterate_cases();
# test_ba_pcg_ref_cpu.py holds the two together).  Not among them: one free camera (M = S, r_1 is rounding: no second
# iterate), the pair1mm family (the product itself is unresolved) and the cases whose worst-case bars exceed a tenth of
# the sensitivity to beta_1 = 0.
SECOND_ITERATE_CASES = (
    'huber/off', 'huber/on', 'obs/ds/axis', 'obs/ds/depth0.1', 'obs/ds/far1e3', 'obs/ds/rot_identity', 'obs/eucm/axis',
    'obs/eucm/ratio1e-12', 'obs/eucm/ratio1e-4', 'obs/eucm/ratio1e-8', 'obs/eucm/rot_identity', 'obs/kb4/axis',
    'obs/kb4/ratio1e-12', 'obs/kb4/ratio1e-4', 'obs/kb4/ratio1e-8', 'obs/pinhole/axis', 'obs/pinhole/ratio1e-12',
    'obs/pinhole/ratio1e-4', 'obs/pinhole/ratio1e-8', 'obs/pinhole/rot_qw0', 'structure/fixed_only_and_unobserved',
    'structure/n16', 'structure/n8', 'structure/observed_30_times', 'structure/observed_twice', 'structure/one_landmark',
    'structure/ragged_chunk', 'seg/empty', 'seg/boundaries', 'many/1040')
# the cases whose preconditioner blocks are singular without a damping term: two free cameras 1 mm apart and no fixed one;
# a single landmark (two equations per camera)
SINGULAR_UNDAMPED = ('obs/ds/pair1mm', 'obs/eucm/pair1mm', 'obs/kb4/pair1mm', 'obs/pinhole/pair1mm', 'structure/one_landmark')


def second_iterate_cases():
    out = []
    for name in NAMES:
        for ir in (0.0, 1e-4):
            A = system(name, ir)
            B = second_iterate_bars(A, A.g.astype(np.float64))
            if B is not None and B["applies"]:
                out.append(name)
                break
    return tuple(out)
