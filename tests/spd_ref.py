"""TEST INFRASTRUCTURE: ill-conditioned band systems, a long-double reference solve and CPU models of the elimination
orders of visual-slam_amd/csrc/chol.hip, in the style of pgo_ref.py.  numpy only; imports neither the package nor the
oracle.  Used by test_spd_ref_cpu.py (which pins everything below) and test_chol_edges_gpu.py.

  generators  chain_spd, scaled, globally_indefinite: dense row-major fp64, deterministic from a seed
  reference   solve_ld: right-looking band Cholesky + substitution in np.longdouble (the cyclic form borders the band
              with its last bw unknowns), refined with exactly formed residuals; backward_error: the normwise
              backward error with S x formed in long double from the band (or ring) only
  models      plain fp64 numpy versions of the orderings described in the header of chol.hip -- natural order with
              32-column panels and explicitly inverted diagonal factors, the two-ended order, the odd-even block order
              (linear and ring) -- written from that description, not from the kernels.  They set the tolerance only.
  cases()     the one case list of both test files

THE TOLERANCE.  For every case LAPACK (fp64) and the model of the case's path are run on the same system; the largest
ratio model / LAPACK per path, of the backward error eta and of the forward error against solve_ld, is recorded below.
A GPU solve passes when   eta <= max(4 x ratio x eta_LAPACK, 4 u)   and   fwd <= 4 x ratio x fwd_LAPACK,   LAPACK run on
the same system inside the GPU test.  The 4 covers what a path leaves open: tile summation order and the fma
contraction setting of csrc/Makefile.  A ratio is never taken below 1 (a path is not asked to beat LAPACK because its
model happened to) and never above RATIO_CAP.
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53                       # unit roundoff of fp64
EPS_LD = float(np.finfo(LD).eps)
LD_OK = EPS_LD < 2e-19                 # 64-bit significand (x86-64); the tests that need the reference skip otherwise
LD_SKIP_REASON = "np.longdouble has eps %.1e here, the reference needs eps < 2e-19" % EPS_LD
NB = 32                                # panel width of chol.hip
BCR_MAXB = 256
CBF_MAXBW = 512
RATIO_CAP = 64.0
FWD_LIMIT = 2e8                        # forward check where n bw^2 <= this (cost of solve_ld)

PATHS = ("dense_panels", "band_panels", "band_fused", "band_two_ended", "bcr", "bcr_cyclic")

# Largest model / LAPACK ratios over cases(), per path: measured by
# tests/test_spd_ref_cpu.py::test_model_over_lapack_ratios_are_pinned (x86-64, 80-bit long double, OpenBLAS LAPACK), which
# prints them and asserts that the constants are the measurements, rounded up and capped at RATIO_CAP.
# Measured (eta ratio, forward ratio):
#   dense_panels    240, 258 (both capped)   band_panels  37.8, 28.2              band_fused  37.8, 28.2
#   band_two_ended  115, 85.7 (both capped)  bcr          209, 314 (both capped)  bcr_cyclic  4.63, 6.63
# THE CAPPED ONES ARE A FINDING ABOUT THE DESIGN ("SPD solver tests"): multiplying by the explicitly inverted
# 32 x 32 factor costs cond(L_kk) u, not u.  Worst cases of the model:
#   dense n = 32, delta 1e-8:            cond(S) 5.7e8, cond(L_kk) 2.4e4, eta 7.0e-15 (LAPACK 2.9e-17), fwd 2.2e-6 (LAPACK 8.6e-9)
#   bcr 479 / 20, delta 1e-8:            cond(S) 4.4e8, cond(L_kk) 1.8e4, eta 8.7e-15 (LAPACK 4.2e-17), fwd 2.1e-6 (LAPACK 6.8e-9)
#   two-ended 467 / 20, delta 1e-8:      cond(S) 4.5e8, cond(L_kk) 1.8e4, eta 8.2e-15 (LAPACK 7.1e-17), fwd 8.2e-7 (LAPACK 9.5e-9)
MODEL_VS_LAPACK_ETA = {"dense_panels": 64.0, "band_panels": 38.0, "band_fused": 38.0, "band_two_ended": 64.0, "bcr": 64.0,
                       "bcr_cyclic": 4.7}
MODEL_VS_LAPACK_FWD = {"dense_panels": 64.0, "band_panels": 29.0, "band_fused": 29.0, "band_two_ended": 64.0, "bcr": 64.0,
                       "bcr_cyclic": 6.7}


# Error of the reference, for the 50 x margin over LAPACK: the refined solve_ld is good to the order of eps_ld (its
# docstring); 2 eps_ld allows for the rounding of the stored solution on top of the limiting accuracy.  (The plain
# long-double solve is good to cond(S) eps_ld only, which is no margin at all on a ring -- one weak eigenvector among n
# puts LAPACK itself sqrt(n) below cond(S) u -- or on a scaled system with cond(D S D) ~ 1e14.)
REF_ERROR = 2.0 * EPS_LD
# Cases whose reference is NOT 50 x more accurate than fp64 LAPACK: they would keep the backward check and drop out of
# the forward check.  Pinned by tests/test_spd_ref_cpu.py::test_reference_is_50x_more_accurate_than_lapack: none.
FORWARD_DROPPED = ()


def eta_bound(path, eta_lapack):
    return max(4.0 * min(max(MODEL_VS_LAPACK_ETA[path], 1.0), RATIO_CAP) * eta_lapack, 4.0 * U64)


def fwd_bound(path, fwd_lapack):
    return 4.0 * min(max(MODEL_VS_LAPACK_FWD[path], 1.0), RATIO_CAP) * fwd_lapack


# ------------------------------------------------------------------------------------------------ generators
def chain_spd(n, bw, seed, delta, cyclic=False):
    """Window Gram matrix: for every window of bw + 1 consecutive indices (range(n - bw) of them, or all n wrapping
    ones if `cyclic`) add v v^T with v standard normal minus its mean; divide by the mean diagonal; add delta to the
    diagonal.  Exact half bandwidth bw (cyclic distance if `cyclic`); S 1 = delta 1, so cond ~ 4 / delta; neighbouring
    blocks stay coupled at ~1.00 on every level of a cyclic reduction.  bw = 0 has zero-sum vectors of one entry: the
    Gram part vanishes and the result is delta I."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    for w in range(n if cyclic else n - bw):
        v = rng.standard_normal(bw + 1)
        v -= v.mean()
        idx = (w + np.arange(bw + 1)) % n
        S[np.ix_(idx, idx)] += np.outer(v, v)
    md = np.trace(S) / n
    if md > 0.0:
        S /= md
    S[np.arange(n), np.arange(n)] += delta
    return S


def scaled(S, decades, seed):
    """D S D with log-uniform D over `decades` decades (rotation and translation blocks of very different scale)."""
    d = 10.0 ** np.random.default_rng(seed).uniform(-0.5 * decades, 0.5 * decades, len(S))
    return S * np.outer(d, d)     # (exactly symmetric: d_i d_j is one rounding either way)


def globally_indefinite(n, bw, seed, cyclic=False):
    """A window Gram matrix with zero-sum vectors and delta = 0, minus eps I.  Ring: chain_spd(delta = 0, cyclic).  Linear:
    the windows of chain_spd plus the clipped ones at both ends (starts -bw + 1 .. n - 2, each made zero-sum after
    clipping): chain_spd's own n - bw windows leave a null space of dimension bw whose vectors live at the two ends, so
    its leading blocks are singular to rounding and no eps > 0 keeps them positive definite; with the end windows the
    constant vector is the only null vector.  eps is half the smallest eigenvalue over the leading, the trailing and the
    middle principal block of order n // 2: by interlacing every principal block inside one of the three -- every leading
    block of order <= n / 2 in particular -- stays positive definite, while the whole matrix has the eigenvalue -eps.
    An elimination can only fail where it has brought the two halves together."""
    if cyclic:
        S = chain_spd(n, bw, seed, 0.0, True)
    else:
        rng = np.random.default_rng(seed)
        S = np.zeros((n, n))
        for w in range(-bw + 1, n - 1):
            idx = np.arange(max(w, 0), min(w + bw, n - 1) + 1)
            v = rng.standard_normal(len(idx))
            v -= v.mean()
            S[np.ix_(idx, idx)] += np.outer(v, v)
        S /= np.trace(S) / n
    h = n // 2
    lam = min(np.linalg.eigvalsh(S[o:o + h, o:o + h])[0] for o in (0, n - h, (n - h) // 2))
    assert lam > 1e-8, lam
    S[np.arange(n), np.arange(n)] -= 0.5 * lam
    for k in list(range(NB, h, NB)) + [h]:
        np.linalg.cholesky(S[:k, :k])
    return S


def truncate(S, bw, cyclic=False):
    """S with everything outside the (cyclic) half bandwidth bw set to zero."""
    i = np.arange(len(S))
    d = np.abs(i[:, None] - i[None, :])
    if cyclic:
        d = np.minimum(d, len(S) - d)
    return np.where(d <= bw, S, 0.0)


def half_bandwidth(S, cyclic=False):
    r, c = np.nonzero(S)
    d = np.abs(r - c)
    if cyclic:
        d = np.minimum(d, len(S) - d)
    return int(d.max()) if len(d) else 0


# ------------------------------------------------------------------------------------------------ long-double reference
def _band_factor_ld(S, bw):
    """Lower band Cholesky in long double, right-looking.  Flat storage F[i + j * bw] = L[i][j] (column j contiguous; the
    trailing block of a step is a regular strided view whose strictly upper part aliases entries of earlier columns, so
    only the lower triangle of the outer product is subtracted)."""
    n = len(S)
    F = np.zeros(n + n * max(bw, 1) + 1, LD)
    for d in range(min(bw, n - 1) + 1):
        j = np.arange(n - d)
        F[j + d + j * bw] = np.diagonal(S, -d)
    st = F.strides[0]
    for j in range(n):
        m = min(bw, n - 1 - j)
        o = j + j * bw
        if not F[o] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        F[o] = np.sqrt(F[o])
        if m:
            F[o + 1:o + 1 + m] /= F[o]
            col = F[o + 1:o + 1 + m]
            T = np.lib.stride_tricks.as_strided(F[o + 1 + bw:], (m, m), (st, st * bw))
            T -= np.tril(np.outer(col, col))
    return F


def _band_solve_ld(F, n, bw, Y):
    """L L^T X = Y for the factor of _band_factor_ld; Y is [n] or [n, k] long double, overwritten and returned."""
    for j in range(n):
        m = min(bw, n - 1 - j)
        o = j + j * bw
        Y[j] = Y[j] / F[o]
        if m:
            Y[j + 1:j + 1 + m] -= np.multiply.outer(F[o + 1:o + 1 + m], Y[j]) if Y.ndim == 2 else F[o + 1:o + 1 + m] * Y[j]
    for j in range(n - 1, -1, -1):
        m = min(bw, n - 1 - j)
        o = j + j * bw
        if m:
            Y[j] = Y[j] - F[o + 1:o + 1 + m] @ Y[j + 1:j + 1 + m]
        Y[j] = Y[j] / F[o]
    return Y


def _dense_factor_ld(A):
    n = len(A)
    A = A.copy()
    for j in range(n):
        if not A[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.tril(np.outer(A[j + 1:, j], A[j + 1:, j]))
    return np.tril(A)


def _dense_subst_ld(L, Y):
    n = len(L)
    for j in range(n):
        Y[j] = (Y[j] - L[j, :j] @ Y[:j]) / L[j, j]
    for j in range(n - 1, -1, -1):
        Y[j] = (Y[j] - L[j + 1:, j] @ Y[j + 1:]) / L[j, j]
    return Y


def _ld_solver(S, bw, cyclic):
    """rhs -> S^-1 rhs in long double, the factorisation done once.  The cyclic form eliminates the band of the first
    n - bw unknowns, to which the last bw are a border: S = [[A, E], [E^T, C]], Schur complement C - E^T A^-1 E by a
    dense long-double Cholesky."""
    n = len(S)
    if not cyclic:
        F = _band_factor_ld(S, bw)
        return lambda r: _band_solve_ld(F, n, bw, np.array(r, LD))
    if n <= 2 * bw + 1:
        L = _dense_factor_ld(S.astype(LD))
        return lambda r: _dense_subst_ld(L, np.array(r, LD))
    if bw == 0:
        d = np.diagonal(S).astype(LD)
        return lambda r: np.array(r, LD) / d
    na = n - bw
    F = _band_factor_ld(S[:na, :na], bw)
    E = S[:na, na:].astype(LD)
    AE = _band_solve_ld(F, na, bw, E.copy())
    Lc = _dense_factor_ld(S[na:, na:].astype(LD) - E.T @ AE)

    def solve(r):
        r = np.array(r, LD)
        y = _band_solve_ld(F, na, bw, r[:na].copy())
        x2 = _dense_subst_ld(Lc, r[na:] - E.T @ y)
        return np.concatenate([y - AE @ x2, x2])
    return solve


_SPLIT = LD(2.0 ** 32 + 1.0)    # Dekker's splitter for a 64-bit significand


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _two_prod(a, b):
    p = a * b
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _band_terms(S, bw, cyclic):
    """(row slice, coefficients, column slice) of every diagonal inside the (cyclic) half bandwidth."""
    n = len(S)
    yield slice(0, n), np.diagonal(S), slice(0, n)
    offs = list(range(1, min(bw, n - 1) + 1))
    if cyclic:  # the corner: |i - j| = n - d, and a diagonal already visited (n <= 2 bw) is not visited twice
        offs += [n - d for d in range(1, bw + 1) if n - d > bw and n - d < n]
    for d in offs:
        yield slice(d, n), np.diagonal(S, -d), slice(0, n - d)     # S[i + d][i]
        yield slice(0, n - d), np.diagonal(S, d), slice(d, n)      # S[i][i + d]


def residual_exact(S, x, b, bw, cyclic=False):
    """b - S x to about eps_ld^2 sum |S| |x|: every product exactly (Dekker) and the sum compensated, in long double."""
    x = np.asarray(x, LD)
    hi = np.array(b, LD)
    lo = np.zeros(len(hi), LD)
    for rows, coef, cols in _band_terms(S, bw, cyclic):
        p, e = _two_prod(-coef.astype(LD), x[cols])
        hi[rows], t = _two_sum(hi[rows], p)
        lo[rows] += t + e
    return hi + lo


def solve_ld(S, b, bw, cyclic=False, info=None):
    """x = S^-1 b in np.longdouble: right-looking band Cholesky with substitution (_ld_solver), then iterative refinement
    with the residual formed exactly (residual_exact) until the correction is below eps_ld.  S is read inside its
    (cyclic) half bandwidth bw only.  The plain solve is good to ~cond(S) eps_ld; with residuals at twice the working
    precision the refinement converges, as long as cond(S) eps_ld < 1, to a forward error of the order of eps_ld whatever
    the condition number (Higham, Accuracy and Stability of Numerical Algorithms, theorem 12.1).  info (optional) receives
    the plain solution and the relative size of every correction."""
    bw = min(bw, len(S) - 1)
    solve = _ld_solver(S, bw, cyclic)
    x = solve(b)
    steps = []
    if info is not None:
        info["plain"] = x.copy()
    for _ in range(6):
        dx = solve(residual_exact(S, x, b, bw, cyclic))
        x = x + dx
        steps.append(float(np.abs(dx).max() / np.abs(x).max()) if np.abs(x).max() > 0 else 0.0)
        if steps[-1] <= EPS_LD:
            break
    if info is not None:
        info["corrections"] = steps
    return x


def _band_product_ld(S, x, bw, cyclic):
    """(S x, row sums of |S|) in long double, from the diagonals within the (cyclic) half bandwidth only: O(n bw)."""
    x = np.asarray(x, LD)
    y = np.zeros(len(S), LD)
    rs = np.zeros(len(S), LD)
    for rows, coef, cols in _band_terms(S, bw, cyclic):
        y[rows] += coef.astype(LD) * x[cols]
        rs[rows] += np.abs(coef)
    return y, rs


def backward_error(S, x, b, bw, cyclic=False):
    """eta = ||S x - b||_inf / (||S||_inf ||x||_inf + ||b||_inf), the product in long double from the band only."""
    y, rs = _band_product_ld(S, x, bw, cyclic)
    den = rs.max() * np.abs(np.asarray(x, LD)).max() + np.abs(np.asarray(b, LD)).max()
    return float(np.abs(y - np.asarray(b, LD)).max() / den)


def forward_error(x, x_ld):
    return float(np.abs(np.asarray(x, LD) - x_ld).max() / np.abs(x_ld).max())


# ------------------------------------------------------------------------------------------------ layouts
def cyclic_layout(n, bw):
    """(B, n_blocks) of the ring solver or None: blocks of floor / ceil (n / n_blocks) >= bw + 1 unknowns, at least 8 of
    them, padded to B, the smallest multiple of 32 <= 256 that admits such a ring (include/vslam_hip.h,
    vsl_bcr_cyclic_layout)."""
    most = n // (bw + 1)
    B = (bw + 1 + 31) // 32 * 32
    while B <= BCR_MAXB:
        nblk = max(8, -(-n // B))
        if nblk <= most:
            return B, nblk
        B += 32
    return None


def bcr_layout(n, bw, cyclic=False):
    """(B, n_blocks, offsets) of the block cyclic reduction."""
    if cyclic:
        B, nblk = cyclic_layout(n, bw)
        return B, nblk, [i * n // nblk for i in range(nblk + 1)]
    B = (bw + 1 + 31) // 32 * 32
    nblk = -(-n // B)
    return B, nblk, [min(n, i * B) for i in range(nblk + 1)]


def bcr_levels(nblk):
    lv = 0
    while nblk > 1:
        nblk = (nblk + 1) // 2
        lv += 1
    return lv


def two_ended_split(n, bw):
    """(s, sp, sepn): top chunk [0, s), bottom chunk [n - sp, n), both whole panels, separator of bw .. bw + 31 between."""
    s = ((n - bw) // 2) // NB * NB
    sp = (n - s - bw) // NB * NB
    return s, sp, n - s - sp


def expected_path(n, bw_pass, cyclic=False, no_fused=0, no_bcr=0, one_ended=0):
    """The branch include/vslam_hip.h documents for vsl_spd_solve / vsl_spd_solve_cyclic, as (path, B, n_blocks, levels)."""
    if cyclic:
        B, nblk = cyclic_layout(n, bw_pass)
        return "bcr_cyclic", B, nblk, bcr_levels(nblk)
    if not (0 <= bw_pass < n - 1):
        return "dense_panels", 0, 0, 0
    B = (bw_pass + 1 + 31) // 32 * 32
    if not no_fused and not no_bcr and B <= BCR_MAXB and n >= 8 * B:
        nblk = -(-n // B)
        return "bcr", B, nblk, bcr_levels(nblk)
    if bw_pass <= CBF_MAXBW and not no_fused:
        if not one_ended and bw_pass + NB - 1 <= CBF_MAXBW and n >= 8 * (bw_pass + NB):
            return "band_two_ended", 0, 0, 0
        return "band_fused", 0, 0, 0
    return "band_panels", 0, 0, 0


# ------------------------------------------------------------------------------------------------ CPU models (fp64)
class PanelFactor:
    """Blocked right-looking Cholesky of a dense symmetric matrix, 32-column panels: the diagonal block is factored and
    its factor INVERTED (forward substitution of the identity); the panel below it and both substitutions multiply by
    that inverse.  `reach`: rows below a diagonal block that a panel visits (the half bandwidth; default all)."""

    def __init__(self, A, reach=None):
        n = len(A)
        self.n, self.reach = n, n if reach is None else reach
        self.L = np.tril(A).astype(np.float64)
        self.Linv, self.cond_diag = [], 1.0
        L = self.L
        for k in range(0, n, NB):
            nb = min(NB, n - k)
            Lkk = np.linalg.cholesky(L[k:k + nb, k:k + nb] + np.tril(L[k:k + nb, k:k + nb], -1).T)
            L[k:k + nb, k:k + nb] = Lkk
            Li = np.zeros((nb, nb))
            for c in range(nb):      # column c of the inverse: forward substitution of L x = e_c
                for r in range(c, nb):
                    Li[r, c] = ((1.0 if r == c else 0.0) - Lkk[r, c:r] @ Li[c:r, c]) / Lkk[r, r]
            self.Linv.append(Li)
            self.cond_diag = max(self.cond_diag, float(np.linalg.cond(Lkk)))
            e = min(n, k + nb + self.reach)
            if e > k + nb:
                P = L[k + nb:e, k:k + nb] @ Li.T
                L[k + nb:e, k:k + nb] = P
                L[k + nb:e, k + nb:e] -= np.tril(P @ P.T)

    def forward(self, Y):
        """L^-1 Y."""
        Y = np.array(Y, np.float64)
        for pi, k in enumerate(range(0, self.n, NB)):
            nb = min(NB, self.n - k)
            e = min(self.n, k + nb + self.reach)
            Y[k:k + nb] = self.Linv[pi] @ Y[k:k + nb]
            Y[k + nb:e] -= self.L[k + nb:e, k:k + nb] @ Y[k:k + nb]
        return Y

    def backward(self, Y):
        """L^-T Y."""
        Y = np.array(Y, np.float64)
        for pi in range(len(self.Linv) - 1, -1, -1):
            k = pi * NB
            nb = min(NB, self.n - k)
            e = min(self.n, k + nb + self.reach)
            Y[k:k + nb] = self.Linv[pi].T @ (Y[k:k + nb] - self.L[k + nb:e, k:k + nb].T @ Y[k + nb:e])
        return Y

    def solve(self, b):
        return self.backward(self.forward(b))


def model_natural(S, b, bw, info=None):
    f = PanelFactor(S, min(bw, len(S)))
    if info is not None:
        info["cond_diag"] = f.cond_diag
    return f.solve(b)


def model_two_ended(S, b, bw, info=None):
    """Top chunk top-down, bottom chunk bottom-up, separator last: the natural-order model under that permutation."""
    n = len(S)
    s, sp, sepn = two_ended_split(n, bw)
    perm = np.concatenate([np.arange(s), np.arange(n - 1, n - sp - 1, -1), np.arange(s, s + sepn)])
    f = PanelFactor(S[np.ix_(perm, perm)])
    if info is not None:
        info["cond_diag"] = f.cond_diag
    x = np.empty(n)
    x[perm] = f.solve(np.asarray(b)[perm])
    return x


def model_odd_even(S, b, bw, cyclic=False, info=None, solve=True):
    """Odd-even block order (block cyclic reduction): blocks of B unknowns, identity-padded; every level eliminates
    every other active block e with its neighbours p, q:  U_x = L_e^-1 S(e, x),  D_x -= U_x^T U_x,
    S(q, p) -= U_q^T U_p,  z_e = L_e^-1 b_e,  b_x -= U_x^T z_e;  back: x_e = L_e^-T (z_e - U_p x_p - U_q x_q).
    A ring (cyclic, >= 3 active blocks) closes the neighbour relation; whatever coupling two survivors already share
    (the wrap of an odd ring, the second coupling of a ring of two) adds to the fill.  info["coupling"][level] = the
    largest ||D_p^-1/2 K D_q^-1/2||_2 over the neighbouring active blocks of that level, info["coupling_min"][level]
    the smallest."""
    n = len(S)
    B, nblk, off = bcr_layout(n, bw, cyclic)
    D, rhs = [], []
    for i in range(nblk):
        sz = off[i + 1] - off[i]
        d = np.eye(B)
        d[:sz, :sz] = S[off[i]:off[i + 1], off[i]:off[i + 1]]
        D.append(d)
        r = np.zeros(B)
        r[:sz] = b[off[i]:off[i + 1]]
        rhs.append(r)
    K = {}                       # K[(a, c)], a > c: block (a, c) of the active system

    def coupling(a, c):          # block (a, c) or None
        if (a, c) in K:
            return K[(a, c)]
        return K[(c, a)].T if (c, a) in K else None

    for i in range(nblk):
        j = (i + 1) % nblk
        if j == 0 and (not cyclic or nblk < 2):
            continue
        k = np.zeros((B, B))
        k[:off[j + 1] - off[j], :off[i + 1] - off[i]] = S[off[j]:off[j + 1], off[i]:off[i + 1]]
        if (max(i, j), min(i, j)) in K:     # ring of two from the start: both couplings join the same pair
            K[(max(i, j), min(i, j))] += k if j > i else k.T
        else:
            K[(max(i, j), min(i, j))] = k if j > i else k.T
    active, steps, coup, coup_min, cond_diag = list(range(nblk)), [], [], [], 1.0
    while len(active) > 1:
        m = len(active)
        if info is not None:
            worst, least = 0.0, np.inf
            for (a, c), k in K.items():
                ia = np.linalg.inv(np.linalg.cholesky(D[a]))
                ic = np.linalg.inv(np.linalg.cholesky(D[c]))
                v = float(np.linalg.norm(ia @ k @ ic.T, 2))
                worst, least = max(worst, v), min(least, v)
            coup.append(worst)
            coup_min.append(least)
            if not solve and worst < 1e-13:
                break
        ring = cyclic and m >= 3
        for j in range(1, m, 2):
            e = active[j]
            nbrs = [active[j - 1]]
            if j + 1 < m:
                nbrs.append(active[j + 1])
            elif ring:
                nbrs.append(active[0])
            f = PanelFactor(D[e])
            cond_diag = max(cond_diag, f.cond_diag)
            Us = [f.forward(coupling(e, x)) for x in nbrs]
            z = f.forward(rhs[e])
            for x, Ux in zip(nbrs, Us):
                D[x] = D[x] - Ux.T @ Ux
                rhs[x] = rhs[x] - Ux.T @ z
                K.pop((max(e, x), min(e, x)))
            if len(nbrs) == 2:
                p, q = nbrs
                fill = -(Us[1].T @ Us[0])       # block (q, p)
                key = (max(p, q), min(p, q))
                if key[0] != q:
                    fill = fill.T
                K[key] = K[key] + fill if key in K else fill
            steps.append((e, nbrs, f, Us, z))
        active = active[0::2]
    if info is not None:
        info["coupling"] = coup
        info["coupling_min"] = coup_min
        info["levels"] = bcr_levels(nblk)
    if not solve:
        return None
    f = PanelFactor(D[active[0]])
    cond_diag = max(cond_diag, f.cond_diag)
    if info is not None:
        info["cond_diag"] = cond_diag
    xs = {active[0]: f.solve(rhs[active[0]])}
    for e, nbrs, f, Us, z in reversed(steps):
        t = z.copy()
        for x, Ux in zip(nbrs, Us):
            t -= Ux @ xs[x]
        xs[e] = f.backward(t)
    return np.concatenate([xs[i][:off[i + 1] - off[i]] for i in range(nblk)])


def model_solve(path, S, b, bw, info=None):
    """The model of the ordering that `path` uses."""
    if path in ("dense_panels", "band_panels", "band_fused"):
        return model_natural(S, b, len(S) if path == "dense_panels" else bw, info)
    if path == "band_two_ended":
        return model_two_ended(S, b, bw, info)
    return model_odd_even(S, b, bw, path == "bcr_cyclic", info)


def lapack_solve(S, b, bw, cyclic=False):
    """fp64 LAPACK on the same system: dpbsv on the band, dposv on a ring or a dense matrix."""
    import scipy.linalg as sla
    n = len(S)
    if cyclic or bw >= n - 1:
        return sla.cho_solve(sla.cho_factor(S, lower=True), b)
    ab = np.zeros((bw + 1, n))
    for d in range(bw + 1):
        ab[d, :n - d] = np.diagonal(S, -d)
    return sla.solveh_banded(ab, b, lower=True)


# ------------------------------------------------------------------------------------------------ the case list
def _case(name, n, bw, delta, seed, cyclic=False, bw_pass=None, decades=0, **diag):
    dense = bw_pass is not None and bw_pass < 0
    bwp = bw if bw_pass is None else bw_pass
    path, B, nblk, levels = expected_path(n, bwp, cyclic, diag.get("chol_no_fused", 0), diag.get("chol_no_bcr", 0),
                                          diag.get("chol_one_ended", 0))
    eff = n if dense else bwp
    return dict(name=name, n=n, bw=bw, delta=delta, seed=seed, cyclic=cyclic, bw_pass=bwp, decades=decades, diag=diag,
                path=path, block=B, n_blocks=nblk, levels=levels, forward=n * min(eff, n) ** 2 <= FWD_LIMIT)


def cases():
    """Every accuracy case of test_spd_ref_cpu.py and test_chol_edges_gpu.py: generator arguments (n, bw, delta, seed,
    cyclic, decades > 0: scaled), the half bandwidth passed to the solver (-1: dense), diagnostics, the expected path
    with block size, block count and level count, and whether the forward error is checked (n bw^2 <= 2e8)."""
    c = []
    # (the scaled variants of the reduction run over three decades, the others over six: with delta = 1e-6 six decades
    #  make cond(D S D) ~ 1e18, beyond what eigvalsh can measure and beyond cond eps_ld < 1, the premise of the reference)
    # (delta = 1e-3 lets the coupling of a reduction fall to 0.2 by the fourth level: the reduction cases use 1e-6 and
    #  1e-8, the band and dense paths all three)
    # linear block cyclic reduction.  B = 32: 8, 9, 15, 16, 17, 33 blocks (odd and even counts at every level), ragged
    # last blocks of 1 and of B - 1 unknowns, bw 0, 1, 20, 31; B = 64, 96, 224 (SLOTS 14) and 256 (SLOTS 17)
    c += [_case("bcr-b32-8blk-bw0", 256, 0, 1e-3, 1),
          # (windows of two make a weighted path: a weak link a^2 decouples the blocks unless delta lies well below
          #  it; delta and seed are chosen so that the coupling stays above 0.9 on all four levels)
          _case("bcr-b32-9blk-ragged1-bw1", 257, 1, 1e-8, 10),
          _case("bcr-b32-15blk-ragged31-bw20", 479, 20, 1e-8, 3),
          _case("bcr-b32-16blk-bw31", 512, 31, 1e-6, 4),
          _case("bcr-b32-17blk-bw31", 544, 31, 1e-6, 5),
          _case("bcr-b32-17blk-bw31-scaled", 544, 31, 1e-6, 5, decades=3),
          _case("bcr-b32-33blk-bw31", 1056, 31, 1e-8, 6),
          _case("bcr-b64-8blk-bw32", 512, 32, 1e-6, 7),
          _case("bcr-b96-9blk-ragged1-bw70", 769, 70, 1e-8, 8),
          _case("bcr-b224-8blk-bw221", 1792, 221, 1e-6, 9),
          _case("bcr-b256-9blk-bw255", 2304, 255, 1e-6, 10),
          _case("bcr-b32-16blk-bw31-1e-8", 512, 31, 1e-8, 12),
          _case("bcr-b32-17blk-bw31-1e-8", 544, 31, 1e-8, 13),
          _case("bcr-global-ba-5988-221", 5988, 221, 1e-6, 11)]
    # ring form: sizes through the ring layout; rings 8 -> 4 -> 2, 9 -> 5 -> 3 -> 2, 15, 16, 17, 33; every block ragged
    c += [_case("ring-b32-8blk-bw0", 256, 0, 1e-3, 21, cyclic=True),
          _case("ring-b32-9blk-bw1", 257, 1, 1e-6, 22, cyclic=True),
          _case("ring-b32-15blk-bw20", 479, 20, 1e-8, 23, cyclic=True),
          _case("ring-b32-16blk-bw31", 512, 31, 1e-6, 24, cyclic=True),
          _case("ring-b32-17blk-bw31", 544, 31, 1e-6, 25, cyclic=True),
          _case("ring-b32-17blk-bw31-scaled", 544, 31, 1e-6, 25, cyclic=True, decades=3),
          _case("ring-b32-33blk-bw31", 1056, 31, 1e-8, 26, cyclic=True),
          _case("ring-b32-16blk-bw31-1e-8", 512, 31, 1e-8, 32, cyclic=True),
          _case("ring-b64-8blk-bw31", 260, 31, 1e-6, 27, cyclic=True),
          _case("ring-b64-8blk-bw32", 512, 32, 1e-8, 28, cyclic=True),
          _case("ring-b96-9blk-bw70", 769, 70, 1e-6, 29, cyclic=True),
          _case("ring-b224-8blk-bw200", 1792, 200, 1e-6, 30, cyclic=True),
          _case("ring-b256-8blk-bw255", 2048, 255, 1e-6, 31, cyclic=True)]
    # two-ended band form: separators of exactly bw and bw + 31 unknowns, the band too wide for the reduction
    # (bw 256 at n = 2304, against bcr-b256-9blk-bw255), the reduction switched off
    c += [_case("two-ended-sep-bw", 436, 20, 1e-6, 41, chol_no_bcr=1),
          _case("two-ended-sep-bw+31", 467, 20, 1e-8, 42, chol_no_bcr=1),
          _case("two-ended-sep-bw-1e-3", 436, 20, 1e-3, 45, chol_no_bcr=1),
          _case("two-ended-bw256", 2304, 256, 1e-6, 43),
          _case("two-ended-scaled", 700, 31, 1e-3, 44, decades=6, chol_no_bcr=1)]
    # fused single-launch band form: one block short of the reduction (n = 8 B - 1 against bcr-b64-8blk-bw32), the widest
    # band it takes (512), bw = n - 2, one-ended by diagnostic
    c += [_case("fused-8B-1", 511, 32, 1e-6, 51),
          _case("fused-8B-1-1e-3", 511, 32, 1e-3, 55),
          _case("fused-bw512", 1000, 512, 1e-6, 52),
          _case("fused-bw-n-2", 300, 298, 1e-8, 53),
          _case("fused-one-ended", 467, 20, 1e-8, 42, chol_no_bcr=1, chol_one_ended=1),
          _case("fused-scaled", 511, 32, 1e-3, 54, decades=6)]
    # one launch per panel step: bw 513, bw = n - 2 beyond 512, the fused kernels switched off
    c += [_case("panels-bw513", 1000, 513, 1e-6, 61),
          _case("panels-bw-n-2", 600, 598, 1e-8, 62),
          _case("panels-no-fused", 467, 20, 1e-8, 42, chol_no_fused=1),
          _case("panels-no-fused-1e-3", 467, 20, 1e-3, 64, chol_no_fused=1),
          _case("panels-scaled", 333, 50, 1e-3, 63, decades=6, chol_no_fused=1)]
    # dense: a ragged last panel, 64-row tiles with 1 and 63 rows; bw = n - 1 is dense whatever is declared
    for n in (1, 31, 32, 33, 63, 64, 65, 97):
        c.append(_case("dense-n%d" % n, n, n // 2, (1e-3, 1e-6, 1e-8)[n % 3], 70 + n, bw_pass=-1))
    c += [_case("dense-n96-1e-8", 96, 48, 1e-8, 83, bw_pass=-1),
          _case("dense-bw-n-1", 300, 299, 1e-6, 81),
          _case("dense-scaled", 97, 48, 1e-3, 82, bw_pass=-1, decades=6)]
    return c


def build_case(case):
    """(S, b) of a case."""
    S = chain_spd(case["n"], case["bw"], case["seed"], case["delta"], case["cyclic"])
    if case["decades"]:
        S = scaled(S, case["decades"], case["seed"] + 1000)
    # b = S x for a random x: the solution then has no preferred direction, so the error along the weak eigenvectors --
    # cond(S) u of it -- is seen in full (a random b gives a solution that is almost all weak eigenvector, and a relative
    # forward error far below cond(S) u for every solver)
    b = S @ np.random.default_rng(case["seed"] + 2000).standard_normal(case["n"])
    return S, b


def band_spd_dominant(n, bw, seed):
    """The diagonally dominant random band of test_chol_gpu.py (its _band_spd), for the coupling comparison."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    for d in range(1, min(bw, n - 1) + 1):
        v = rng.standard_normal(n - d)
        S[np.arange(d, n), np.arange(0, n - d)] = v
    S = S + S.T
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(1) + rng.uniform(0.5, 1.5, n)
    return S
