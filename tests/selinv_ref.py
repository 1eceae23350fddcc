"""Reference side of the selected inversion (csrc/chol.hip "SELECTED INVERSION", vsl_spd_inverse_band): a long-double
inverse, the fold that turns a cyclic band into a linear one, and a plain fp64 numpy model of the panel recurrence.

The recurrence (Takahashi), over the 32-column panels of the band Cholesky factor L, LAST panel first: for the columns
K = [k, k + nb), W = the rows [k + nb, min(n, k + nb + bw)) and G = L_WK L_KK^-1
    Z_WK = -Z_WW G
    Z_KK = L_KK^-T L_KK^-1 - G^T Z_WK
Z_KK needs the whole product Z_WW G, the ragged-corner rows i - c > bw of a panel column c included; those are entries
of the inverse OUTSIDE the band, computed from in-band entries only (every |i - j| inside W is <= bw - 1).  `model`
with zero_ragged=True drops them before Z_KK is formed: the trap tests/test_selinv_ref_cpu.py keeps on record.

Tolerance of the device tests (the project's covariance rule, tests/test_ba_covariance_gpu.py): max |Z - Z_ref| over
the band <= 64 cond(S) 2^-52 max |Z_ref|, cond and Z_ref from the long-double reference.
"""
import functools

import numpy as np

import spd_ref as R

LD = R.LD
NB = R.NB


def inverse_ld(S):
    """S^-1 in long double: dense Cholesky and substitution on the unit columns (spd_ref's helpers)."""
    n = len(S)
    L = R._dense_factor_ld(np.asarray(S, LD))
    return R._dense_subst_ld(L, np.eye(n, dtype=LD))


def cond_of(S, Z_ref):
    """2-norm condition number from the matrix and its reference inverse."""
    return float(np.linalg.norm(np.asarray(S, np.float64), 2) * np.linalg.norm(np.asarray(Z_ref, np.float64), 2))


def tolerance(S, Z_ref):
    return 64.0 * cond_of(S, Z_ref) * 2.0 ** -52 * float(np.abs(Z_ref).max())


def band_mask(n, bw, cyclic=False):
    i = np.arange(n)
    d = np.abs(i[:, None] - i[None, :])
    if cyclic:
        d = np.minimum(d, n - d)
    return d <= bw


def band_error(Z, Z_ref, bw, cyclic=False):
    """max |Z - Z_ref| over the (cyclic) band."""
    m = band_mask(len(Z), bw, cyclic)
    return float(np.abs(np.where(m, np.asarray(Z, LD) - Z_ref, 0)).max())


# ------------------------------------------------------------------------------------------------ fold
def fold(n):
    """pos[p] = folded position of ring position p: 2 p on the way out (p < ceil(n / 2)), 2 (n - 1 - p) + 1 on the way
    back; ring[f] = the ring position at folded position f."""
    p = np.arange(n)
    pos = np.where(p < (n + 1) // 2, 2 * p, 2 * (n - 1 - p) + 1)
    ring = np.empty(n, int)
    ring[pos] = p
    return pos, ring


def folded(S):
    """The folded matrix A[pos[i], pos[j]] = S[i, j]."""
    _, ring = fold(len(S))
    return S[np.ix_(ring, ring)]


# ------------------------------------------------------------------------------------------------ model
def model(S, bw, zero_ragged=False):
    """The panel recurrence in plain fp64 numpy.  Returns the band of the inverse (|i - j| <= bw), zero elsewhere."""
    n = len(S)
    L = np.linalg.cholesky(S)
    Z = np.zeros((n, n))
    for k in reversed(range(0, n, NB)):
        nb = min(NB, n - k)
        K = slice(k, k + nb)
        hi = min(n, k + nb + bw)
        W = slice(k + nb, hi)
        Li = np.linalg.inv(L[K, K])
        G = L[W, K] @ Li
        T = Z[W, W] @ G
        rows = np.arange(k + nb, hi)[:, None]
        cols = np.arange(k, k + nb)[None, :]
        inband = rows - cols <= bw
        if zero_ragged:
            T = np.where(inband, T, 0.0)
        ZKK = Li.T @ Li + G.T @ T
        ZWK = np.where(inband, -T, 0.0)
        Z[W, K] = ZWK
        Z[K, W] = ZWK.T
        kk = np.arange(nb)
        low = np.where((kk[:, None] >= kk[None, :]) & (kk[:, None] - kk[None, :] <= bw), ZKK, 0.0)
        Z[K, K] = low + np.tril(low, -1).T   # the mirror of the lower triangle; a panel wider than the band is cut to it
    return Z


def model_cyclic(S, bw, zero_ragged=False):
    """The ring: fold, invert the linear band of half bandwidth min(2 bw, n - 1), unfold, keep the cyclic band."""
    n = len(S)
    pos, _ = fold(n)
    Zf = model(folded(S), min(2 * bw, n - 1), zero_ragged)
    return np.where(band_mask(n, bw, True), Zf[np.ix_(pos, pos)], 0.0)


# ------------------------------------------------------------------------------------------------ cases
def _c(name, n, bw, delta, cyclic=False, decades=0, seed=3, bw_pass=None):
    return dict(name=name, n=n, bw=bw, delta=delta, cyclic=cyclic, decades=decades, seed=seed,
                bw_pass=bw if bw_pass is None else bw_pass)


def cases():
    """The accuracy cases of the CPU model test and of the device test."""
    return [
        _c("one_panel_plus_row", 33, 5, 1e-3),
        _c("window_wider_than_panel", 64, 40, 1e-2),
        _c("n97_bw40", 97, 40, 1e-4),
        _c("n132_bw11", 132, 11, 1e-2),
        _c("n200_bw20", 200, 20, 1e-6),
        _c("n479_bw20_cond4e8", 479, 20, 1e-8),
        _c("ring_n138_bw11", 138, 11, 1e-4, cyclic=True),
        _c("ring_odd_n301_bw17", 301, 17, 1e-6, cyclic=True),
        _c("scaled_n200_bw20", 200, 20, 1e-3, decades=6),
        _c("diagonal_n40", 40, 0, 1.0),
        _c("single_unknown", 1, 0, 1.0),
        _c("dense_route_n45", 45, 9, 1e-3, bw_pass=44),
    ]


def build(case):
    if case["n"] == 1:
        return np.array([[2.5]])
    if case["bw"] == 0:
        return np.diag(np.random.default_rng(case["seed"]).uniform(0.5, 4.0, case["n"]))
    S = R.chain_spd(case["n"], case["bw"], case["seed"], case["delta"], case["cyclic"])
    if case["decades"]:
        S = R.scaled(S, case["decades"], case["seed"] + 1)
    return S


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = next(c for c in cases() if c["name"] == name)
    S = build(case)
    S.setflags(write=False)
    Z = inverse_ld(S)
    Z.setflags(write=False)
    return S, Z, tolerance(S, Z)


def reference(case):
    """(S, Z_ref in long double, tolerance) of a case, computed once per process and read-only."""
    return _reference(case["name"])
