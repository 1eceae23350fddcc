"""The solver of the reduced camera system on its own (visual-slam_amd/csrc/chol.hip through vsl_spd_solve): the place
where Ceres hands S to a sparse Cholesky (include/visnav/map_utils.h:406-411, loop_closure_utils.h:735).  Checked by
the property the caller relies on -- S x = b to a relative residual of 1e-10 -- against numpy on small systems, and
at the size of BASELINE configs[4] (5988 unknowns, half bandwidth 221) where a dense reference would take minutes.

The matrices here are diagonally dominant (cond ~3, block coupling that vanishes by the fourth reduction level): this
file pins the agreement of the paths on easy systems.  Accuracy claims -- ill-conditioned systems, backward and forward
error against a long-double reference, the path each case takes -- are made by tests/test_chol_edges_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _band_spd(n, bw, seed):
    """Random symmetric band matrix made positive definite by diagonal dominance; dense row-major."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    for d in range(1, min(bw, n - 1) + 1):
        v = rng.standard_normal(n - d)
        S[np.arange(d, n), np.arange(0, n - d)] = v
    S = S + S.T
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(1) + rng.uniform(0.5, 1.5, n)
    return S


def _residual(S, x, b):
    return np.linalg.norm(S @ x - b) / np.linalg.norm(b)


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 64, 200, 777])
def test_dense_solve_small(ctx, n):
    rng = np.random.default_rng(n)
    A = rng.standard_normal((n, n + 3))
    S = A @ A.T + 0.5 * np.eye(n)
    b = rng.standard_normal(n)
    x = ctx.spd_solve(S, b)
    assert _residual(S, x, b) < 1e-10
    assert np.allclose(x, np.linalg.solve(S, b), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("n,bw", [(40, 3), (100, 31), (100, 32), (333, 50), (600, 221), (1000, 512), (1000, 513), (700, 640)])
@pytest.mark.parametrize("fused", [1, 0])
def test_band_solve_matches_dense_and_numpy(ctx, n, bw, fused):
    # half bandwidths around the 32-column panel width, at the limit of the single-launch kernel (512) and beyond it;
    # both band code paths (single launch / one launch per panel step) and the dense path agree
    S = _band_spd(n, bw, 7 * n + bw)
    b = np.random.default_rng(n + bw).standard_normal(n)
    ctx.set_diagnostic("chol_no_fused", 0 if fused else 1)
    try:
        x = ctx.spd_solve(S, b, bw)
    finally:
        ctx.set_diagnostic("chol_no_fused", 0)
    assert _residual(S, x, b) < 1e-10
    xd = ctx.spd_solve(S, b)
    assert np.allclose(x, xd, rtol=1e-9, atol=1e-12)
    assert np.allclose(x, np.linalg.solve(S, b), rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize("n,bw", [(700, 20), (701, 20), (2000, 100), (2017, 100), (3000, 37), (1500, 150), (4200, 481)])
def test_two_ended_elimination_matches_one_ended(ctx, n, bw):
    # long narrow bands (n >= 8 (bw + 32)) are eliminated from both ends towards a separator in the middle; sizes with
    # whole and ragged panel counts on either side, separators of bw .. bw + 31 unknowns, up to the widest band the
    # split is used for (bw + 31 <= 512)
    assert n >= 8 * (bw + 32)
    S = _band_spd(n, bw, 3 * n + bw)
    b = np.random.default_rng(n - bw).standard_normal(n)
    ctx.set_diagnostic("chol_no_bcr", 1)   # (long bands default to block cyclic reduction: next test)
    try:
        x2 = ctx.spd_solve(S, b, bw)
        ctx.set_diagnostic("chol_one_ended", 1)
        x1 = ctx.spd_solve(S, b, bw)
    finally:
        ctx.set_diagnostic("chol_one_ended", 0)
        ctx.set_diagnostic("chol_no_bcr", 0)
    assert _residual(S, x2, b) < 1e-10 and _residual(S, x1, b) < 1e-10
    assert np.allclose(x2, x1, rtol=1e-9, atol=1e-12)
    assert np.allclose(x2, np.linalg.solve(S, b), rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize("n,bw", [(300, 20), (700, 20), (701, 31), (2000, 100), (2017, 100), (3000, 37), (1500, 150), (2100, 255),
                                  (5988, 221)])
def test_block_cyclic_reduction_matches_band_cholesky(ctx, n, bw):
    # long narrow bands (n >= 8 blocks of B = ceil((bw + 1) / 32) * 32 <= 256 unknowns) are solved by block cyclic
    # reduction: odd and even block counts, a ragged last block (identity-padded), block sizes from 32 to 256, and the
    # size of BASELINE configs[4]; same solution as the band Cholesky and as numpy
    B = (bw + 1 + 31) // 32 * 32
    assert n >= 8 * B and B <= 256
    S = _band_spd(n, bw, 5 * n + bw)
    b = np.random.default_rng(n + 3 * bw).standard_normal(n)
    x = ctx.spd_solve(S, b, bw)
    ctx.set_diagnostic("chol_no_bcr", 1)
    try:
        xb = ctx.spd_solve(S, b, bw)
    finally:
        ctx.set_diagnostic("chol_no_bcr", 0)
    assert _residual(S, x, b) < 1e-10
    assert np.allclose(x, xb, rtol=1e-9, atol=1e-12)
    if n <= 3000:
        assert np.allclose(x, np.linalg.solve(S, b), rtol=1e-8, atol=1e-11)
    x_again = ctx.spd_solve(S, b, bw)
    assert np.array_equal(x, x_again)  # no atomics anywhere: bit-identical reruns


@pytest.mark.parametrize("where", [40, 1003, 1990])
@pytest.mark.parametrize("no_bcr", [0, 1])
def test_long_band_solvers_report_a_bad_pivot_anywhere(ctx, vsl, where, no_bcr):
    # a negative diagonal entry near the top, in the middle (the separator of the two-ended form), near the bottom --
    # through block cyclic reduction (different blocks / levels) and through the two-ended band Cholesky
    n, bw = 2000, 60
    S = _band_spd(n, bw, 9)
    S[where, where] = -1.0
    ctx.set_diagnostic("chol_no_bcr", no_bcr)
    try:
        with pytest.raises(vsl.VslError) as e:
            ctx.spd_solve(S, np.ones(n), bw)
    finally:
        ctx.set_diagnostic("chol_no_bcr", 0)
    assert e.value.code == -7


def test_band_solve_at_global_ba_size(ctx):
    # BASELINE configs[4]: 998 free cameras -> 5988 unknowns, half bandwidth 221 after the reverse Cuthill-McKee
    # renumbering; ||S x - b|| / ||b|| <= 1e-10, and a wider declared band gives the same x
    n, bw = 5988, 221
    S = _band_spd(n, bw, 11)
    b = np.random.default_rng(12).standard_normal(n)
    x = ctx.spd_solve(S, b, bw)
    assert _residual(S, x, b) < 1e-10
    x2 = ctx.spd_solve(S, b, 300)
    assert np.allclose(x, x2, rtol=1e-9, atol=1e-13)


def test_badly_scaled_band_system(ctx):
    # a reduced camera system mixes rotation and translation blocks of very different scale: rows / columns of a
    # well-conditioned band matrix scaled over six decades (condition number ~1e12).  Cholesky is scale-invariant, so
    # the componentwise backward error stays at rounding level and the scaled solution agrees with the unscaled one
    n, bw = 900, 60
    rng = np.random.default_rng(5)
    S0 = _band_spd(n, bw, 21)
    d = 10.0 ** rng.uniform(-3, 3, n)
    S = S0 * d[:, None] * d[None, :]
    b0 = rng.standard_normal(n)
    b = b0 * d
    x = ctx.spd_solve(S, b, bw)
    back = np.abs(S @ x - b) / (np.abs(S) @ np.abs(x) + np.abs(b))
    assert back.max() < 1e-12
    x0 = ctx.spd_solve(S0, b0, bw)
    assert np.allclose(x * d, x0, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("bw", [-1, 40])
def test_not_positive_definite_is_reported(ctx, vsl, bw):
    n = 300
    S = _band_spd(n, 40, 3)
    S[150, 150] = -1.0
    with pytest.raises(vsl.VslError) as e:
        ctx.spd_solve(S, np.ones(n), bw)
    assert e.value.code == -7  # VSL_ERR_NUMERIC


def _cyclic_band_spd(n, bw, seed):
    """Random symmetric CYCLIC band matrix (non-zeros within cyclic distance bw of the diagonal), diagonally dominant."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    idx = np.arange(n)
    for d in range(1, bw + 1):
        v = rng.standard_normal(n)
        r, c = idx, (idx - d) % n      # (i, i - d), the wrap-around corner included
        S[r, c] += v
        S[c, r] += v
    S[idx, idx] = np.abs(S).sum(1) + rng.uniform(0.5, 1.5, n)
    return S


@pytest.mark.parametrize("n,bw", [(1024, 100), (1000, 113), (2000, 221), (5988, 113), (1100, 31), (1030, 127), (4097, 60),
                                  (1040, 128)])
def test_cyclic_block_cyclic_reduction(ctx, n, bw):
    # the ring form of the block cyclic reduction (a closed camera loop ordered along its trajectory): even and odd rings
    # at every level, rings of three and two at the end, block sizes that are / are not multiples of the kernels' 32,
    # a half bandwidth of exactly a block (the layout moves to the next block size)
    S = _cyclic_band_spd(n, bw, n + bw)
    rng = np.random.default_rng(7 * n + bw)
    b = rng.standard_normal(n)
    x = ctx.spd_solve_cyclic(S, b, bw)
    assert _residual(S, x, b) < 1e-10
    if n <= 2000:
        assert np.allclose(x, np.linalg.solve(S, b), rtol=1e-8, atol=1e-10)


def test_cyclic_form_equals_the_linear_band_form_without_a_corner(ctx):
    # a plain band matrix IS a cyclic band matrix with an empty corner: both solvers, the same solution
    n, bw = 3000, 90
    S = _band_spd(n, bw, 99)
    b = np.random.default_rng(5).standard_normal(n)
    x_lin = ctx.spd_solve(S, b, bw)
    x_cyc = ctx.spd_solve_cyclic(S, b, bw)
    assert _residual(S, x_cyc, b) < 1e-10
    assert np.allclose(x_cyc, x_lin, rtol=1e-9, atol=1e-12)


def test_cyclic_solver_reports_what_it_cannot_take(ctx, vsl):
    S = _cyclic_band_spd(600, 100, 3)
    with pytest.raises(vsl.VslError):
        ctx.spd_solve_cyclic(S, np.ones(600), 100)     # fewer than 8 blocks of >= 101 unknowns
    S = _cyclic_band_spd(1200, 40, 4)
    S[700, 700] = -1.0
    with pytest.raises(vsl.VslError):
        ctx.spd_solve_cyclic(S, np.ones(1200), 40)     # not positive definite
