"""GPU parity: bundle adjustment with free intrinsics (ba.hip from "optimize_intrinsics" on: project_intr_jac, the bai_*
kernels, the 16-column border of the reduced system, the dense-solver seam at nt = 6 n_free + 16 <= 128) against the
long-double reference tests/ba_intr_ref.py on its case table, through the parity hook vsl_ba_intrinsics_system and one
iteration of the public call.

Tolerances (ba_intr_ref.py; the constants are measured on the CPU by test_ba_intr_ref_cpu.py):
  G                jac_tol(case) relative to the block's largest entry; unused columns exactly 0
  scale            (K_INTR_GPU * 2^-52 + jac_tol(case)) relative; exactly 1 on zero columns
  S, rhs           entrywise |x - x_ref| <= K_INTR_GPU * 2^-52 * A, A from the reference in the scaled variables
  S - S^T          2 K_INTR_GPU * 2^-52 * A (both triangles are accumulated by atomics in an order of their own)
  cost             ba_ref.COST_GPU relative
  d, dl, one step  64 * cond_S * 2^-52 * max|x_ref| wherever 64 * cond_S * 2^-52 < 1e-3
Each test prints its worst figure (`pytest -s`).
The step at 1 / radius = 0 is compared on ba_intr_ref.UNDAMPED_SOLVABLE only: every other case is singular there by
construction (unused parameters are zero columns, one fixed camera leaves the scale free); a case with a zero column
must report chol_ok == 0.
"""
import ctypes as C

import numpy as np
import pytest

import ba_intr_ref as ref
import ba_ref

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = ref.U
NAMES = sorted(ref.cases())
K = ref.K_INTR_GPU


def _arr(vsl, p):
    return vsl.BaArrays(p.poses, p.cam_fixed, p.cam_intr, p.intr, p.points, p.obs_cam, p.obs_lm, p.obs_uv, p.cam_model)


_OUT = {}


def _system(ctx, vsl, name, inv_radius):
    """The hook's output of a case, computed once and shared by the checks (read-only)."""
    key = (name, inv_radius)
    if key not in _OUT:
        p = ref.cases()[name]
        _OUT[key] = ctx.ba_intrinsics_system(_arr(vsl, p), inv_radius, use_huber=p.use_huber, huber=p.huber)
    return _OUT[key]


@pytest.mark.parametrize("name", NAMES)
def test_intrinsics_jacobian(ctx, vsl, name):
    p, R = ref.cases()[name], ref.reference(name, 1e-4)
    G = _system(ctx, vsl, name, 1e-4)["G"]
    e = float(ref.block_error(G, R.G).max())
    print("%s: G %.3g (bound %.3g)" % (name, e, ref.jac_tol(name)))
    assert e <= ref.jac_tol(name)
    for i in range(len(p.obs_cam)):
        used = ref.N_USED[p.cam_model[p.cam_intr[p.obs_cam[i]]]]
        assert not G[i, :, used:].any(), (name, i)
    if name == "g_kb4_awkward":     # r == 0: u = cx, v = cy whatever the rest; residual = uv - projection
        want = np.zeros((2, 8))
        want[0, 2] = want[1, 3] = -1.0
        assert np.array_equal(G[p.special[0]], want)


@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
@pytest.mark.parametrize("name", NAMES)
def test_system(ctx, vsl, name, inv_radius):
    p, R = ref.cases()[name], ref.reference(name, inv_radius)
    out = _system(ctx, vsl, name, inv_radius)
    n = 6 * p.n_free
    nt = n + 16
    assert out["n_free"] == p.n_free and out["S"].shape == (nt, nt)
    # scale
    D = R.D[:nt]
    zero = np.diag(R.H)[:nt] == 0
    kD = float((np.abs(out["scale"] - D) / (U * D)).max())
    assert np.array_equal(out["scale"][zero], np.ones(int(zero.sum())))
    # S, rhs, symmetry, cost
    kS, kg = ref.ratio(out["S"], R.S, R.A_S), ref.ratio(out["rhs"], R.g, R.A_g)
    ksym = ref.ratio(out["S"], out["S"].T, R.A_S)
    ce = abs(out["cost"] - R.cost) / R.cost
    print("%s 1/radius %g: scale %.3g, S %.3g, rhs %.3g (bound %.3g), S - S^T %.3g (bound %.3g), cost %.3g (bound %.3g)"
          % (name, inv_radius, kD, kS, kg, K, ksym, 2 * K, ce, ba_ref.COST_GPU))
    assert kD * U <= K * U + ref.jac_tol(name)
    assert kS <= K and kg <= K
    assert ksym <= 2 * K
    assert ce <= ba_ref.COST_GPU
    # a column nobody observes: the damping on the diagonal, nothing else, to the bit
    for j in np.flatnonzero(zero):
        row, col = out["S"][j].copy(), out["S"][:, j].copy()
        assert row[j] == 1e-6 * inv_radius
        row[j] = col[j] = 0.0
        assert not row.any() and not col.any() and out["rhs"][j] == 0.0, (name, j)
    if name == "b_unobserved_block":
        assert np.array_equal(np.flatnonzero(zero)[-8:], np.arange(n + 8, n + 16))
    # the step
    solvable = ref.solvable(R)
    assert solvable == (inv_radius > 0 or name in ref.UNDAMPED_SOLVABLE), (name, R.cond_S)
    if solvable:
        assert out["chol_ok"] == 1
        tol = 64 * R.cond_S * U
        ed = float(np.abs(out["d"] - R.d).max() / np.abs(R.d).max())
        el = float(np.abs(out["dl"] - R.dl).max() / np.abs(R.dl).max())
        print("%s 1/radius %g: d %.3g, dl %.3g (bound %.3g, cond %.3g)" % (name, inv_radius, ed, el, tol, R.cond_S))
        assert ed <= tol and el <= tol
    else:
        print("%s 1/radius %g: step not compared (cond %.3g), chol_ok %d" % (name, inv_radius, R.cond_S, out["chol_ok"]))
        if inv_radius == 0 and zero.any():
            assert out["chol_ok"] == 0      # a zero pivot


def _mark_spd_path(ctx):
    """Leaves the record of a BAND solve (tridiagonal, 64 unknowns) in the context, which no dense solve produces: a later
    read-out tells whether the general SPD solver ran in between."""
    S = 4.0 * np.eye(64) + np.eye(64, k=1) + np.eye(64, k=-1)
    ctx.spd_solve(S, np.ones(64), 1)
    return ctx.last_spd_path()


def test_both_sides_of_the_dense_solver_seam(ctx, vsl):
    # nt = 124: ba_chol_small_kernel, which does not pass through the SPD plan; nt = 130: vsl_chol_solve_band_dev, which
    # records its path (vsl_ctx_last_spd_path) -- although n = 114 <= 128.  Both cases pass every check of test_system.
    for name, nt, general in (("i_seam_18_free", 124, False), ("i_seam_19_free", 130, True)):
        p = ref.cases()[name]
        assert 6 * p.n_free + 16 == nt and 6 * p.n_free <= 128
        marker = _mark_spd_path(ctx)
        out = ctx.ba_intrinsics_system(_arr(vsl, p), 1e-4, use_huber=p.use_huber, huber=p.huber)
        assert out["chol_ok"] == 1
        after = ctx.last_spd_path()
        print("%s: nt %d, SPD path record %s -> %s" % (name, nt, marker, after))
        assert (after != marker) == general and (after[0] != marker[0]) == general, (name, marker, after)


@pytest.mark.parametrize("name", NAMES)
def test_one_iteration_of_the_public_call(ctx, vsl, name):
    p, s = ref.cases()[name], ref.reference_step(name, 1e-4)
    assert ref.solvable(s.lin)
    arr = _arr(vsl, p)
    summ = ctx.bundle_adjust_intrinsics(arr, use_huber=p.use_huber, huber=p.huber, max_iters=1)
    assert abs(summ.initial_cost - s.cost) <= ba_ref.COST_GPU * s.cost
    assert summ.iterations == 1 and summ.successful_steps == int(s.accepted)
    if not s.accepted:
        print("%s: step rejected (gain %.4g)" % (name, s.gain))
        assert np.array_equal(arr.poses, p.poses) and np.array_equal(arr.points, p.points) and np.array_equal(arr.intr, p.intr)
        return
    tol = 64 * s.lin.cond_S * U
    n = 6 * p.n_free
    free = p.cam_fixed == 0
    q = arr.poses.copy()
    q[np.sum(q[:, :4] * s.poses[:, :4].astype(np.float64), axis=1) < 0, :4] *= -1
    ep = float(np.abs(q - s.poses).max() / np.abs(s.step_c).max()) if free.any() else 0.0
    el = float(np.abs(arr.points - s.points).max() / np.abs(s.step_l).max())
    # intrinsics: absolute, in units of the scaled step's largest entry times the column's D
    Di = s.lin.D[n:n + 16].reshape(2, 8)
    ei = float((np.abs(arr.intr - s.intr) / (Di * np.abs(s.d).max())).max())
    print("%s: poses %.3g, points %.3g, intrinsics %.3g of the step (bound %.3g); cost %.6g -> %.6g, gain %.4g"
          % (name, ep, el, ei, tol, s.cost, s.cand_cost, s.gain))
    assert ep <= tol and el <= tol and ei <= tol
    assert np.array_equal(arr.poses[~free], p.poses[~free])
    for k in range(2):      # parameters the model does not use, and a block nobody observes, keep their bits
        used = ref.N_USED[p.cam_model[k]] if (p.cam_intr[p.obs_cam] == k).any() else 0
        assert np.array_equal(arr.intr[k, used:], p.intr[k, used:]), (name, k)
    assert abs(summ.final_cost - s.cand_cost) <= max(ba_ref.COST_GPU, tol) * s.cost


def test_repeatability(ctx, vsl):
    # the fp64 atomics may land in another order from call to call: bounded, not bitwise
    name = "a_base_ds"
    p, R = ref.cases()[name], ref.reference(name, 1e-4)
    a = ctx.ba_intrinsics_system(_arr(vsl, p), 1e-4, use_huber=p.use_huber, huber=p.huber)
    b = ctx.ba_intrinsics_system(_arr(vsl, p), 1e-4, use_huber=p.use_huber, huber=p.huber)
    kS, kg = ref.ratio(a["S"], b["S"], R.A_S), ref.ratio(a["rhs"], b["rhs"], R.A_g)
    print("%s twice: S %.3g, rhs %.3g units of 2^-52 A (bound %.3g); bit-equal %s" % (name, kS, kg, 2 * K, kS == 0 and kg == 0))
    assert kS <= 2 * K and kg <= 2 * K
    assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["scale"][-16:] == 1.0, b["scale"][-16:] == 1.0)


def test_error_returns_write_nothing(ctx, vsl):
    p = ref.cases()["a_base_ds"]
    arr = _arr(vsl, p)
    st = ctx._ba_struct(arr)
    o = ctx._ba_opts(True, 1.0, 0, 0)
    f64p = C.POINTER(C.c_double)
    nt, O, L = 6 * p.n_free + 16, len(p.obs_cam), len(p.points)
    bufs = [np.full(k, 7.25) for k in (16 * O, nt, nt * nt, nt, 1, nt, 3 * L)]
    ok = C.c_int32(77)

    def call(prob, opt, intr, inv_radius):
        G, scale, S, rhs, cost, d, dl = (b.ctypes.data_as(f64p) for b in bufs)
        return ctx.L.vsl_ba_intrinsics_system(ctx.h, prob, opt, intr, C.c_double(inv_radius), G, scale, S, rhs, cost, d, dl, C.byref(ok))

    intr = arr.intr.ctypes.data_as(f64p)
    assert call(None, C.byref(o), intr, 1e-4) == -1
    assert call(C.byref(st), None, intr, 1e-4) == -1
    assert call(C.byref(st), C.byref(o), None, 1e-4) == -1
    for bad in (float("nan"), float("inf"), -1.0):
        assert call(C.byref(st), C.byref(o), intr, bad) == -1
    bad_st = ctx._ba_struct(arr)
    bad_st.obs_cam = None
    assert call(C.byref(bad_st), C.byref(o), intr, 1e-4) == -1
    assert all((b == 7.25).all() for b in bufs) and ok.value == 77
    # and every output may be absent
    assert ctx.L.vsl_ba_intrinsics_system(ctx.h, C.byref(st), C.byref(o), intr, C.c_double(1e-4), None, None, None, None, None,
                                          None, None, C.byref(ok)) == 0 and ok.value == 1
