"""GPU parity: the bundle-adjustment kernels (ba.hip, ba_fused.hip, ba_large.h, ba_device.h) against the long-double
reference tests/ba_ref.py on the observation, Huber and structure tables of that file -- the cases the synthetic scenes
of test_ba_gpu.py never reach.

Tolerances (ba_ref.py; the constants are measured on the CPU by test_ba_ref_cpu.py, the device gets 8 x):
  residuals        RES_GPU px absolute
  Jacobian blocks  jac_tol(case) relative to the block's largest entry: 8 x the oracle's constant unless the case's own
                   finite differences are coarser than a tenth of that
  S, g / rhs       entrywise |x - x_ref| <= K_GPU * 2^-52 * A, A from the reference (never max|S|); in the fused hook's
                   scaled variables A keeps the condition numbers of the plain landmark blocks (ba_ref.py, "fused form")
  scale_c          (K_GPU * 2^-52 + jac_tol(case)) relative: diag H is a sum of squares (A is the entry itself, the root halves
                   the error) of Jacobian entries that are themselves only held to jac_tol
  cost             COST_GPU relative
  dc, first step   64 * cond * 2^-52 * max|x_ref|, cond of the reference's system
Each test prints its worst figure (`pytest -s`).
Out of scope: a landmark with a single observation in the whole problem -- P_l is singular by construction and the
reference project behaves no better.
"""
import numpy as np
import pytest

import ba_ref as ref

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = ref.U
NAMES = sorted(ref.cases())
SMALL = [n for n in NAMES if 0 < 6 * ref.cases()[n].n_free <= 126]
DC_UNDAMPED = ("structure/cams64", "structure/fixed_only_and_unobserved", "structure/n1", "structure/n8", "structure/n16",
               "structure/n21")
FUSED_DECLINES = ("structure/observed_twice", "structure/observed_30_times", "structure/cams65")


def _arr(vsl, p):
    return vsl.BaArrays(p.poses, p.cam_fixed, p.cam_intr, p.intr, p.points, p.obs_cam, p.obs_lm, p.obs_uv, p.cam_model)


def _check_system(name, S, g, cost, R, what):
    kS, kg = ref.ratio(S, R.S, R.A_S), ref.ratio(g, R.g, R.A_g)
    ce = abs(cost - R.cost) / (R.cost if R.cost > 0 else 1.0)
    print("%s %s: S %.3g, g %.3g (bound %.3g); cost %.3g (bound %.3g)" % (name, what, kS, kg, ref.K_GPU, ce, ref.COST_GPU))
    assert kS <= ref.K_GPU and kg <= ref.K_GPU, (name, what, kS, kg)
    assert ce <= ref.COST_GPU, (name, what, ce)
    return max(kS, kg)


@pytest.mark.parametrize("name", NAMES)
def test_residuals_and_jacobian_blocks(ctx, vsl, name):
    p, R = ref.cases()[name], ref.reference(name)
    r, F, E = ctx.ba_residuals_jacobians(_arr(vsl, p))
    er = float(np.abs(r - R.r).max())
    eF, eE = float(ref.block_error(F, R.F).max()), float(ref.block_error(E, R.E).max())
    print("%s: residual %.3g px (bound %.3g), F %.3g, E %.3g (bound %.3g)" % (name, er, ref.RES_GPU, eF, eE, ref.jac_tol(name)))
    assert er <= ref.RES_GPU
    assert eF <= ref.jac_tol(name) and eE <= ref.jac_tol(name)
    if name == "obs/kb4/axis":      # the r == 0 branch: the value is (cx, cy) exactly
        assert np.array_equal(r[p.special], p.obs_uv[p.special] - p.intr[p.cam_intr[p.obs_cam[p.special]], 2:4])


@pytest.mark.parametrize("name", NAMES)
def test_linearize_default(ctx, vsl, name):
    p = ref.cases()[name]
    S, g, cost = ctx.ba_linearize(_arr(vsl, p), use_huber=p.use_huber, huber=p.huber)
    _check_system(name, S, g, cost, ref.reference(name), "linearize")


@pytest.mark.parametrize("name", SMALL)
def test_linearize_single_entry_ownership(ctx, vsl, name):
    p = ref.cases()[name]
    ctx.set_diagnostic("ba_schur_entries", 1)
    try:
        S, g, cost = ctx.ba_linearize(_arr(vsl, p), use_huber=p.use_huber, huber=p.huber)
    finally:
        ctx.set_diagnostic("ba_schur_entries", 0)
    _check_system(name, S, g, cost, ref.reference(name), "ba_schur_entries")


@pytest.mark.parametrize("atomics", [0, 1])
def test_linearize_beyond_128_unknowns(ctx, vsl, atomics):
    name = "structure/n22"
    p = ref.cases()[name]
    assert 6 * p.n_free > 128
    ctx.set_diagnostic("ba_schur_atomics", atomics)
    try:
        S, g, cost = ctx.ba_linearize(_arr(vsl, p), use_huber=p.use_huber, huber=p.huber)
    finally:
        ctx.set_diagnostic("ba_schur_atomics", 0)
    _check_system(name, S, g, cost, ref.reference(name), "atomics" if atomics else "gather")


@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
@pytest.mark.parametrize("name", SMALL)
def test_fused_system(ctx, vsl, name, inv_radius):
    p = ref.cases()[name]
    out = ctx.ba_fused_system(_arr(vsl, p), inv_radius, use_huber=p.use_huber, huber=p.huber)
    if name in FUSED_DECLINES:
        assert out is None       # a camera seeing a landmark more than once / more than 64 cameras: handled == 0
        return
    assert out is not None and out["n_free"] == p.n_free
    R = ref.reference(name, inv_radius)
    n = 6 * p.n_free
    D = R.D[:n]
    kD = float((np.abs(out["scale_c"] - D) / (U * D)).max())
    print("%s 1/radius %g: scale_c %.3g" % (name, inv_radius, kD))
    assert kD * U <= ref.K_GPU * U + ref.jac_tol(name)
    _check_system(name, out["S"], out["rhs"], out["cost"], R, "fused 1/radius %g" % inv_radius)
    assert np.array_equal(out["S"][np.tril_indices(n, -16)], out["S"].T[np.tril_indices(n, -16)])
    # (at 1 / radius = 0 the reference's S and g ARE D_c S D_c and D_c g of the plain system: test_ba_ref_cpu.py)
    # dc: at 1 / radius = 1e-4 on EVERY case; undamped only where two fixed cameras pin the scale (the rig problems
    # and the windows with one fixed camera have a singular S there: the reference's own Cholesky fails or cond ~ 1e16)
    solvable = R.dc is not None and 64 * R.cond_S * U < 1e-3
    assert solvable == (inv_radius > 0 or name in DC_UNDAMPED), (name, R.cond_S)
    if solvable:
        assert out["chol_ok"] == 1
        e = float(np.abs(out["dc"] - R.dc).max() / np.abs(R.dc).max())
        print("%s 1/radius %g: dc %.3g (bound %.3g, cond %.3g)" % (name, inv_radius, e, 64 * R.cond_S * U, R.cond_S))
        assert e <= 64 * R.cond_S * U


def test_fused_plan_declines_65_cameras(ctx, vsl):
    p = ref.cases()["structure/cams65"]
    assert ctx.ba_fused_system(_arr(vsl, p), 1e-4) is None
    p = ref.cases()["structure/cams64"]
    assert ctx.ba_fused_system(_arr(vsl, p), 1e-4) is not None


@pytest.mark.parametrize("name", SMALL + ["structure/n22"])
def test_recompute_form_entry_by_entry(ctx, vsl, name):
    # ba_large.h through vsl_ba_schur_apply: column j of S is S e_j, every case (up to 132 calls)
    p, R = ref.cases()[name], ref.reference(name)
    n = 6 * p.n_free
    arr = _arr(vsl, p)
    S = np.stack([ctx.ba_schur_apply(arr, np.eye(n)[j], use_huber=p.use_huber, huber=p.huber) for j in range(n)], axis=1)
    k = ref.ratio(S, R.S, R.A_S)
    print("%s schur_apply: S %.3g (bound %.3g)" % (name, k, ref.K_GPU))
    assert k <= ref.K_GPU


@pytest.mark.parametrize("name,route", [("structure/n8", "fused"), ("structure/n8", "ba_no_fused"), ("structure/n22", "large"),
                                        ("obs/kb4/ratio1e-12", "fused"), ("obs/ds/angle85", "fused"), ("huber/on", "fused")])
def test_first_step(ctx, vsl, name, route):
    p = ref.cases()[name]
    poses, points, step_c, step_l, c0, c1, R = ref.lm_step(p, 1e-4)
    assert c1 < c0                       # the reference's step lowers the cost: the solver has to accept it
    arr = _arr(vsl, p)
    ctx.set_diagnostic("ba_no_fused", int(route == "ba_no_fused"))
    try:
        s = ctx.bundle_adjust(arr, use_huber=p.use_huber, huber=p.huber, max_iters=1)
    finally:
        ctx.set_diagnostic("ba_no_fused", 0)
    assert (s.iterations, s.successful_steps) == (1, 1)
    assert abs(s.initial_cost - c0) <= ref.COST_GPU * c0
    tol = 64 * R.cond_H * U
    free = p.cam_fixed == 0
    q = arr.poses.copy()
    q[np.sum(q[:, :4] * poses[:, :4].astype(np.float64), axis=1) < 0, :4] *= -1
    ep = float(np.abs(q - poses).max() / np.abs(step_c).max())
    el = float(np.abs(arr.points - points).max() / np.abs(step_l).max())
    print("%s %s: poses %.3g, points %.3g of the step (bound %.3g, cond %.3g); cost %.6g -> %.6g" % (name, route, ep, el, tol, R.cond_H, c0, c1))
    assert tol < 1e-3 and ep <= tol and el <= tol
    assert np.array_equal(arr.poses[~free], p.poses[~free])
    assert abs(s.final_cost - c1) <= max(ref.COST_GPU, tol) * c0
