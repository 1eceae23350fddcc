"""GPU: the rig MAP route (ba_rig.hip: vsl_global_bundle_adjust_rig, vsl_ba_rig_map_system -- the reduced body system
gathered over co-visible body pairs, stored dense / band / cyclic band, solved by the band and ring Cholesky) on the case
table of tests/ba_rig_map_cases.py: against the long-double reference tests/ba_rig_ref.py, against the dense route
(vsl_ba_rig_system, vsl_bundle_adjust_rig: unchanged code), and as a solver.

Tolerances (those of test_ba_rig_gpu.py):
  S, rhs     entrywise |x - x_ref| <= K * 2^-52 * A, A the reference's magnitudes (in the scaled variables A carries the
             scaling).  K = ba_rig_map_cases.k_gpu(case): 8 x the CPU oracle's fold-vs-reference figure, capped at 64 --
             test_ba_rig_map_plan_cpu.py measures that figure on these cases (13.10 at worst, so K = 64; `small` is a
             case of ba_rig_ref and keeps K_RIG_GPU = 24)
  scale_b    (K * 2^-52 + jac_tol) relative
  cost       ba_ref.COST_GPU relative
  db         64 * cond(S') * 2^-52 * max|db_ref|
  solve      against vsl_bundle_adjust_rig by the bar of test_bundle_adjust_matches_oracle: same iterations, termination
             and successful steps; final cost to 1e-7 relative; bodies and points to 1e-6
Each test prints its figures (`pytest -s`)."""
import hashlib

import numpy as np
import pytest

import ba_ref
import ba_rig_map_cases as mc
import ba_rig_ref as ref

pytestmark = pytest.mark.gpu

U = ba_ref.U
NAMES = sorted(mc.cases())


def _arrays(vsl, rp):
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr, rp.points, rp.obs_camera,
                       rp.obs_lm, rp.obs_uv, rp.cam_model)
    return arr, vsl.RigArrays(rp.poses, rp.cam_fixed, rp.cam_body, rp.T_b_c)


def _jac_tol(name):
    return min(max(8.0 * ba_ref.ORACLE_VS_REF_JAC, 10.0 * mc.reference(name).fd_disagreement), 1e-9)


@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
@pytest.mark.parametrize("name", NAMES)
def test_system_against_the_reference(ctx, vsl, name, inv_radius):
    rp = mc.cases()[name]
    arr, rig = _arrays(vsl, rp)
    out = ctx.ba_rig_map_system(arr, rig, inv_radius, use_huber=rp.use_huber, huber=rp.huber)
    assert ctx.last_ba_layout()[1] == mc.EXPECT_FORM[name]
    R = mc.reference(name, inv_radius)
    K = mc.k_gpu(name)
    n = 6 * rp.n_free
    D = R.D[:n]
    kD = float((np.abs(out["scale_b"] - D) / (U * D)).max())
    kS, kg = ba_ref.ratio(out["S"], R.S, R.A_S), ba_ref.ratio(out["rhs"], R.g, R.A_g)
    ce = abs(out["cost"] - R.cost) / R.cost
    print("%s 1/radius %g: S %.3g, rhs %.3g (bound %.3g); scale_b %.3g; cost %.3g (bound %.3g)" %
          (name, inv_radius, kS, kg, K, kD, ce, ba_ref.COST_GPU))
    assert kD * U <= K * U + _jac_tol(name)
    assert kS <= K and kg <= K, (name, kS, kg)
    assert ce <= ba_ref.COST_GPU
    assert np.array_equal(out["S"], out["S"].T)
    assert np.array_equal(rig.body_poses, rp.poses) and np.array_equal(arr.points, rp.points)      # nothing is optimised
    # db where the reference's own system is solvable (the rule of test_scaled_system): everywhere but the undamped systems
    # of the `open` family and ring_narrow, whose thinnest bodies see one landmark (cond ~ 1e17)
    solvable = R.dc is not None and 64 * R.cond_S * U < 1e-3
    assert solvable == (inv_radius > 0 or name not in ("open", "open_edges", "open_huber_models", "open_long_body", "ring_narrow")), (name, R.cond_S)
    if solvable:
        assert out["chol_ok"] == 1
        bound = 64 * R.cond_S * U
        e = float(np.abs(out["db"] - R.dc).max() / np.abs(R.dc).max())
        print("%s 1/radius %g: db %.3g (bound %.3g, cond %.3g)" % (name, inv_radius, e, bound, R.cond_S))
        assert e <= bound


@pytest.mark.parametrize("name", NAMES)
def test_same_system_as_the_dense_route(ctx, vsl, name):
    """Entry by entry under the device bound (not bit for bit: a renumbered pair computes the transposed product).  What
    the band does not hold is an exact zero in both."""
    rp = mc.cases()[name]
    arr, rig = _arrays(vsl, rp)
    m = ctx.ba_rig_map_system(arr, rig, 1e-4, use_huber=rp.use_huber, huber=rp.huber)
    d = ctx.ba_rig_system(arr, rig, 1e-4, use_huber=rp.use_huber, huber=rp.huber)
    R = mc.reference(name, 1e-4)
    K = mc.k_gpu(name)
    kS, kg = ba_ref.ratio(m["S"], d["S"], R.A_S), ba_ref.ratio(m["rhs"], d["rhs"], R.A_g)
    print("%s: map vs dense route: S %.3g, rhs %.3g (bound %.3g)" % (name, kS, kg, K))
    assert kS <= K and kg <= K
    assert np.array_equal(m["S"] == 0.0, d["S"] == 0.0)
    # upstream of the gather: the same kernels on the same per-body sums (the cost adds its 256-observation partials in
    # the sorted order, which follows the slots)
    assert np.array_equal(m["scale_b"], d["scale_b"]) and abs(m["cost"] - d["cost"]) <= ba_ref.COST_GPU * d["cost"]


def _digest(rig, arr):
    h = hashlib.sha256()
    for a in (rig.body_poses, arr.points, arr.poses):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _solve(vsl, c, name, call="global_bundle_adjust_rig", **kw):
    rp = mc.cases()[name]
    arr, rig = _arrays(vsl, rp)
    s = getattr(c, call)(arr, rig, use_huber=rp.use_huber, huber=rp.huber, **kw)
    return s, arr, rig


@pytest.mark.parametrize("name", mc.SOLVE_CASES)
def test_solve_matches_the_dense_route(ctx, vsl, name):
    m, ma, mr = _solve(vsl, ctx, name, max_iters=mc.SOLVE_MAX_ITERS[name])
    form = ctx.last_ba_layout()[1]
    d, da, dr = _solve(vsl, ctx, name, "bundle_adjust_rig", max_iters=mc.SOLVE_MAX_ITERS[name])
    print("%s (form %d): map %d iterations, %d successful, termination %d, cost %.12g -> %.12g; dense %d, %d, %d, %.12g -> %.12g" %
          (name, form, m.iterations, m.successful_steps, m.termination, m.initial_cost, m.final_cost, d.iterations,
           d.successful_steps, d.termination, d.initial_cost, d.final_cost))
    assert form == mc.EXPECT_FORM[name]
    assert d.termination == 1 and d.successful_steps >= 1          # the dense route stops on the function tolerance
    assert (m.iterations, m.successful_steps, m.termination) == (d.iterations, d.successful_steps, d.termination)
    assert abs(m.initial_cost - d.initial_cost) <= 1e-7 * d.initial_cost and abs(m.final_cost - d.final_cost) <= 1e-7 * d.final_cost
    eb, ep = np.abs(mr.body_poses - dr.body_poses).max(), np.abs(ma.points - da.points).max()
    print("%s: bodies %.3g, points %.3g, cameras %.3g" % (name, eb, ep, np.abs(ma.poses - da.poses).max()))
    assert eb <= 1e-6 and ep <= 1e-6 and np.abs(ma.poses - da.poses).max() <= 1e-6


def test_two_solves_give_the_same_bits_and_the_constraint_holds(ctx, vsl):
    rp = mc.cases()["ring_cyclic"]
    out = []
    for _ in range(2):
        s, arr, rig = _solve(vsl, ctx, "ring_cyclic")
        out.append((_digest(rig, arr), s.iterations, s.final_cost))
    print("ring_cyclic: %d iterations, cost %.9g, sha256 %s" % (out[0][1], out[0][2], out[0][0]))
    assert ctx.last_ba_layout()[1] == 2 and out[0][1] >= 1 and s.final_cost < s.initial_cost
    assert out[0] == out[1]
    want = rp.cameras(rig.body_poses)
    worst = 0.0
    for c in range(len(rp.cam_body)):
        tn = float(np.linalg.norm(arr.poses[c, 4:]))
        et = float(np.abs(arr.poses[c, 4:] - want[c, 4:]).max()) / np.spacing(tn)
        sign = 1.0 if float(np.dot(arr.poses[c, :4], want[c, :4].astype(np.float64))) > 0 else -1.0
        eq = float(np.abs(sign * arr.poses[c, :4] - want[c, :4]).max()) / np.spacing(1.0)
        worst = max(worst, et, eq)
    print("worst camera-vs-body*extrinsic error: %.2f ulp" % worst)
    assert worst <= 4.0
    fixed = rp.cam_fixed != 0
    assert np.array_equal(rig.body_poses[fixed], rp.poses[fixed]) and not np.array_equal(rig.body_poses[~fixed], rp.poses[~fixed])


def test_storage_is_defined_by_every_build(ctx, vsl):
    """The solver destroys S in place and the arena is the context's: a cyclic solve, then the open trajectory on the same
    context, whose band lies over what the ring's factorisation left.  Bit for bit a fresh context's result."""
    _solve(vsl, ctx, "ring_cyclic")
    s1, a1, r1 = _solve(vsl, ctx, "open")
    assert ctx.last_ba_layout()[1] == 1
    fresh = vsl.Context(0)
    try:
        s2, a2, r2 = _solve(vsl, fresh, "open")
    finally:
        fresh.close()
    assert (s1.iterations, s1.final_cost) == (s2.iterations, s2.final_cost) and s1.iterations >= 1
    assert _digest(r1, a1) == _digest(r2, a2)


@pytest.mark.parametrize("name", NAMES)
def test_layout(ctx, vsl, name):
    _solve(vsl, ctx, name, max_iters=1)
    elems, form, bw = ctx.last_ba_layout()
    n = 6 * mc.cases()[name].n_free
    print("%s: form %d, bandwidth %d, %d doubles of S" % (name, form, bw, elems))
    assert form == mc.EXPECT_FORM[name]
    if form == 0:
        assert (elems, bw) == (n * n, n)
    else:
        assert elems == n * (bw + 33) + 64 and bw < n
    if name == "open":
        assert bw == 17
    if name == "ring_cyclic":
        assert bw == 29
        ctx.set_diagnostic("ba_no_cyclic", 1)
        try:
            _solve(vsl, ctx, name, max_iters=1)
            assert ctx.last_ba_layout()[1] == 1
        finally:
            ctx.set_diagnostic("ba_no_cyclic", 0)


def _expect_invalid(vsl, ctx, arr, rig, code=-1):
    keep = (rig.body_poses.copy(), arr.points.copy(), arr.poses.copy())
    for call in (lambda: ctx.global_bundle_adjust_rig(arr, rig), lambda: ctx.ba_rig_map_system(arr, rig, 1e-4)):
        with pytest.raises(vsl.VslError) as e:
            call()
        assert e.value.code == code
        assert np.array_equal(rig.body_poses, keep[0]) and np.array_equal(arr.points, keep[1]) and np.array_equal(arr.poses, keep[2])


def test_invalid_inputs(ctx, vsl):
    """The codes of vsl_bundle_adjust_rig (test_ba_rig_gpu.py test_invalid_inputs), case by case."""
    rp = mc.cases()["small"]
    arr, rig = _arrays(vsl, rp)
    rig.cam_body[3] = 3                                   # out of range
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)
    rig.cam_body[3] = -1
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)                           # a fourth body that carries no camera
    rig = vsl.RigArrays(np.vstack([rp.poses, rp.poses[:1]]), [1, 0, 0, 0], rp.cam_body, rp.T_b_c)
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)                           # the two cameras of body 1 on one intrinsics block
    arr.cam_intr[3] = 0
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)                           # no free body
    rig.body_fixed[:] = 1
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)                           # an empty problem
    arr.obs_cam, arr.obs_lm, arr.obs_uv = arr.obs_cam[:0].copy(), arr.obs_lm[:0].copy(), arr.obs_uv[:0].copy()
    _expect_invalid(vsl, ctx, arr, rig)
    arr, rig = _arrays(vsl, rp)
    with pytest.raises(vsl.VslError) as e:
        ctx.ba_rig_map_system(arr, rig, -1.0)
    assert e.value.code == -1
    C = vsl.C
    st, rg = ctx._ba_rig_structs(*_arrays(vsl, rp))
    o, s = ctx._ba_opts(True, 1.0, 20, 0), vsl.BaSummary()
    assert ctx.L.vsl_global_bundle_adjust_rig(ctx.h, C.byref(st), None, C.byref(o), C.byref(s)) == -1
    assert ctx.L.vsl_global_bundle_adjust_rig(ctx.h, None, C.byref(rg), C.byref(o), C.byref(s)) == -1
    assert ctx.L.vsl_global_bundle_adjust_rig(ctx.h, C.byref(st), C.byref(rg), None, C.byref(s)) == -1
    rg.T_b_c = None
    assert ctx.L.vsl_global_bundle_adjust_rig(ctx.h, C.byref(st), C.byref(rg), C.byref(o), C.byref(s)) == -1


def test_gauge_free_problem(ctx, vsl):
    rp = mc.cases()["open"]
    arr, rig = _arrays(vsl, rp)
    rig.body_fixed[:] = 0
    with pytest.raises(vsl.VslError) as e:
        ctx.ba_rig_map_system(arr, rig, 0.0)
    assert e.value.code == -7
    assert np.array_equal(rig.body_poses, rp.poses)
    s = ctx.global_bundle_adjust_rig(arr, rig)
    print("gauge-free solve: %d iterations, termination %d, cost %.6g -> %.6g" % (s.iterations, s.termination, s.initial_cost, s.final_cost))
    assert np.isfinite(rig.body_poses).all() and np.isfinite(arr.poses).all() and np.isfinite(arr.points).all()
    assert s.final_cost <= s.initial_cost
