"""GPU: the rig-constrained bundle adjustment (ba_rig.hip: vsl_bundle_adjust_rig, vsl_ba_rig_linearize,
vsl_ba_rig_system) against the long-double reference tests/ba_rig_ref.py on its case table, against this library's own
free-camera linearisation folded with A, and as a solver.

Tolerances:
  S, g / rhs   entrywise |x - x_ref| <= K_RIG_GPU * 2^-52 * A (ba_rig_ref.py: 8 x the figure test_ba_rig_ref_cpu.py
               measures for the CPU oracle's fold); in the scaled variables A carries the scaling (ba_ref.py, "fused form")
  scale_b      (K_RIG_GPU * 2^-52 + jac_tol(case)) relative, the rule of test_ba_edges_gpu.py for scale_c
  cost         ba_ref.COST_GPU relative
  db           64 * cond(S') * 2^-52 * max|db_ref|
Each test prints its figures (`pytest -s`)."""
import hashlib

import numpy as np
import pytest

import ba_ref
import ba_rig_ref as ref

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = ba_ref.U
NAMES = sorted(ref.cases())


def _arrays(vsl, rp, bodies=None, points=None):
    """(BaArrays of the cameras, RigArrays).  arr.poses is output only for the rig calls: handed in as zeros."""
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr,
                       rp.points if points is None else points, rp.obs_camera, rp.obs_lm, rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(rp.poses if bodies is None else bodies, rp.cam_fixed, rp.cam_body, rp.T_b_c)
    return arr, rig


def _check_system(name, S, g, cost, R, what):
    kS, kg = ba_ref.ratio(S, R.S, R.A_S), ba_ref.ratio(g, R.g, R.A_g)
    ce = abs(cost - R.cost) / R.cost
    print("%s %s: S %.3g, g %.3g (bound %.3g); cost %.3g (bound %.3g)" % (name, what, kS, kg, ref.K_RIG_GPU, ce, ba_ref.COST_GPU))
    assert kS <= ref.K_RIG_GPU and kg <= ref.K_RIG_GPU, (name, what, kS, kg)
    assert ce <= ba_ref.COST_GPU, (name, what, ce)


@pytest.mark.parametrize("name", NAMES)
def test_linearize_against_the_reference(ctx, vsl, name):
    rp = ref.cases()[name]
    arr, rig = _arrays(vsl, rp)
    S, g, cost = ctx.ba_rig_linearize(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    _check_system(name, S, g, cost, ref.reference(name), "rig linearize")
    assert np.array_equal(S, S.T)
    assert np.array_equal(rig.body_poses, rp.poses) and np.array_equal(arr.points, rp.points)      # nothing is optimised


@pytest.mark.parametrize("name", NAMES)
def test_fold_identity_on_the_device(ctx, vsl, name):
    """S_rig = A^T S_free A with S_free from THIS library's vsl_ba_linearize of the expanded problem: independent of the
    rig reference's numbers except for the magnitudes A_S, A_g of the bound."""
    rp = ref.cases()[name]
    arr, rig = _arrays(vsl, rp)
    S, g, cost = ctx.ba_rig_linearize(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    ex = rp.expanded()
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    S_free, g_free, cost_free = ctx.ba_linearize(exa, use_huber=ex.use_huber, huber=ex.huber)
    A = rp.fold_matrix()
    Sf, gf = A.T @ S_free.astype(LD) @ A, A.T @ g_free.astype(LD)
    # the magnitudes of the bound are those of the FREE system (ba_ref's, of the expanded problem), folded with |A|
    Rf = ba_ref.linearize(ex)
    kS, kg = ba_ref.ratio(S, Sf, np.abs(A).T @ Rf.A_S @ np.abs(A)), ba_ref.ratio(g, gf, np.abs(A).T @ Rf.A_g)
    print("%s: rig vs folded free system: S %.3g, g %.3g (bound %.3g)" % (name, kS, kg, ref.K_RIG_GPU))
    assert kS <= ref.K_RIG_GPU and kg <= ref.K_RIG_GPU
    assert abs(cost - cost_free) <= ba_ref.COST_GPU * cost


@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
@pytest.mark.parametrize("name", NAMES)
def test_scaled_system(ctx, vsl, name, inv_radius):
    rp = ref.cases()[name]
    arr, rig = _arrays(vsl, rp)
    out = ctx.ba_rig_system(arr, rig, inv_radius, use_huber=rp.use_huber, huber=rp.huber)
    R = ref.reference(name, inv_radius)
    n = 6 * rp.n_free
    D = R.D[:n]
    kD = float((np.abs(out["scale_b"] - D) / (U * D)).max())
    print("%s 1/radius %g: scale_b %.3g" % (name, inv_radius, kD))
    assert kD * U <= ref.K_RIG_GPU * U + ref.jac_tol(name)
    _check_system(name, out["S"], out["rhs"], out["cost"], R, "rig system 1/radius %g" % inv_radius)
    assert np.array_equal(out["S"], out["S"].T)
    # db where the reference's own system is solvable (the rule of test_ba_edges_gpu.py): everywhere but case i undamped,
    # one camera per body with one fixed body -- a monocular window whose scale is free (S singular, cond ~ 1e16)
    solvable = R.dc is not None and 64 * R.cond_S * U < 1e-3
    assert solvable == (inv_radius > 0 or name != "i_identity_single"), (name, R.cond_S)
    if solvable:
        assert out["chol_ok"] == 1
        bound = 64 * R.cond_S * U
        e = float(np.abs(out["db"] - R.dc).max() / np.abs(R.dc).max())
        print("%s 1/radius %g: db %.3g (bound %.3g, cond %.3g)" % (name, inv_radius, e, bound, R.cond_S))
        assert e <= bound


def test_identity_rig_is_the_free_solve(ctx, vsl):
    """Case i: identity extrinsics, one camera per body -- the rig problem IS the free problem; two implementations of
    one LM trajectory."""
    rp = ref.cases()["i_identity_single"]
    arr, rig = _arrays(vsl, rp)
    s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    ex = rp.expanded()
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    f = ctx.bundle_adjust(exa, use_huber=ex.use_huber, huber=ex.huber)
    print("rig: %d iterations, %d successful, termination %d, cost %.12g -> %.12g; free: %d, %d, %d, %.12g -> %.12g" %
          (s.iterations, s.successful_steps, s.termination, s.initial_cost, s.final_cost, f.iterations, f.successful_steps,
           f.termination, f.initial_cost, f.final_cost))
    assert (s.iterations, s.successful_steps, s.termination) == (f.iterations, f.successful_steps, f.termination)
    assert abs(s.final_cost - f.final_cost) <= 1e-7 * f.final_cost and abs(s.initial_cost - f.initial_cost) <= 1e-7 * f.initial_cost
    assert np.abs(rig.body_poses - exa.poses).max() <= 1e-6 and np.abs(arr.poses - exa.poses).max() <= 1e-6
    assert np.abs(arr.points - exa.points).max() <= 1e-6


def _perturbed_base(dt, dr, seed=500, noise=0.5):
    return ref.base_case(name="a_base/perturbed", seed=seed, drift_t=dt, drift_r=dr, noise=noise)


def test_constraint_holds_after_a_solve(ctx, vsl):
    """Start 2 cm / 0.5 degrees off per body.  Every returned camera pose is its body's pose times the extrinsic to 4 ulp
    of the translation norm (and of 1 for the unit quaternion); fixed bodies keep their bits, and so do their cameras:
    prob->poses is output only, so 'unchanged' is against what the call derives from the untouched fixed bodies, i.e. what
    a call with max_iters = 0 returns."""
    rp = _perturbed_base(0.02, np.deg2rad(0.5))
    arr0, rig0 = _arrays(vsl, rp)
    s0 = ctx.bundle_adjust_rig(arr0, rig0, use_huber=rp.use_huber, huber=rp.huber, max_iters=0)
    assert s0.iterations == 0 and np.array_equal(rig0.body_poses, rp.poses)
    arr, rig = _arrays(vsl, rp)
    s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    print("iterations %d, successful %d, termination %d, cost %.6g -> %.6g" % (s.iterations, s.successful_steps, s.termination,
                                                                             s.initial_cost, s.final_cost))
    assert s.successful_steps >= 1 and s.final_cost <= s.initial_cost and s.initial_cost == s0.initial_cost
    want = rp.cameras(rig.body_poses)
    worst = 0.0
    for c in range(len(rp.cam_body)):
        tn = float(np.linalg.norm(arr.poses[c, 4:]))
        et = float(np.abs(arr.poses[c, 4:] - want[c, 4:]).max()) / (np.spacing(tn))
        sign = 1.0 if float(np.dot(arr.poses[c, :4], want[c, :4].astype(np.float64))) > 0 else -1.0
        eq = float(np.abs(sign * arr.poses[c, :4] - want[c, :4]).max()) / np.spacing(1.0)
        worst = max(worst, et, eq)
    print("worst camera-vs-body*extrinsic error: %.2f ulp" % worst)
    assert worst <= 4.0
    fixed_b = rp.cam_fixed != 0
    fixed_c = fixed_b[rp.cam_body]
    assert fixed_b.any() and np.array_equal(rig.body_poses[fixed_b], rp.poses[fixed_b])
    assert np.array_equal(arr.poses[fixed_c], arr0.poses[fixed_c])
    assert not np.array_equal(rig.body_poses[~fixed_b], rp.poses[~fixed_b])


def test_converges_to_the_rig_optimum(ctx, vsl):
    """Case a, 0.5 px noise: the max-norm of the reference's reduced gradient at the returned point over its value at the
    start, against the same quantity of vsl_bundle_adjust on the expanded free problem (ba_ref's own gradient of that
    problem).  The free figure comes from THIS build's vsl_bundle_adjust, not from a run of the parent's library: that the
    two are the same computation is an inference from no existing kernel or host loop having changed, of which
    test_existing_bundle_adjust_bits pins one other problem bit for bit.  Both stop on the same function
    tolerance: the rig solve may be at most 10 x the free one.  The rig problem is a restriction of the free one, so its
    final cost is not lower."""
    rp = ref.cases()["a_base"]
    g0 = float(np.abs(ref.reference("a_base").g).max())
    arr, rig = _arrays(vsl, rp)
    s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    end = ref.RigProblem(rig.body_poses, rp.cam_fixed, rp.cam_body, rp.cam_intr, rp.T_b_c, rp.intr, arr.points, rp.obs_camera,
                         rp.obs_lm, rp.obs_uv, rp.cam_model, use_huber=rp.use_huber, huber=rp.huber)
    rel_rig = float(np.abs(ref.linearize(end).g).max()) / g0
    ex = rp.expanded()
    f0 = float(np.abs(ba_ref.linearize(ex).g).max())
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    f = ctx.bundle_adjust(exa, use_huber=ex.use_huber, huber=ex.huber)
    ex.poses, ex.points = exa.poses.copy(), exa.points.copy()
    rel_free = float(np.abs(ba_ref.linearize(ex).g).max()) / f0
    print("gradient reduction: rig %.3g (%d iterations, termination %d, cost %.9g), free %.3g (%d, %d, cost %.9g)" %
          (rel_rig, s.iterations, s.termination, s.final_cost, rel_free, f.iterations, f.termination, f.final_cost))
    assert s.termination in (1, 2, 3)
    assert rel_rig <= 10.0 * rel_free
    assert s.final_cost >= f.final_cost * (1 - 1e-9)


def _digest(rig, arr, s):
    h = hashlib.sha256()
    for a in (rig.body_poses, arr.points, np.array([s.final_cost])):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_two_solves_give_the_same_bits(ctx, vsl):
    rp = ref.cases()["h_23_free"]
    out = []
    for _ in range(2):
        arr, rig = _arrays(vsl, rp)
        s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
        out.append((_digest(rig, arr, s), s.iterations, s.final_cost, s.initial_cost))
    print("case h: %d iterations, cost %.6g -> %.6g, sha256 %s" % (out[0][1], out[0][3], out[0][2], out[0][0]))
    assert out[0][1] >= 1 and out[0][2] < out[0][3]
    assert out[0] == out[1]


def _expect_invalid(vsl, ctx, arr, rig, code=-1):
    """All three entry points return `code` and leave bodies, points and poses as they were."""
    keep = (rig.body_poses.copy(), arr.points.copy(), arr.poses.copy())
    for call in (lambda: ctx.bundle_adjust_rig(arr, rig), lambda: ctx.ba_rig_linearize(arr, rig), lambda: ctx.ba_rig_system(arr, rig, 1e-4)):
        with pytest.raises(vsl.VslError) as e:
            call()
        assert e.value.code == code
        assert np.array_equal(rig.body_poses, keep[0]) and np.array_equal(arr.points, keep[1]) and np.array_equal(arr.poses, keep[2])


def test_invalid_inputs(ctx, vsl):
    rp = ref.cases()["a_base"]
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
    # null pointers, at the C ABI
    C = vsl.C
    st, rg = ctx._ba_rig_structs(*_arrays(vsl, rp))
    o, s = ctx._ba_opts(True, 1.0, 20, 0), vsl.BaSummary()
    assert ctx.L.vsl_bundle_adjust_rig(ctx.h, C.byref(st), None, C.byref(o), C.byref(s)) == -1
    assert ctx.L.vsl_bundle_adjust_rig(ctx.h, None, C.byref(rg), C.byref(o), C.byref(s)) == -1
    assert ctx.L.vsl_bundle_adjust_rig(ctx.h, C.byref(st), C.byref(rg), None, C.byref(s)) == -1
    arr, rig = _arrays(vsl, rp)
    st, rg = ctx._ba_rig_structs(arr, rig)
    rg.T_b_c = None
    assert ctx.L.vsl_bundle_adjust_rig(ctx.h, C.byref(st), C.byref(rg), C.byref(o), C.byref(s)) == -1
    assert ctx.L.vsl_ba_rig_linearize(ctx.h, C.byref(st), C.byref(rg), C.byref(o), None, None, None, None) == -1
    assert np.array_equal(rig.body_poses, rp.poses)


def test_gauge_free_problem(ctx, vsl):
    rp = ref.cases()["a_base"]
    arr, rig = _arrays(vsl, rp)
    rig.body_fixed[:] = 0
    for call in (lambda: ctx.ba_rig_linearize(arr, rig), lambda: ctx.ba_rig_system(arr, rig, 0.0)):
        with pytest.raises(vsl.VslError) as e:
            call()
        assert e.value.code == -7
    assert np.array_equal(rig.body_poses, rp.poses)
    s = ctx.bundle_adjust_rig(arr, rig)
    print("gauge-free solve: %d iterations, termination %d, cost %.6g -> %.6g" % (s.iterations, s.termination, s.initial_cost, s.final_cost))
    assert np.isfinite(rig.body_poses).all() and np.isfinite(arr.poses).all() and np.isfinite(arr.points).all()
    assert s.final_cost <= s.initial_cost


# vsl_bundle_adjust on synth.ba_problem(3, n_lms=2000), default path and "ba_no_fused": SHA-256 over poses, points and
# final cost, computed with the library built from the parent commit on an MI355X.  No existing kernel or host loop
# changes with the rig solver: the bits stay.
PARENT_SHA = {"fused": "b20c38af8fed21f4fe74f14aee7c388948a56faa3f1e0e049631bd22a7f79b46",
              "no_fused": "32e995818d88423fd2392b4982c242cbcbbf006e788f5749a6c74d16bed151f7"}


@pytest.mark.parametrize("route", ["fused", "no_fused"])
def test_existing_bundle_adjust_bits(ctx, vsl, synth, route):
    arr = vsl.BaArrays.from_dict(synth.ba_problem(3, n_lms=2000))
    ctx.set_diagnostic("ba_no_fused", 1 if route == "no_fused" else 0)
    try:
        s = ctx.bundle_adjust(arr)
    finally:
        ctx.set_diagnostic("ba_no_fused", 0)
    h = hashlib.sha256()
    for a in (arr.poses, arr.points, np.array([s.final_cost])):
        h.update(np.ascontiguousarray(a).tobytes())
    print("bundle_adjust %s: sha256 %s" % (route, h.hexdigest()))
    assert h.hexdigest() == PARENT_SHA[route]


# ------------------------------------------------------------------------------------------ parent-commit pins (rig)
# SHA-256 values computed with the library built from the parent commit on an MI355X.  The rig chain now runs on
# ba.hip's shared kernels and on the one host LM loop of lm_policy.h; the arithmetic and its order are the parent's, so
# every bit stays.  Each test prints its digest (`pytest -s`).
def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _solve_digest(ctx, vsl, rp, **kw):
    arr, rig = _arrays(vsl, rp)
    s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber, **kw)
    return _sha(rig.body_poses, arr.points, arr.poses, np.array([s.final_cost]), np.array([s.iterations], np.int64)), s


def _system_digest(ctx, vsl, rp):
    arr, rig = _arrays(vsl, rp)
    out = ctx.ba_rig_system(arr, rig, 1e-4, use_huber=rp.use_huber, huber=rp.huber)
    return _sha(out["S"], out["rhs"], out["scale_b"], out["db"], np.array([out["cost"]]))


_MULTI = []


def _multi_segment():
    """3 bodies x 2 cameras x 600 landmarks, everything seen by everything: 3600 observations, 1200 per body -- three
    segments per body in the body-block sum, two per block in the Schur gather, 15 observation workgroups, 3 update
    workgroups.  No long-double reference: a parent-bits pin only."""
    if not _MULTI:
        _MULTI.append(ref.rig_scene(3, 1, 600, 509))
    return _MULTI[0]


PARENT_RIG_SOLVE = {"a_base": "748f1a0e6c16c471070bf901e6eba85f5f9d51826999937b3801f6627b0e6894",
                    "g_huber_outliers": "6ec40faefa184110913a39475362734bbca922c7ad78d40d932e8e1ee632f06c",
                    "h_23_free": "8498a21a92239697c03edd1ae3239f16b16ecf5569bde47d450c2a8136a8d07f"}
PARENT_RIG_SYSTEM = {"a_base": "05e12a7cacaf28fc10f40f6977574482e80f71c8226ac345632163d5eaab2c6d",
                     "h_23_free": "86399a26cf2a8690c6652c404c7853671fd94fb583ecb422d7a09d3237d56f09"}
PARENT_RIG_MULTI = {"system": "bc0630cca3c0e2097aabd2c3ab363aa7fc2adc3783ef821f4add5e51dac1a85d",
                    "solve5": "1cd3bbcb1ff8af1799555dc80b0299d6c1b128ba2c943b00084d67ce83cbad45"}
PARENT_RIG_COV = "5b12b0e8b513573658714f6d32d06221a086cbff4c3b8891641f8bec052f26ca"


@pytest.mark.parametrize("name", sorted(PARENT_RIG_SOLVE))
def test_rig_solve_parent_bits(ctx, vsl, name):
    d, s = _solve_digest(ctx, vsl, ref.cases()[name])
    print("bundle_adjust_rig %s: %d iterations, termination %d, sha256 %s" % (name, s.iterations, s.termination, d))
    assert s.iterations >= 1
    assert d == PARENT_RIG_SOLVE[name]


@pytest.mark.parametrize("name", sorted(PARENT_RIG_SYSTEM))
def test_rig_system_parent_bits(ctx, vsl, name):
    d = _system_digest(ctx, vsl, ref.cases()[name])
    print("ba_rig_system %s 1/radius 1e-4: sha256 %s" % (name, d))
    assert d == PARENT_RIG_SYSTEM[name]


def test_rig_multi_segment_parent_bits(ctx, vsl):
    rp = _multi_segment()
    assert len(rp.obs_lm) == 3600 and np.array_equal(np.bincount(rp.cam_body[rp.obs_camera]), [1200, 1200, 1200])
    d_sys = _system_digest(ctx, vsl, rp)
    d_solve, s = _solve_digest(ctx, vsl, rp, max_iters=5)
    print("multi-segment: ba_rig_system sha256 %s; 5-iteration solve (%d iterations, termination %d, cost %.9g -> %.9g) sha256 %s" %
          (d_sys, s.iterations, s.termination, s.initial_cost, s.final_cost, d_solve))
    assert s.iterations >= 1
    assert d_sys == PARENT_RIG_MULTI["system"]
    assert d_solve == PARENT_RIG_MULTI["solve5"]


def test_rig_covariance_parent_bits(ctx, vsl):
    rp = ref.cases()["a_base"]
    arr, rig = _arrays(vsl, rp)
    cams = np.flatnonzero(rp.cam_fixed[rp.cam_body] == 0)                       # (a camera of a fixed body has no block)
    cb, cc, cl, nd = ctx.ba_rig_covariance(arr, rig, cams=cams, lms=np.arange(len(rp.points)), use_huber=rp.use_huber, huber=rp.huber)
    d = _sha(cb, cc, cl)
    print("ba_rig_covariance a_base: %d body, %d camera, %d point blocks, %d degenerate, sha256 %s" % (len(cb), len(cc), len(cl), nd, d))
    assert len(cb) == rp.n_free and nd == 0
    assert d == PARENT_RIG_COV
