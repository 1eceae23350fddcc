"""GPU: the rig bundle adjustment with the extrinsics as unknowns (ba_rig.hip "EXTRINSICS": vsl_bundle_adjust_rig_ext,
vsl_ba_rig_ext_linearize, vsl_ba_rig_ext_system) against the long-double reference tests/ba_rig_ext_ref.py on its case
table, against this library's own free-camera linearisation folded with A, and as a solver.

Tolerances (the rules of test_ba_rig_gpu.py):
  S, g / rhs   entrywise |x - x_ref| <= K_EXT_GPU * 2^-52 * A (ba_rig_ext_ref.py: 8 x the figure
               test_ba_rig_ext_ref_cpu.py measures for the CPU oracle's fold)
  scale        (K_EXT_GPU * 2^-52 + jac_tol(case)) relative
  cost         ba_ref.COST_GPU relative
  d            64 * cond(S') * 2^-52 * max|d_ref| where the reference calls the system solvable
  parameters   1e-6: one LM problem reached two ways
Each test prints its figures (`pytest -s`)."""
import hashlib

import numpy as np
import pytest

import ba_ref
import ba_rig_ref
import ba_rig_ext_ref as ref
from pgo_ref import _ld, se3_mul

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = ba_ref.U
NAMES = sorted(ref.cases())


def _arrays(vsl, xp, bodies=None, points=None, T_b_c=None):
    """(BaArrays of the cameras, RigArrays whose T_b_c is NaN: the calls must not read it, the extrinsics [2, 7])."""
    rp = xp.rp
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr,
                       rp.points if points is None else points, rp.obs_camera, rp.obs_lm, rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(rp.poses if bodies is None else bodies, rp.cam_fixed, rp.cam_body, np.full((2, 7), np.nan))
    return arr, rig, np.array(rp.T_b_c if T_b_c is None else T_b_c, np.float64).reshape(2, 7).copy()


def _kw(xp):
    return dict(ext_free=xp.ext_free, use_huber=xp.rp.use_huber, huber=xp.rp.huber)


def _check_system(name, S, g, cost, R, what):
    kS, kg = ba_ref.ratio(S, R.S, R.A_S), ba_ref.ratio(g, R.g, R.A_g)
    ce = abs(cost - R.cost) / R.cost
    print("%s %s: S %.3g, g %.3g (bound %.3g); cost %.3g (bound %.3g)" % (name, what, kS, kg, ref.K_EXT_GPU, ce, ba_ref.COST_GPU))
    assert kS <= ref.K_EXT_GPU and kg <= ref.K_EXT_GPU, (name, what, kS, kg)
    assert ce <= ba_ref.COST_GPU, (name, what, ce)


@pytest.mark.parametrize("name", NAMES)
def test_linearize_against_the_reference(ctx, vsl, name):
    xp = ref.cases()[name]
    arr, rig, T = _arrays(vsl, xp)
    S, g, cost = ctx.ba_rig_ext_linearize(arr, rig, T, **_kw(xp))
    assert S.shape == (xp.nt, xp.nt)
    _check_system(name, S, g, cost, ref.reference(name), "ext linearize")
    assert np.array_equal(S, S.T)
    assert np.array_equal(rig.body_poses, xp.rp.poses) and np.array_equal(arr.points, xp.rp.points) and np.array_equal(T, xp.rp.T_b_c)


@pytest.mark.parametrize("name", NAMES)
def test_fold_identity_on_the_device(ctx, vsl, name):
    """S = A^T S_P A with S_P from THIS library's vsl_ba_linearize of P: independent of the reference's numbers except
    for the magnitudes of the bound."""
    xp = ref.cases()[name]
    arr, rig, T = _arrays(vsl, xp)
    S, g, cost = ctx.ba_rig_ext_linearize(arr, rig, T, **_kw(xp))
    ex = xp.expanded()
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    S_free, g_free, cost_free = ctx.ba_linearize(exa, use_huber=ex.use_huber, huber=ex.huber)
    A = xp.fold_matrix()
    Sf, gf = A.T @ S_free.astype(LD) @ A, A.T @ g_free.astype(LD)
    R = ref.reference(name)
    kS, kg = ba_ref.ratio(S, Sf, R.A_S), ba_ref.ratio(g, gf, R.A_g)
    print("%s: ext vs folded free system: S %.3g, g %.3g (bound %.3g)" % (name, kS, kg, ref.K_EXT_GPU))
    assert kS <= ref.K_EXT_GPU and kg <= ref.K_EXT_GPU
    assert abs(cost - cost_free) <= ba_ref.COST_GPU * cost


@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
@pytest.mark.parametrize("name", NAMES)
def test_scaled_system(ctx, vsl, name, inv_radius):
    xp = ref.cases()[name]
    arr, rig, T = _arrays(vsl, xp)
    out = ctx.ba_rig_ext_system(arr, rig, T, inv_radius, **_kw(xp))
    R = ref.reference(name, inv_radius)
    n = xp.nt
    assert out["scale"].shape == (n,) and out["d"].shape == (n,)
    D = R.D[:n]
    kD = float((np.abs(out["scale"] - D) / (U * D)).max())
    print("%s 1/radius %g: scale %.3g" % (name, inv_radius, kD))
    assert kD * U <= ref.K_EXT_GPU * U + ref.jac_tol(name)
    _check_system(name, out["S"], out["rhs"], out["cost"], R, "ext system 1/radius %g" % inv_radius)
    assert np.array_equal(out["S"], out["S"].T)
    solvable = R.dc is not None and 64 * R.cond_S * U < 1e-3
    # everywhere but the gauge case undamped: one fixed body, the baseline's length is free (S singular)
    assert solvable == (inv_radius > 0 or name not in ref.GAUGE_CASES), (name, R.cond_S)
    if solvable:
        assert out["chol_ok"] == 1
        bound = 64 * R.cond_S * U
        e = float(np.abs(out["d"] - R.dc).max() / np.abs(R.dc).max())
        print("%s 1/radius %g: d %.3g (bound %.3g, cond %.3g)" % (name, inv_radius, e, bound, R.cond_S))
        assert e <= bound
    else:
        print("%s 1/radius %g: gauge: chol_ok %d, cond %.3g" % (name, inv_radius, out["chol_ok"], R.cond_S))
        assert out["chol_ok"] == 0 or np.isfinite(out["d"]).all()


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.parametrize("name", ["a_base", "j_22_free"])
def test_no_free_block_is_the_rig_solve(ctx, vsl, name):
    xp = ref.cases()[name]
    rp = xp.rp
    kw = dict(use_huber=rp.use_huber, huber=rp.huber)
    arr, rig, T = _arrays(vsl, xp)
    T[1, :4] *= 1.7                                             # comes back normalised and otherwise untouched
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, ext_free=(0, 0), **kw)
    arr2, rig2, _ = _arrays(vsl, xp)
    rig2.T_b_c[:] = rp.T_b_c
    rig2.T_b_c[1, :4] *= 1.7
    s2 = ctx.bundle_adjust_rig(arr2, rig2, **kw)
    dig = lambda r, a, q: _sha(r.body_poses, a.points, a.poses, np.array([q.initial_cost, q.final_cost]), np.array([q.iterations], np.int64))
    print("%s: ext_free (0, 0): %d iterations, sha256 %s" % (name, s.iterations, dig(rig, arr, s)))
    assert s.iterations >= 1 and dig(rig, arr, s) == dig(rig2, arr2, s2)
    want = rig2.T_b_c.copy()
    want[1, :4] /= np.sqrt(np.sum(want[1, :4] ** 2))
    want[0, :4] /= np.sqrt(np.sum(want[0, :4] ** 2))
    assert np.array_equal(T, want)
    # the two hooks
    arr, rig, T = _arrays(vsl, xp)
    rig2.body_poses[:] = rp.poses
    rig2.T_b_c[:] = rp.T_b_c
    arr2, _, _ = _arrays(vsl, xp)
    a, b = ctx.ba_rig_ext_linearize(arr, rig, T, ext_free=(0, 0), **kw), ctx.ba_rig_linearize(arr2, rig2, **kw)
    assert _sha(a[0], a[1], np.array([a[2]])) == _sha(b[0], b[1], np.array([b[2]]))
    a, b = ctx.ba_rig_ext_system(arr, rig, T, 1e-4, ext_free=(0, 0), **kw), ctx.ba_rig_system(arr2, rig2, 1e-4, **kw)
    assert _sha(a["S"], a["rhs"], a["scale"], a["d"], np.array([a["cost"]])) == _sha(b["S"], b["rhs"], b["scale_b"], b["db"], np.array([b["cost"]]))
    assert a["chol_ok"] == b["chol_ok"] == 1


# ------------------------------------------------------------------------------------------------------ the solver
_REC = {}


def _recovery_scene(noise):
    """(the scene handed in: base scene at `noise` px, bodies and points with the scene's own drift, extrinsic block 1 moved
    by exp((5 mm u, 0.3 deg w)); the true bodies; the true extrinsics)."""
    if noise not in _REC:
        rp = ref.base_scene(noise=noise)
        true = ref.base_scene(noise=noise, drift_t=0.0, drift_r=0.0)      # the same draws, nothing moved
        assert np.array_equal(true.obs_uv, rp.obs_uv) and np.array_equal(true.T_b_c, rp.T_b_c)
        xp = ref.ExtProblem(rp, (0, 1), "a_base/recovery").with_state(T_b_c=ref.perturbed_extrinsic(rp.T_b_c))
        _REC[noise] = (xp, true.poses.copy(), rp.T_b_c.copy())
    return _REC[noise]


def _pose_err(a, b):
    """max |a - b| over poses, quaternions compared up to sign"""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64).reshape(-1, 7)
    sign = np.where(np.sum(a[:, :4] * b[:, :4], axis=1) < 0, -1.0, 1.0)[:, None]
    return float(max(np.abs(sign * a[:, :4] - b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max()))


def test_recovers_the_extrinsic(ctx, vsl):
    xp, true_bodies, true_T = _recovery_scene(0.0)
    arr, rig, T = _arrays(vsl, xp)
    start = _pose_err(T, true_T)
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, **_kw(xp))
    eT, eB = _pose_err(T, true_T), _pose_err(rig.body_poses, true_bodies)
    print("recovery: %d iterations, %d successful, termination %d, cost %.6g -> %.6g; extrinsic error %.3g -> %.3g, bodies %.3g" %
          (s.iterations, s.successful_steps, s.termination, s.initial_cost, s.final_cost, start, eT, eB))
    assert s.termination in (1, 2, 3)
    assert eT <= 1e-6 and eB <= 1e-6
    assert np.array_equal(T[0], true_T[0])                                    # the held block keeps its bits
    want = se3_mul(_ld(rig.body_poses)[xp.rp.cam_body], _ld(T)[xp.rp.cam_intr]).astype(np.float64)
    assert _pose_err(arr.poses, want) <= 1e-12


def test_ordering_of_optima(ctx, vsl):
    """final(free solve of P) <= final(rig_ext) <= final(rig at the perturbed extrinsic), each a restriction of the one before."""
    xp, _, _ = _recovery_scene(0.5)
    rp = xp.rp
    kw = dict(use_huber=rp.use_huber, huber=rp.huber)
    arr, rig, T = _arrays(vsl, xp)
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, **_kw(xp))
    arr2, rig2, T2 = _arrays(vsl, xp)
    rig2.T_b_c[:] = T2
    r = ctx.bundle_adjust_rig(arr2, rig2, **kw)
    ex = xp.expanded()
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    f = ctx.bundle_adjust(exa, **kw)
    print("final costs: free solve of P %.9g (termination %d), rig_ext %.9g (%d), rig at the perturbed extrinsic %.9g (%d)" %
          (f.final_cost, f.termination, s.final_cost, s.termination, r.final_cost, r.termination))
    assert f.termination in (1, 2, 3) and s.termination in (1, 2, 3) and r.termination in (1, 2, 3)
    assert f.final_cost * (1 - 1e-9) <= s.final_cost <= r.final_cost * (1 + 1e-9)
    assert s.final_cost <= 0.9 * r.final_cost                                # strict by a visible margin


def test_two_solves_give_the_same_bits(ctx, vsl):
    xp = ref.cases()["j_22_free"]
    out = []
    for _ in range(2):
        arr, rig, T = _arrays(vsl, xp)
        s = ctx.bundle_adjust_rig_ext(arr, rig, T, **_kw(xp))
        out.append((_sha(rig.body_poses, arr.points, arr.poses, T, np.array([s.final_cost])), s.iterations, s.final_cost, s.initial_cost))
    print("case j: %d iterations, cost %.6g -> %.6g, sha256 %s" % (out[0][1], out[0][3], out[0][2], out[0][0]))
    assert out[0][1] >= 1 and out[0][2] < out[0][3]
    assert out[0] == out[1]


def test_no_free_body_moves_the_extrinsic_and_the_points_only(ctx, vsl):
    xp = ref.cases()["i_no_free_body"]
    arr, rig, T = _arrays(vsl, xp)
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, **_kw(xp))
    print("no free body: %d iterations, termination %d, cost %.6g -> %.6g" % (s.iterations, s.termination, s.initial_cost, s.final_cost))
    assert s.successful_steps >= 1 and s.final_cost < s.initial_cost
    assert np.array_equal(rig.body_poses, xp.rp.poses) and np.array_equal(T[0], xp.rp.T_b_c[0])
    assert not np.array_equal(T[1], xp.rp.T_b_c[1]) and not np.array_equal(arr.points, xp.rp.points)
    assert np.isfinite(T).all() and np.isfinite(arr.points).all() and np.isfinite(arr.poses).all()


def test_gauge_case_solves(ctx, vsl):
    xp = ref.cases()["l_gauge_one_fixed"]
    arr, rig, T = _arrays(vsl, xp)
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, **_kw(xp))
    print("gauge solve: %d iterations, termination %d, cost %.6g -> %.6g" % (s.iterations, s.termination, s.initial_cost, s.final_cost))
    assert np.isfinite(rig.body_poses).all() and np.isfinite(arr.poses).all() and np.isfinite(arr.points).all() and np.isfinite(T).all()
    assert s.final_cost <= s.initial_cost


def _expect_invalid(vsl, ctx, arr, rig, T, ext_free=(0, 1), code=-1):
    keep = (rig.body_poses.copy(), arr.points.copy(), arr.poses.copy(), T.copy())
    for call in (lambda: ctx.bundle_adjust_rig_ext(arr, rig, T, ext_free=ext_free), lambda: ctx.ba_rig_ext_linearize(arr, rig, T, ext_free=ext_free),
                 lambda: ctx.ba_rig_ext_system(arr, rig, T, 1e-4, ext_free=ext_free)):
        with pytest.raises(vsl.VslError) as e:
            call()
        assert e.value.code == code
        assert np.array_equal(rig.body_poses, keep[0]) and np.array_equal(arr.points, keep[1]) and np.array_equal(arr.poses, keep[2])
        assert np.array_equal(T, keep[3], equal_nan=True)


def test_invalid_inputs(ctx, vsl):
    xp = ref.cases()["a_base"]
    arr, rig, T = _arrays(vsl, xp)
    rig.cam_body[3] = 4                                   # what the rig calls refuse: out of range
    _expect_invalid(vsl, ctx, arr, rig, T)
    arr, rig, T = _arrays(vsl, xp)                        # the two cameras of body 1 on one intrinsics block
    arr.cam_intr[3] = 0
    _expect_invalid(vsl, ctx, arr, rig, T)
    arr, rig, T = _arrays(vsl, xp)                        # a non-finite extrinsic
    T[0, 5] = np.nan
    _expect_invalid(vsl, ctx, arr, rig, T)
    arr, rig, T = _arrays(vsl, xp)
    T[1, :4] = 0
    _expect_invalid(vsl, ctx, arr, rig, T)
    arr, rig, T = _arrays(vsl, xp)                        # no free body and no free block
    rig.body_fixed[:] = 1
    _expect_invalid(vsl, ctx, arr, rig, T, ext_free=(0, 0))
    xs = ref.ExtProblem(ba_rig_ref.rig_scene(3, 2, 9, 650, cams_of_body=[(0,)] * 3), (0, 1))   # a free block that no camera carries
    arr, rig, T = _arrays(vsl, xs)
    _expect_invalid(vsl, ctx, arr, rig, T)
    # null pointers, at the C ABI
    C = vsl.C
    arr, rig, T = _arrays(vsl, xp)
    st, rg = ctx._ba_rig_structs(arr, rig)
    o, s = ctx._ba_opts(True, 1.0, 20, 0), vsl.BaSummary()
    ef = np.array([0, 1], np.uint8)
    f64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    efp, Tp = ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p)
    L = ctx.L
    assert L.vsl_bundle_adjust_rig_ext(ctx.h, C.byref(st), C.byref(rg), None, Tp, C.byref(o), C.byref(s)) == -1
    assert L.vsl_bundle_adjust_rig_ext(ctx.h, C.byref(st), C.byref(rg), efp, None, C.byref(o), C.byref(s)) == -1
    assert L.vsl_bundle_adjust_rig_ext(ctx.h, None, C.byref(rg), efp, Tp, C.byref(o), C.byref(s)) == -1
    assert L.vsl_bundle_adjust_rig_ext(ctx.h, C.byref(st), None, efp, Tp, C.byref(o), C.byref(s)) == -1
    assert L.vsl_bundle_adjust_rig_ext(ctx.h, C.byref(st), C.byref(rg), efp, Tp, None, C.byref(s)) == -1
    assert L.vsl_ba_rig_ext_linearize(ctx.h, C.byref(st), C.byref(rg), efp, Tp, C.byref(o), None, None, None, None, None) == -1
    assert L.vsl_ba_rig_ext_system(ctx.h, C.byref(st), C.byref(rg), None, Tp, C.byref(o), C.c_double(0.0), None, None, None, None, None, None) == -1
    assert L.vsl_ba_rig_ext_system(ctx.h, C.byref(st), C.byref(rg), efp, Tp, C.byref(o), C.c_double(-1.0), None, None, None, None, None, None) == -1
    assert np.array_equal(rig.body_poses, xp.rp.poses) and np.array_equal(T, xp.rp.T_b_c)
