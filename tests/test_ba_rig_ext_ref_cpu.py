"""CPU: pins tests/ba_rig_ext_ref.py (the long-double reference of the rig bundle adjustment with the extrinsics as
unknowns) on every case the GPU tests of test_ba_rig_ext_gpu.py use, with no library code:
  * F_x (ba_ref's camera Jacobian) equals a long-double central difference along T_b_c * exp(eps), to the case's jac_tol;
  * the fold identity A^T S_P A = S, A^T g_P = g with S_P, g_P the long-double reference of the free problem P;
  * with no free block the reference is ba_rig_ref.linearize;
  * the gauge: with one fixed body the analytic scale direction v has |J v| at the finite-difference level; with two
    fixed bodies every case satisfies the solvability rule 64 cond(S') 2^-52 < 1e-3 of test_ba_rig_gpu.py;
  * the tolerance constant: the CPU ORACLE's ba_linearize of P, folded with A in float64 numpy, against the reference,
    entrywise in units of 2^-52 A.  The worst figure is printed (`pytest -s`) and must not exceed
    ba_rig_ext_ref.ORACLE_FOLD_VS_REF_K, which the device tolerance is 8 x of (at most 64)."""
import numpy as np
import pytest

import ba_ref
import ba_rig_ref
import ba_rig_ext_ref as ref
from pgo_ref import LD, _ld, se3_exp, se3_mul

NAMES = ("a_base", "b_both_free", "c_block0_free", "d_fixed_bodies_only", "e_block0_cameras_only", "f_single_camera_body",
         "g_models", "h_huber_outliers", "i_no_free_body", "j_22_free", "k_multi_segment", "l_gauge_one_fixed")


def test_case_table_holds_its_premises():
    C = ref.cases()
    assert tuple(C) == NAMES
    a = C["a_base"]
    assert len(a.rp.poses) == 4 and a.rp.cam_fixed.tolist() == [1, 1, 0, 0] and len(a.rp.points) == 9 and a.ext_free == (0, 1)
    assert len(a.rp.obs_lm) == 8 * 9 - 4 and a.nt == 18
    b = C["b_both_free"]
    assert b.ext_free == (1, 1) and b.nt == 24 and int((b.rp.cam_fixed != 0).sum()) == 3
    assert C["c_block0_free"].ext_free == (1, 0)
    d = C["d_fixed_bodies_only"].rp
    assert set(d.cam_body[d.obs_camera[d.obs_lm == 3]]) == {0, 1}
    e = C["e_block0_cameras_only"].rp
    assert set(e.cam_intr[e.obs_camera[e.obs_lm == 4]]) == {0} and (e.obs_lm == 4).sum() == 4
    assert np.bincount(C["f_single_camera_body"].rp.cam_body).tolist() == [2, 2, 2, 1]
    assert C["g_models"].rp.cam_model == (0, 3)
    h = C["h_huber_outliers"]
    assert ref.reference("h_huber_outliers").outlier[list(h.rp.outliers)].all()
    i = C["i_no_free_body"]
    assert i.n_free_bodies == 0 and i.nt == 6
    j = C["j_22_free"]
    assert j.n_free_bodies == 22 and j.nt == 138 > 128
    k = C["k_multi_segment"]
    sb, se = k.obs_slots()
    assert (sb == 0).sum() == 1040 > 512 and (se == 1).sum() == 1560 > 512 and len(k.rp.points) == 520 > 512
    g = C["l_gauge_one_fixed"]
    assert int((g.rp.cam_fixed != 0).sum()) == 1
    for n, xp in C.items():
        assert np.bincount(xp.rp.obs_lm, minlength=len(xp.rp.points)).min() >= 2
        assert int((xp.rp.cam_fixed != 0).sum()) >= 2 or n in ref.GAUGE_CASES


@pytest.mark.parametrize("name", NAMES)
def test_extrinsic_jacobian_is_a_central_difference_along_the_extrinsic(name):
    """An independent difference quotient (plain central, step h, then h / 2, Richardson) of the residual along
    T_b_c[k] * exp(eps): the composition T_w_b (T_b_c exp(eps)) is formed explicitly, in long double."""
    xp = ref.cases()[name]
    rp = xp.rp
    Fx = ref.reference(name).Fx
    k = rp.cam_intr[rp.obs_camera]
    ip, model = _ld(rp.intr)[k], rp.obs_model()
    X = _ld(rp.points)[rp.obs_lm]
    bodies = _ld(rp.poses)[rp.obs_cam]
    dist = np.sqrt(np.sum(ba_ref.camera_point(rp.cameras()[rp.obs_camera], X) ** 2, axis=-1))
    D = []
    for s in (1, 2):
        cols = []
        for c in range(6):
            h = (LD(rp.fd_step) * dist / s) if c < 3 else np.full(dist.shape, LD(rp.fd_step) / s)
            d = np.zeros(dist.shape + (6,), LD)
            d[..., c] = h
            out = []
            for sign in (1, -1):
                Te = se3_mul(_ld(rp.T_b_c)[k], se3_exp(sign * d))
                out.append(ba_ref.residual(model, ip, se3_mul(bodies, Te), X, rp.obs_uv))
            cols.append((out[0] - out[1]) / (2 * h)[..., None])
        D.append(np.stack(cols, axis=-1))
    J = (4 * D[1] - D[0]) / 3
    err = ba_ref.block_error(Fx, J)
    tol = ref.jac_tol(name)
    print("%s: max |F_x - fd along T_b_c exp(eps)| / max|F_x| = %.3g (tolerance %.3g)" % (name, err.max(), tol))
    assert err.max() <= tol


@pytest.mark.parametrize("name", NAMES)
def test_fold_of_the_reference_of_P(name):
    xp = ref.cases()[name]
    R = ref.reference(name)
    RP = ba_ref.linearize(xp.expanded())
    A = xp.fold_matrix()
    S, g = A.T @ RP.S @ A, A.T @ RP.g
    kS, kg = ba_ref.ratio(S, R.S, R.A_S), ba_ref.ratio(g, R.g, R.A_g)
    print("%s: A^T S_P A vs the reference: S %.3g, g %.3g units of 2^-52 A" % (name, kS, kg))
    # two long-double computations that differ in ONE thing: P's cameras are rounded to double.  The oracle's fold below sees
    # the same rounded P and adds its own double arithmetic, so this figure lies inside the constant measured there
    assert max(kS, kg) <= ref.ORACLE_FOLD_VS_REF_K


def test_no_free_block_is_the_rig_reference():
    rp = ref.cases()["a_base"].rp
    for inv_radius in (None, 1e-4):
        R = ref.linearize(ref.ExtProblem(rp, (0, 0)), inv_radius)
        Q = ba_rig_ref.linearize(rp, inv_radius)
        assert np.abs(R.S - Q.S).max() <= 1e-17 * np.abs(Q.S).max() and np.abs(R.g - Q.g).max() <= 1e-17 * np.abs(Q.g).max()
        assert np.abs(R.A_S - Q.A_S).max() <= 1e-17 * np.abs(Q.A_S).max() and R.cost == Q.cost
        if inv_radius is not None:
            assert np.abs(R.dc - Q.dc).max() <= 1e-14 * np.abs(Q.dc).max()


def test_gauge_direction_with_one_fixed_body():
    xp = ref.cases()["l_gauge_one_fixed"]
    v = ref.gauge_direction(xp)
    Jv = ref.jacobian_times(xp, v)
    R = ref.reference("l_gauge_one_fixed")
    scale = max(np.abs(R.F).max(), np.abs(R.Fx).max(), np.abs(R.E).max()) * np.abs(v).max()
    rel = float(np.abs(Jv).max() / scale)
    print("gauge: |J v| / (max|J| max|v|) = %.3g (finite-difference level %.3g)" % (rel, ref.jac_tol("l_gauge_one_fixed")))
    assert rel <= 10 * ref.jac_tol("l_gauge_one_fixed")
    # so the undamped S has the null vector: v^T H v ~ 0, and the reduced system is numerically singular
    R0 = ref.reference("l_gauge_one_fixed", 0.0)
    assert not (64 * R0.cond_S * ba_ref.U < 1e-3)
    # the same direction is NOT free with two fixed bodies
    xa = ref.cases()["a_base"]
    assert 64 * ref.reference("a_base", 0.0).cond_S * ba_ref.U < 1e-3 and xa.n_ext == 1


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ref.GAUGE_CASES])
@pytest.mark.parametrize("inv_radius", [0.0, 1e-4])
def test_two_fixed_bodies_are_solvable(name, inv_radius):
    R = ref.reference(name, inv_radius)
    print("%s 1/radius %g: cond(S') = %.3g" % (name, inv_radius, R.cond_S))
    assert R.dc is not None and 64 * R.cond_S * ba_ref.U < 1e-3


_WORST = {}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_fold_against_the_reference(orc, name):
    xp = ref.cases()[name]
    R = ref.reference(name)
    ex = xp.expanded()
    arr = orc.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    S_free, g_free, cost = orc.ba_linearize(arr, use_huber=ex.use_huber, huber=ex.huber)
    A = xp.fold_matrix().astype(np.float64)
    S, g = A.T @ S_free @ A, A.T @ g_free
    kS, kg = ba_ref.ratio(S, R.S, R.A_S), ba_ref.ratio(g, R.g, R.A_g)
    _WORST[name] = (kS, kg)
    print("%s: fold of the oracle vs reference: S %.2f, g %.2f units of 2^-52 A; cost rel %.3g" %
          (name, kS, kg, abs(cost - R.cost) / R.cost))
    assert max(kS, kg) <= ref.ORACLE_FOLD_VS_REF_K
    assert abs(cost - R.cost) <= ba_ref.COST_GPU * R.cost


def test_constants():
    assert ref.ORACLE_FOLD_VS_REF_K <= 8 and ref.K_EXT_GPU == min(8 * ref.ORACLE_FOLD_VS_REF_K, 64)
    if len(_WORST) == len(NAMES):
        print("worst fold figure: %.2f (ORACLE_FOLD_VS_REF_K = %.2f)" % (max(max(v) for v in _WORST.values()), ref.ORACLE_FOLD_VS_REF_K))


def test_lm_step_lowers_the_cost():
    xp = ref.cases()["a_base"]
    bodies, T, points, step, step_l, R = ref.lm_step(xp, 1e-4)
    c1 = xp.with_state(bodies.astype(np.float64), points.astype(np.float64), T.astype(np.float64)).rp.cost()
    assert c1 < R.cost
    assert np.array_equal(bodies[:2].astype(np.float64), xp.rp.poses[:2]) and np.array_equal(T[0].astype(np.float64), xp.rp.T_b_c[0])
    assert not np.array_equal(T[1].astype(np.float64), xp.rp.T_b_c[1])
