"""CPU: pins tests/ba_rig_ref.py (the long-double reference of the rig-constrained bundle adjustment) on every case the
GPU tests of test_ba_rig_gpu.py use, with no new library code:
  * the fold identity S_rig = A^T S_free A, g_rig = A^T g_free -- S_free, g_free from the CPU ORACLE's ba_linearize of
    the expanded problem, folded in float64 numpy -- against the reference, entrywise in units of 2^-52 A.  The worst
    figure is printed (`pytest -s`) and must not exceed ba_rig_ref.ORACLE_FOLD_VS_REF_K, which the device tolerance is
    8 x of (at most 64);
  * the definition: the reference's finite-difference F_b equals F_c Ad(T_b_c^-1), F_c from ba_ref, to the case's
    jac_tol."""
import numpy as np
import pytest

import ba_ref
import ba_rig_ref as ref

LD = np.longdouble
NAMES = ("a_base", "b_all_see_all", "c_fixed_body_only", "d_one_body_left_right", "e_single_camera_body", "f_models",
         "g_huber_outliers", "h_23_free", "i_identity_single")


def test_case_table_holds_its_premises():
    C = ref.cases()
    assert tuple(C) == NAMES
    a = C["a_base"]
    assert len(a.poses) == 3 and len(a.cam_body) == 6 and a.cam_fixed.tolist() == [1, 0, 0] and len(a.points) == 9
    e1 = a.T_b_c[1]
    assert abs(np.linalg.norm(e1[4:]) - 0.11) < 1e-3 and abs(np.degrees(2 * np.arccos(e1[3])) - 2.0) < 1e-9
    b = C["b_all_see_all"]
    assert len(b.obs_lm) == 6 * 9
    c = C["c_fixed_body_only"]
    assert set(c.cam_body[c.obs_camera[c.obs_lm == 3]]) == {0}
    d = C["d_one_body_left_right"]
    assert sorted(d.obs_camera[d.obs_lm == 4].tolist()) == [2, 3] and set(d.cam_body[[2, 3]]) == {1}
    e = C["e_single_camera_body"]
    assert np.bincount(e.cam_body).tolist() == [2, 2, 1]
    assert C["f_models"].cam_model == (0, 3)
    g = C["g_huber_outliers"]
    assert g.use_huber and ref.reference("g_huber_outliers").outlier[list(g.outliers)].all()
    h = C["h_23_free"]
    assert h.n_free == 23 and 6 * h.n_free > 128 and int((h.obs_lm == 0).sum()) == 30
    assert len(set(h.obs_camera[h.obs_lm == 0].tolist())) == 30
    i = C["i_identity_single"]
    assert np.array_equal(i.T_b_c, [ba_ref.IDENT, ba_ref.IDENT]) and np.bincount(i.cam_body).max() == 1
    for rp in C.values():
        assert np.bincount(rp.obs_lm, minlength=len(rp.points)).min() >= 2      # no single-observation landmark


@pytest.mark.parametrize("name", NAMES)
def test_finite_difference_body_jacobian_is_the_adjoint_fold(name):
    rp = ref.cases()[name]
    R = ref.reference(name)
    rp.blocks()                                      # leaves ba_ref's F_c of the same point
    err = ba_ref.block_error(R.F, rp.adjoint_jacobian())
    print("%s: max |F_b(fd) - F_c Ad| / max|F_b| = %.3g (tolerance %.3g)" % (name, err.max(), ref.jac_tol(name)))
    assert err.max() <= ref.jac_tol(name)


_WORST = {}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_fold_against_the_reference(orc, name):
    rp = ref.cases()[name]
    R = ref.reference(name)
    ex = rp.expanded()
    arr = orc.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    S_free, g_free, cost = orc.ba_linearize(arr, use_huber=ex.use_huber, huber=ex.huber)
    A = rp.fold_matrix().astype(np.float64)
    S, g = A.T @ S_free @ A, A.T @ g_free
    kS, kg = ba_ref.ratio(S, R.S, R.A_S), ba_ref.ratio(g, R.g, R.A_g)
    _WORST[name] = (kS, kg)
    print("%s: fold of the oracle vs reference: S %.2f, g %.2f units of 2^-52 A; cost rel %.3g" %
          (name, kS, kg, abs(cost - R.cost) / R.cost))
    assert max(kS, kg) <= ref.ORACLE_FOLD_VS_REF_K
    assert abs(cost - R.cost) <= ba_ref.COST_GPU * R.cost


def test_constants():
    assert ref.ORACLE_FOLD_VS_REF_K <= 8 and ref.K_RIG_GPU == min(8 * ref.ORACLE_FOLD_VS_REF_K, 64)
    if len(_WORST) == len(NAMES):
        print("worst fold figure: %.2f (ORACLE_FOLD_VS_REF_K = %.2f)" % (max(max(v) for v in _WORST.values()), ref.ORACLE_FOLD_VS_REF_K))


def test_scaled_reference_reduces_to_the_plain_one_without_damping():
    R0, Rs = ref.reference("a_base"), ref.reference("a_base", 0.0)
    nc = 6 * ref.cases()["a_base"].n_free
    Dc = Rs.D[:nc]
    assert np.abs(Rs.S - Dc[:, None] * R0.S * Dc[None, :]).max() <= 1e-17 * np.abs(Rs.S).max()
    assert np.abs(Rs.g - Dc * R0.g).max() <= 1e-17 * np.abs(Rs.g).max()


def test_lm_step_lowers_the_cost():
    rp = ref.cases()["a_base"]
    bodies, points, step_b, step_l, c0, c1, R = ref.lm_step(rp, 1e-4)
    assert c1 < c0 and np.array_equal(bodies[0].astype(np.float64), rp.poses[0])
