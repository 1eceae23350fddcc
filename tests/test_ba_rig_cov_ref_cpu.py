"""CPU: the reference of the rig covariances (tests/ba_rig_cov_ref.py) against itself.

  block formula   the Schur-form landmark block of the contract against the block of the full inverse, both in long
                  double: 64 cond(H) eps_LD max|Sigma| (the rule of the covariance tests at the long double's epsilon)
  camera block    the adjoint sandwich against a finite-difference re-parameterisation: G = d log(T_w_c^-1 T_w_b exp(d)
                  T_b_c) / d d at 0 by central differences (h, h / 2, Richardson) in long double.  The map is smooth with
                  derivatives of order 1, so the extrapolated difference is off by ~h^4 = 1e-16 and by rounding
                  eps_LD / h = 1e-15: G is good to 1e-13 relative with a factor 100 in hand, and a sandwich of two G
                  (36 products per entry) to 72e-13 max|G|^2 max|Sigma_bb|
  case j          identity extrinsics, one camera per body: the rig problem is the free problem of expanded() -- its
                  Sigma against the inverse of ba_ref.linearize(expanded()).H within Ref.tol (the camera poses of
                  expanded() are rounded to double, a relative perturbation of 2^-53 of H's entries)
Each test prints its figures (`pytest -s`)."""
import numpy as np
import pytest

import ba_ref
import ba_rig_cov_ref as ref
from pgo_ref import LD, _ld, se3_exp, se3_inv, se3_log, se3_mul

NAMES = sorted(n for n in ref.cases() if n[0] in "abcdefgkm")
EPS_LD = float(np.finfo(LD).eps)


def test_case_table():
    c = ref.cases()
    assert sorted(n[0] for n in c) == list("abcdefghijkm")
    for name in NAMES + ["j_identity_is_free"]:
        R = ref.reference(name)
        print("%s: cond(H) %.3g, max|Sigma| %.3g, tol %.3g, degenerate %s" % (name, R.cond, np.abs(R.Sigma).max(), R.tol, R.degenerate))
        assert not R.singular and R.cond < 1e7
    assert ref.reference("k_one_observation").degenerate == [5]
    assert all(ref.reference(n).degenerate == [] for n in NAMES if n[0] != "k")


def test_case_i_is_singular_to_working_precision():
    """One camera per body, one fixed body: the scale is free.  The long-double factorisation either fails or leaves a
    condition number beyond anything the float64 rule could bound."""
    R = ref.reference("i_identity_single")
    print("case i: singular %s, cond(H) %.3g" % (R.singular, R.cond))
    assert R.singular or 64 * R.cond * ref.EPS > 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_block_formula_against_the_full_inverse(name):
    R = ref.reference(name)
    bound = 64 * R.cond * EPS_LD * float(np.abs(R.Sigma).max())
    worst = 0.0
    for l in R.lm_pos:
        worst = max(worst, float(np.abs(R.schur_point_block(l) - R.point_block(l, ld=True)).max()))
    print("%s: block formula vs full inverse %.3g (bound %.3g)" % (name, worst, bound))
    assert worst <= bound


def _fd_map(rp, cam, h):
    """d log(T_w_c^-1 T_w_b exp(d) T_b_c) / d d at 0, central differences at step h, [6, 6] long double."""
    Twb = _ld(rp.poses[rp.cam_body[cam]])
    Tbc = _ld(rp.T_b_c[rp.cam_intr[cam]])
    Tcw = se3_inv(se3_mul(Twb, Tbc))
    cols = []
    for k in range(6):
        out = []
        for sign in (1, -1):
            d = np.zeros(6, LD)
            d[k] = sign * LD(h)
            out.append(se3_log(se3_mul(Tcw, se3_mul(se3_mul(Twb, se3_exp(d)), Tbc))))
        cols.append((out[0] - out[1]) / (2 * LD(h)))
    return np.stack(cols, axis=-1)


@pytest.mark.parametrize("name", ["a_base", "e_single_camera_body", "m_sparse_groups"])
def test_camera_block_against_a_reparameterisation(name):
    R = ref.reference(name)
    rp = R.rp
    for cam in np.flatnonzero(rp.cam_fixed[rp.cam_body] == 0):
        G = (4 * _fd_map(rp, cam, 5e-5) - _fd_map(rp, cam, 1e-4)) / 3
        Sbb = R.body_block(rp.cam_body[cam], ld=True)
        M = G @ Sbb @ G.T
        err = float(np.abs((M + M.T) / 2 - R.cam_block(cam, ld=True)).max())
        bound = 72e-13 * float(np.abs(G).max()) ** 2 * float(np.abs(Sbb).max())
        eG = float(np.abs(G - R.cam_adjoint(cam)).max())
        print("%s camera %d: |G - Ad| %.3g, sandwich %.3g (bound %.3g)" % (name, cam, eG, err, bound))
        assert eG <= 1e-13 * float(np.abs(G).max())
        assert err <= bound


def test_identity_rig_is_the_free_problem():
    R = ref.reference("j_identity_is_free")
    ex = R.rp.expanded()
    Sf = ref.cholesky_inverse(ba_ref.linearize(ex).H)
    err = float(np.abs(Sf - R.Sigma_ld).max())
    print("case j: rig Sigma vs free Sigma %.3g (tol %.3g, cond %.3g)" % (err, R.tol, R.cond))
    assert Sf.shape == R.Sigma_ld.shape and err <= R.tol
    for cam in range(len(R.rp.cam_body)):
        if not R.rp.cam_fixed[R.rp.cam_body[cam]]:
            assert np.array_equal(R.cam_block(cam, ld=True), R.body_block(R.rp.cam_body[cam], ld=True))


def test_relative_pose_reference_runs_on_bodies():
    R = ref.reference("a_base")
    rel = R.relpose()
    p = rel.pair(1, 2)
    q = rel.pair(0, 1)                                   # body 0 is fixed: its rows and columns are zero
    assert np.array_equal(p.joint[:6, :6], R.body_block(1)) and np.array_equal(p.joint[6:, 6:], R.body_block(2))
    assert not q.joint[:6].any() and not q.joint[:, :6].any() and np.array_equal(q.joint[6:, 6:], R.body_block(1))
    assert np.allclose(p.info @ p.cov, np.eye(6), atol=1e-6)
