"""CPU: the long-double reference of the covariances with free stereo extrinsics (tests/ba_rig_ext_cov_ref.py) against
itself -- the Schur form of the contract equals the blocks of the dense H^-1, the camera block equals the posterior pushed
through the fold matrix A of DESIGN.md 31, and the pivot rule separates the gauge case from the regular ones."""
import numpy as np
import pytest

import ba_rig_ext_cov_ref as ref
import ba_rig_ext_ref as xr

REGULAR = ("a_base", "b_both_free", "c_block0_free", "f_single_camera_body", "i_no_free_body", "j_22_free")
SMALL = sorted(n for n in xr.cases() if n[0] in "abcdefghi")


@pytest.mark.parametrize("name", SMALL + ["j_22_free"])
def test_schur_form_equals_the_blocks_of_the_dense_inverse(name):
    R = ref.reference(name)
    assert not R.singular and R.dense
    Sinv = R.schur_pose_inverse()
    scale = float(np.abs(R.Sigma_ld).max())
    bound = 64.0 * R.cond * float(np.finfo(np.longdouble).eps) * scale      # the tolerance rule at long-double precision
    e_pose = float(np.abs(Sinv - R.Sigma_ld[:R.nt, :R.nt]).max())
    e_lm = max(float(np.abs(R.schur_point_block(l, Sinv) - R.point_block(l, ld=True)).max()) for l in R.lm_pos)
    print("%s: Schur form vs dense inverse: pose part %.3g, landmarks %.3g (bound %.3g)" % (name, e_pose, e_lm, bound))
    assert e_pose <= bound and e_lm <= bound
    assert R.tol > 1e4 * max(e_pose, e_lm)                                  # far below what the device is allowed


@pytest.mark.parametrize("name", SMALL)
def test_camera_block_is_the_posterior_pushed_through_the_fold(name):
    """xi = A x maps [free bodies | free blocks] to the tangents of the free cameras of the expanded problem P
    (ExtProblem.fold_matrix, built independently of ExtCovRef.cam_matrix): the camera block is the (c, c) block of
    A Sigma A^T."""
    xp, R = xr.cases()[name], ref.reference(name)
    A = xp.fold_matrix()
    M = A @ R.Sigma_ld[:R.nt, :R.nt] @ A.T
    cams = np.flatnonzero(xp.cam_free_mask())
    e = max(float(np.abs(M[6 * k:6 * k + 6, 6 * k:6 * k + 6] - R.cam_block(c, ld=True)).max()) for k, c in enumerate(cams))
    assert e <= 1e-15 * float(np.abs(M).max())
    held = np.flatnonzero(~xp.cam_free_mask())
    for c in held:
        with pytest.raises(ValueError):
            R.cam_matrix(c)


def test_pivot_rule_separates_the_gauge_case():
    """The smallest pivot ratio L_ii^2 / S_ii of the regular cases is 3.69e-5 (case b; quoted as 3.7e-5), six orders above
    2^-36 = 1.5e-11.  Case l: cond(S) 1.7e18 and a pivot ratio of 3e-15 in long double.  In FLOAT64 that pivot is rounding
    noise (7e-11 here, above the threshold): the unknowns along the gauge direction are mostly those eliminated first.
    The same ratio for the unknown eliminated LAST, 1 / (S_uu [S^-1]_uu), minimised over u, is 1.4e-5 or more in every
    regular case and 4e-16 in case l in float64: the form the device tests as well."""
    for name in REGULAR:
        S = ref.reference(name).reduced()
        p = ref.pivot_ratio(S)
        q = float((1.0 / (np.diag(S) * np.diag(np.linalg.inv(S.astype(np.float64))))).min())
        print("%s: pivot ratio %.3g, order-independent %.3g" % (name, p, q))
        assert p >= 3.69e-5 and q >= 1.4e-5
    S = ref.reference("l_gauge_one_fixed").reduced()
    cond = float(np.linalg.cond(S.astype(np.float64)))
    p_ld = ref.pivot_ratio(S, np.longdouble)
    q = float((1.0 / (np.diag(S) * np.diag(np.linalg.inv(S.astype(np.float64))))).astype(np.float64).min())
    print("l: cond %.3g, long-double pivot ratio %.3g, float64 %s, order-independent %.3g" % (cond, p_ld, ref.pivot_ratio(S), q))
    assert cond >= 1e17 and p_ld <= 1e-3 * ref.PIVOT_TOL and q <= 1e-3 * ref.PIVOT_TOL
