"""CPU: pins tests/ba_relpose_ref.py, the reference of vsl_ba_relative_pose_covariance, on the shapes the GPU tests use
(tests/test_ba_relative_pose_covariance_gpu.py): Sigma_r,ref is symmetric positive definite for every pair, and the
Jacobians it takes from pgo_ref agree with the brute-force route (perturb both poses, difference the residual, at steps
pgo_ref does not use) to pgo_ref.GPU_TOL -- the level tests/test_pgo_ref_cpu.py establishes for pgo_ref's own
Jacobians."""
import numpy as np
import pytest

import ba_cov_band_ref as B
import ba_cov_ref as R
import ba_relpose_ref as RP
import pgo_ref as pg


def _check(rr, pairs, label):
    worst_j, min_eig, worst_cond = 0.0, np.inf, 0.0
    P = pg._ld(rr.case.g.poses)
    rr.prepare(pairs)
    pa, pb = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    # the Jacobians against the brute-force route, all pairs in one batched evaluation
    _, J = rr.jacobians(pairs)
    brute = RP.brute_force_jacobian(P[pa], P[pb])
    for k, (a, b) in enumerate(pairs):
        p = rr.pair(a, b)
        assert np.array_equal(p.cov, p.cov.T) and np.abs(p.joint - p.joint.T).max() <= p.tol_joint
        lam = np.linalg.eigvalsh(p.cov)
        assert lam[0] > 0, (a, b)
        min_eig, worst_cond = min(min_eig, lam[0]), max(worst_cond, lam[-1] / lam[0])
        assert np.isfinite(p.info).all() and np.all(np.linalg.eigvalsh(p.info) > 0)
        for side, cam in ((0, a), (1, b)):
            blk = slice(6 * side, 6 * side + 6)
            if rr.fixed[cam]:
                assert not J[k][:, blk].any() and not p.joint[blk].any() and not p.joint[:, blk].any()
            else:
                worst_j = max(worst_j, float(np.abs(J[k][:, blk] - brute[k][:, blk]).max() / np.abs(brute[k]).max()))
    print("%s: %d pairs, J vs brute force %.3g (bound %.3g), min eig(Sigma_r) %.3g, max cond(Sigma_r) %.3g"
          % (label, len(pairs), worst_j, pg.GPU_TOL, min_eig, worst_cond))
    assert worst_j <= pg.GPU_TOL


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("huber", [True, False])
def test_small_window(orc, synth, model, huber):
    d = R.problem(synth, 5, n_free=6, n_lms=60, model=model)
    rr = RP.RelRef(R.Ref(orc, R.arrays(orc, d), use_huber=huber), d["poses"], d["cam_fixed"])
    _check(rr, RP.all_pairs(d["cam_fixed"]), "6 free, model %d, huber %d" % (model, huber))


def test_window_of_twenty(orc, synth):
    d = R.problem(synth, 6, n_free=20, n_lms=60)
    rr = RP.RelRef(R.Ref(orc, R.arrays(orc, d)), d["poses"], d["cam_fixed"])
    _check(rr, RP.all_pairs(d["cam_fixed"]), "20 free")


def test_open_chain(orc, synth):
    d = B.open_chain(synth)
    rr = RP.RelRef(B.chain_ref(orc, synth), d["poses"], d["cam_fixed"])
    pairs = [(a, a + 2) for a in range(0, 58, 2)] + [(2, 59), (10, 40), (0, 7), (33, 1), (59, 2)]
    _check(rr, pairs, "open chain")


def test_a_measurement_offset_does_not_move_the_jacobians(orc, synth):
    d = R.problem(synth, 5, n_free=6, n_lms=60)
    P = pg._ld(d["poses"])
    _, Ja0, Jb0, _ = pg.residual_jacobian(P[3], P[6], np.zeros(6))
    _, Ja1, Jb1, _ = pg.residual_jacobian(P[3], P[6], np.array([0.3, -0.2, 0.1, 0.05, -0.04, 0.02]))
    assert np.array_equal(Ja0, Ja1) and np.array_equal(Jb0, Jb1)
