"""CPU: tests/ba_cov_ref.py, the numpy reference that tests/test_ba_covariance_gpu.py compares vsl_ba_covariance with, pinned
to the oracle.  Tolerance (every comparison): 64 * cond(H) * 2^-52 * max|quantity compared|, cond(H) from the helper's own
dense H -- the helper is built from the oracle's Jacobians alone and never reads a device output."""
import numpy as np
import pytest

import ba_cov_ref as R


@pytest.fixture(scope="module")
def case(orc, synth):
    d = R.problem(synth, 5, n_free=3, n_lms=40)
    # landmark 0 keeps its observations in fixed cameras only (it has some: every camera looks at the same cloud)
    free = d["cam_fixed"][d["obs_cam"]] == 0
    d = R.drop_observations(d, (d["obs_lm"] == 0) & free)
    assert (d["obs_lm"] == 0).sum() >= 2
    arr = R.arrays(orc, d)
    return arr, {h: R.Ref(orc, arr, use_huber=h) for h in (True, False)}


@pytest.mark.parametrize("huber", [True, False])
def test_schur_of_reference_H_is_the_oracles_S(orc, case, huber):
    arr, refs = case
    ref = refs[huber]
    S, _, _ = orc.ba_linearize(arr, use_huber=huber)
    assert ref.nc == 18 and S.shape == (18, 18)
    assert np.abs(ref.schur() - S).max() <= 64 * ref.cond * R.EPS * np.abs(S).max()


@pytest.mark.parametrize("huber", [True, False])
def test_pose_blocks_are_blocks_of_inverse_S(orc, case, huber):
    arr, refs = case
    ref = refs[huber]
    S, _, _ = orc.ba_linearize(arr, use_huber=huber)
    Si = np.linalg.inv(S)
    for k, c in enumerate(ref.free):
        assert np.abs(ref.pose_block(c) - Si[6 * k:6 * k + 6, 6 * k:6 * k + 6]).max() <= ref.tol


def test_landmark_seen_by_fixed_cameras_only_is_its_own_inverse(case):
    _, refs = case
    ref = refs[True]
    assert np.abs(ref.point_block(0) - ref.landmark_own_inverse(0)).max() <= ref.tol
    # and one that free cameras see is NOT (the camera uncertainty adds to it)
    assert np.abs(ref.point_block(1) - ref.landmark_own_inverse(1)).max() > ref.tol


def test_corrector_is_active_and_degenerate_landmarks_are_left_out(orc, synth):
    d = R.problem(synth, 5, n_free=3, n_lms=40, outlier_frac=0.2)
    arr = R.arrays(orc, d)
    a, b = R.Ref(orc, arr, use_huber=True), R.Ref(orc, arr, use_huber=False)
    assert np.abs(a.H - b.H).max() > 1e-3 * np.abs(b.H).max()
    keep = np.ones(len(d["obs_lm"]), bool)
    keep[np.flatnonzero(d["obs_lm"] == 3)[1:]] = False
    c = R.Ref(orc, R.arrays(orc, R.drop_observations(d, ~keep)))
    assert c.degenerate == [3] and 3 not in c.lm_pos and c.H.shape[0] == a.H.shape[0] - 3
