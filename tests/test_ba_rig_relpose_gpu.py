"""GPU: relative-pose covariances of BODY pairs in rig form (vsl_ba_rig_relative_pose_covariance) against
tests/ba_rig_cov_ref.py -- ba_relpose_ref's scheme and its derived tolerances (joint: Ref.tol; cov, info, meas: see
ba_relpose_ref.py) on the bodies.  Each test prints its figures (`pytest -s`)."""
import numpy as np
import pytest

import ba_relpose_ref as RP
import ba_rig_cov_ref as ref
import pgo_ref as pg

pytestmark = pytest.mark.gpu


def _arrays(vsl, rp):
    """(BaArrays of the cameras, RigArrays).  arr.poses is not read by the covariance calls: handed in as zeros."""
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr, rp.points, rp.obs_camera,
                       rp.obs_lm, rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(rp.poses, rp.cam_fixed, rp.cam_body, rp.T_b_c)
    return arr, rig


def _raises(vsl, code, call):
    with pytest.raises(vsl.VslError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def _errors(rel, pairs, out, label):
    joint, meas, cov, info = out[:4]
    rel.prepare(pairs)
    worst = dict(joint=0.0, meas=0.0, cov=0.0, info=0.0)
    for k, (a, b) in enumerate(pairs):
        p = rel.pair(a, b)
        for name, got, want, tol in (("joint", joint[k], p.joint, p.tol_joint), ("meas", meas[k], p.meas, p.tol_meas),
                                     ("cov", cov[k], p.cov, p.tol_cov), ("info", info[k], p.info, p.tol_info)):
            e = float(np.abs(got - want).max())
            worst[name] = max(worst[name], e / tol)
            assert e <= tol, (label, name, (a, b), e, tol)
    print("%s, %d pairs: worst error / bound: " % (label, len(pairs)) + ", ".join("%s %.2g" % kv for kv in worst.items()))


@pytest.mark.parametrize("name", ["a_base", "g_huber_outliers", "m_sparse_groups"])
def test_all_pairs_against_the_reference(ctx, vsl, name):
    rp = ref.cases()[name]
    R = ref.reference(name)
    arr, rig = _arrays(vsl, rp)
    pairs = RP.all_pairs(rp.cam_fixed)
    assert any(rp.cam_fixed[a] for a, _ in pairs)                                    # one member of a pair is fixed
    kw = dict(use_huber=rp.use_huber, huber=rp.huber)
    out = ctx.ba_rig_relative_pose_covariance(arr, rig, pairs, **kw)
    assert out[4] == 0 and all(np.isfinite(x).all() for x in out[:4])
    _errors(R.relpose(), pairs, out, name)
    joint, meas, cov, info = out[:4]
    assert np.array_equal(joint, joint.transpose(0, 2, 1))
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(info, info.transpose(0, 2, 1))
    # the diagonal blocks are the marginal call's bits; a fixed member's rows and columns are exactly +0.0
    free = [int(b) for b in np.flatnonzero(rp.cam_fixed == 0)]
    cb = ctx.ba_rig_covariance(arr, rig, free, **kw)[0]
    at = {b: k for k, b in enumerate(free)}
    for k, (a, b) in enumerate(pairs):
        for side, body in ((0, a), (1, b)):
            blk = slice(6 * side, 6 * side + 6)
            if rp.cam_fixed[body]:
                assert not joint[k][blk].any() and not joint[k][:, blk].any() and not np.signbit(joint[k][blk]).any()
            else:
                assert joint[k][blk, blk].tobytes() == cb[at[body]].tobytes(), (a, b)
    # (b, a) is (a, b) swapped and transposed; a subset with duplicates and a second call return the same bits
    sw = ctx.ba_rig_relative_pose_covariance(arr, rig, [(b, a) for a, b in pairs], **kw)
    perm = np.r_[6:12, 0:6]
    assert np.array_equal(sw[0], joint[:, perm][:, :, perm])
    _errors(R.relpose(), [(b, a) for a, b in pairs], sw, name + " reversed")
    pick = [len(pairs) - 1, 0, len(pairs) - 1, 1]
    sub = ctx.ba_rig_relative_pose_covariance(arr, rig, [pairs[k] for k in pick], **kw)
    assert all(x.tobytes() == y[pick].tobytes() for x, y in zip(sub[:4], out[:4]))
    again = ctx.ba_rig_relative_pose_covariance(arr, rig, pairs, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:4], out[:4]))


def test_the_pose_graph_accepts_the_rig_information(ctx, vsl):
    """meas / info of the body pairs are edge_meas / edge_info of a pose graph whose nodes are the bodies."""
    rp = ref.cases()["m_sparse_groups"]
    arr, rig = _arrays(vsl, rp)
    pairs = RP.all_pairs(rp.cam_fixed)
    joint, meas, cov, info, ns = ctx.ba_rig_relative_pose_covariance(arr, rig, pairs, use_huber=rp.use_huber, huber=rp.huber)
    assert ns == 0
    g = pg.Graph(rp.poses, rp.cam_fixed, [a for a, _ in pairs], [b for _, b in pairs], meas)
    before = g.poses.copy()
    s = ctx.pose_graph_optimize(g, edge_info=info)                  # VSL_ERR_INVALID would raise: every Omega is accepted
    move = float(np.abs(g.poses - before).max())
    print("weighted pose graph on its own measurements: initial cost %.3g, poses moved by %.3g" % (s.initial_cost, move))
    assert s.initial_cost < 1e-20 and move <= 1e-12


def test_refusals(ctx, vsl):
    rp = ref.cases()["a_base"]
    arr, rig = _arrays(vsl, rp)
    for pairs in ([(1, 3)], [(-1, 2)], [(1, 2), (2, 2)]):
        _raises(vsl, -1, lambda: ctx.ba_rig_relative_pose_covariance(arr, rig, pairs))
    rp2 = ref.cases()["j_identity_is_free"]                                         # bodies 0 and 1 are fixed
    a2, r2 = _arrays(vsl, rp2)
    _raises(vsl, -1, lambda: ctx.ba_rig_relative_pose_covariance(a2, r2, [(2, 3), (0, 1)]))
    ok = ctx.ba_rig_relative_pose_covariance(a2, r2, [(0, 2), (3, 1)])
    assert ok[4] == 0 and np.isfinite(ok[3]).all()
    rig.body_fixed[:] = 0
    _raises(vsl, -7, lambda: ctx.ba_rig_relative_pose_covariance(arr, rig, [(1, 2)]))
    ri = ref.cases()["i_identity_single"]
    ai, gi = _arrays(vsl, ri)
    _raises(vsl, -7, lambda: ctx.ba_rig_relative_pose_covariance(ai, gi, [(1, 2)]))
    empty = ctx.ba_rig_relative_pose_covariance(*_arrays(vsl, rp), np.zeros((0, 2), np.int32))
    assert empty[0].shape == (0, 12, 12) and empty[4] == 0
