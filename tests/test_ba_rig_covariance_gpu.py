"""GPU: marginal covariances in rig form (vsl_ba_rig_covariance; ba_rig.hip "COVARIANCES") against the long-double
reference tests/ba_rig_cov_ref.py.

Tolerance, every comparison with the reference: 64 * cond(H) * 2^-52 * max|Sigma| (Ref.tol, the rule of DESIGN.md 16);
for case k cond and the maximum are those of the system without landmark 5; twice that where two device results are
compared with each other.  Each test prints its figures (`pytest -s`)."""
import hashlib

import numpy as np
import pytest

import ba_rig_cov_ref as ref
import ba_rig_ref as rr

pytestmark = pytest.mark.gpu


def _arrays(vsl, rp):
    """(BaArrays of the cameras, RigArrays).  arr.poses is not read by the covariance calls: handed in as zeros."""
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr, rp.points, rp.obs_camera,
                       rp.obs_lm, rp.obs_uv, rp.cam_model)
    rig = vsl.RigArrays(rp.poses, rp.cam_fixed, rp.cam_body, rp.T_b_c)
    return arr, rig


def _full_query(rp):
    bodies = np.flatnonzero(rp.cam_fixed == 0)
    cams = np.flatnonzero(rp.cam_fixed[rp.cam_body] == 0)
    return bodies, cams, np.arange(len(rp.points))


def _full(ctx, vsl, name):
    rp = ref.cases()[name]
    arr, rig = _arrays(vsl, rp)
    bodies, cams, lms = _full_query(rp)
    out = ctx.ba_rig_covariance(arr, rig, bodies, cams, lms, use_huber=rp.use_huber, huber=rp.huber)
    assert np.array_equal(rig.body_poses, rp.poses) and np.array_equal(arr.points, rp.points)      # nothing is optimised
    return rp, (bodies, cams, lms), out


def _check(name, R, query, out, skip_lms=()):
    bodies, cams, lms = query
    cb, cc, cl, nd = out
    eb = max(float(np.abs(cb[k] - R.body_block(b)).max()) for k, b in enumerate(bodies))
    ec = max(float(np.abs(cc[k] - R.cam_block(c)).max()) for k, c in enumerate(cams))
    el = max(float(np.abs(cl[k] - R.point_block(l)).max()) for k, l in enumerate(lms) if l not in skip_lms)
    print("%s: body %.3g, camera %.3g, landmark %.3g (tol %.3g, cond %.3g)" % (name, eb, ec, el, R.tol, R.cond))
    assert eb <= R.tol and ec <= R.tol and el <= R.tol, (name, eb, ec, el, R.tol)
    for x in (cb, cc, cl):
        assert np.array_equal(x, x.transpose(0, 2, 1), equal_nan=True)                             # exactly symmetric


@pytest.mark.parametrize("name", sorted(n for n in ref.cases() if n[0] in "abcdefgm"))
def test_full_query_against_the_reference(ctx, vsl, name):
    rp, query, out = _full(ctx, vsl, name)
    assert out[3] == 0
    _check(name, ref.reference(name), query, out)


def test_identity_rig_against_the_free_covariance(ctx, vsl):
    """Case j: identity extrinsics, one camera per body.  Against Context.ba_covariance of the expanded problem (two
    device results: twice the tolerance); the camera blocks ARE the body blocks."""
    rp, (bodies, cams, lms), (cb, cc, cl, nd) = _full(ctx, vsl, "j_identity_is_free")
    R = ref.reference("j_identity_is_free")
    ex = rp.expanded()
    exa = vsl.BaArrays(ex.poses, ex.cam_fixed, ex.cam_intr, ex.intr, ex.points, ex.obs_cam, ex.obs_lm, ex.obs_uv, ex.cam_model)
    fp, fl, fnd = ctx.ba_covariance(exa, cams, lms, use_huber=ex.use_huber, huber=ex.huber)
    ep, el = float(np.abs(cc - fp).max()), float(np.abs(cl - fl).max())
    print("case j: rig vs free: pose %.3g, landmark %.3g (bound %.3g)" % (ep, el, 2 * R.tol))
    assert nd == 0 and fnd == 0 and ep <= 2 * R.tol and el <= 2 * R.tol
    assert list(rp.cam_body[cams]) == list(bodies)
    assert np.array_equal(cc, cb)                                    # the contract: compared with ==
    _check("j", R, (bodies, cams, lms), (cb, cc, cl, nd))


def test_one_body_left_right_and_fixed_body_only(ctx, vsl):
    """Case d, landmark 4: seen by the left and right cameras of free body 1 only -- one group of two observations, one
    W.  Case c, landmark 3: seen by the fixed body only -- P^-1 alone."""
    for name, lm in (("d_one_body_left_right", 4), ("c_fixed_body_only", 3)):
        rp = ref.cases()[name]
        R = ref.reference(name)
        arr, rig = _arrays(vsl, rp)
        _, _, cl, nd = ctx.ba_rig_covariance(arr, rig, [], [], [lm], use_huber=rp.use_huber, huber=rp.huber)
        e = float(np.abs(cl[0] - R.point_block(lm)).max())
        print("%s landmark %d: %.3g (tol %.3g)" % (name, lm, e, R.tol))
        assert nd == 0 and e <= R.tol
    k = R.nc + 3 * R.lm_pos[3]
    own = np.linalg.inv(R.H[k:k + 3, k:k + 3].astype(np.float64))
    assert float(np.abs(cl[0] - own).max()) <= R.tol                                                # case c: P^-1 alone


def test_degenerate_landmark(ctx, vsl):
    rp, query, out = _full(ctx, vsl, "k_one_observation")
    R = ref.reference("k_one_observation")
    assert out[3] == 1 and np.isnan(out[2][5]).all() and np.isfinite(np.delete(out[2], 5, axis=0)).all()
    _check("k", R, query, out, skip_lms=(5,))
    arr, rig = _arrays(vsl, rp)
    _, _, cl, nd = ctx.ba_rig_covariance(arr, rig, [], [], [5, 2, 5], use_huber=rp.use_huber, huber=rp.huber)
    assert nd == 2 and np.isnan(cl[[0, 2]]).all() and cl[1].tobytes() == out[2][2].tobytes()


def _solve_digest(ctx, vsl, rp):
    arr, rig = _arrays(vsl, rp)
    s = ctx.bundle_adjust_rig(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    h = hashlib.sha256()
    for a in (rig.body_poses, arr.points, arr.poses, np.array([s.final_cost])):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _raises(vsl, code, call):
    with pytest.raises(vsl.VslError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_errors_and_arena_hygiene(ctx, vsl):
    rp = ref.cases()["a_base"]
    before = _solve_digest(ctx, vsl, rp)
    arr, rig = _arrays(vsl, rp)
    good = ctx.ba_rig_covariance(arr, rig, [1, 2], [2], [0])
    assert _solve_digest(ctx, vsl, rp) == before
    # VSL_ERR_NUMERIC: the free scale of one camera per body with one fixed body (after device work); no fixed body (before)
    ri = ref.cases()["i_identity_single"]
    ai, gi = _arrays(vsl, ri)
    _raises(vsl, -7, lambda: ctx.ba_rig_covariance(ai, gi))
    assert _solve_digest(ctx, vsl, rp) == before
    again = ctx.ba_rig_covariance(arr, rig, [1, 2], [2], [0])
    assert all(np.array_equal(x, y) for x, y in zip(good[:3], again[:3]))
    arr, rig = _arrays(vsl, rp)
    rig.body_fixed[:] = 0
    _raises(vsl, -7, lambda: ctx.ba_rig_covariance(arr, rig))
    # VSL_ERR_INVALID: the query rules
    arr, rig = _arrays(vsl, rp)
    for kw in (dict(bodies=[0]), dict(bodies=[3]), dict(bodies=[-1]), dict(bodies=[1], cams=[0]), dict(bodies=[1], cams=[1]),
               dict(bodies=[1], cams=[6]), dict(bodies=[1], cams=[-1]), dict(bodies=[1], lms=[9]), dict(bodies=[1], lms=[-1])):
        _raises(vsl, -1, lambda: ctx.ba_rig_covariance(arr, rig, **kw))
    # ... and what vsl_ba_rig_linearize rejects
    arr, rig = _arrays(vsl, rp)
    rig.cam_body[3] = 3
    _raises(vsl, -1, lambda: ctx.ba_rig_covariance(arr, rig))
    arr, rig = _arrays(vsl, rp)
    arr.cam_intr[3] = 0
    _raises(vsl, -1, lambda: ctx.ba_rig_covariance(arr, rig))
    # a negative count and a null output, at the C ABI
    C = vsl.C
    arr, rig = _arrays(vsl, rp)
    st, rg = ctx._ba_rig_structs(arr, rig)
    o = ctx._ba_opts(True, 1.0, 0, 0)
    one = np.array([1], np.int32)
    p = one.ctypes.data_as(C.POINTER(C.c_int32))
    assert ctx.L.vsl_ba_rig_covariance(ctx.h, C.byref(st), C.byref(rg), C.byref(o), p, -1, None, None, 0, None, None, 0, None, None) == -1
    assert ctx.L.vsl_ba_rig_covariance(ctx.h, C.byref(st), C.byref(rg), C.byref(o), p, 1, None, None, 0, None, None, 0, None, None) == -1
    assert ctx.L.vsl_ba_rig_covariance(ctx.h, C.byref(st), None, C.byref(o), p, 1, None, None, 0, None, None, 0, None, None) == -1
    # all counts zero: validates, launches nothing
    assert ctx.L.vsl_ba_rig_covariance(ctx.h, C.byref(st), C.byref(rg), C.byref(o), None, 0, None, None, 0, None, None, 0, None, None) == 0
    empty = ctx.ba_rig_covariance(arr, rig, [], [], [])
    assert empty[0].shape == (0, 6, 6) and empty[3] == 0
    assert _solve_digest(ctx, vsl, rp) == before


def test_group_cap(ctx, vsl):
    """A landmark seen by 257 free bodies has 257 groups: VSL_ERR_INVALID when it is queried, alone or after another."""
    rp = rr.rig_scene(258, 1, 2, 512, cams_of_body=[(0,)] * 258)
    rp = rr._drop(rp, ~((rp.obs_lm == 1) & (rp.obs_camera > 20)))
    arr, rig = _arrays(vsl, rp)
    _raises(vsl, -1, lambda: ctx.ba_rig_covariance(arr, rig, [], [], [0]))
    _raises(vsl, -1, lambda: ctx.ba_rig_covariance(arr, rig, [], [], [1, 0]))


def test_factor_route_past_the_small_solver(ctx, vsl):
    """Case h, 138 unknowns: bodies, cameras and landmark 0 (15 groups).  Pose blocks against numpy.linalg.inv of the
    device's own S (ba_rig_linearize), and everything against the reference."""
    rp = ref.cases()["h_23_free"]
    R = ref.reference("h_23_free")
    arr, rig = _arrays(vsl, rp)
    bodies, cams, _ = _full_query(rp)
    out = ctx.ba_rig_covariance(arr, rig, bodies, cams, [0], use_huber=rp.use_huber, huber=rp.huber)
    S, _, _ = ctx.ba_rig_linearize(arr, rig, use_huber=rp.use_huber, huber=rp.huber)
    Si = np.linalg.inv(S)
    es = max(float(np.abs(out[0][k] - Si[6 * k:6 * k + 6, 6 * k:6 * k + 6]).max()) for k in range(len(bodies)))
    print("case h: body blocks vs inv(device S) %.3g (tol %.3g)" % (es, R.tol))
    assert es <= R.tol and out[3] == 0
    assert (rp.obs_lm == 0).sum() == 30
    _check("h", R, (bodies, cams, [0]), out)


@pytest.mark.parametrize("name", ["a_base", "m_sparse_groups"])
def test_bit_properties(ctx, vsl, name):
    rp, (bodies, cams, lms), full = _full(ctx, vsl, name)
    arr, rig = _arrays(vsl, rp)
    kw = dict(use_huber=rp.use_huber, huber=rp.huber)
    for x in full[:3]:
        assert np.array_equal(x, x.transpose(0, 2, 1))
    again = ctx.ba_rig_covariance(arr, rig, bodies, cams, lms, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(full[:3], again[:3]))
    # a subset, permuted, with duplicates
    pb, pc, pl = [len(bodies) - 1, 0, len(bodies) - 1], [len(cams) - 1, 1, 1], [len(lms) - 2, 0, len(lms) - 2, 3]
    sub = ctx.ba_rig_covariance(arr, rig, bodies[pb], cams[pc], lms[pl], **kw)
    assert sub[0].tobytes() == full[0][pb].tobytes() and sub[1].tobytes() == full[1][pc].tobytes()
    assert sub[2].tobytes() == full[2][pl].tobytes()
    assert sub[0][0].tobytes() == sub[0][2].tobytes() and sub[2][0].tobytes() == sub[2][2].tobytes()
    # one block alone
    b1 = ctx.ba_rig_covariance(arr, rig, bodies[:1], [], [], **kw)
    l1 = ctx.ba_rig_covariance(arr, rig, [], [], lms[-1:], **kw)
    c1 = ctx.ba_rig_covariance(arr, rig, [], cams[-1:], [], **kw)
    assert b1[0][0].tobytes() == full[0][0].tobytes() and l1[2][0].tobytes() == full[2][-1].tobytes()
    assert c1[1][0].tobytes() == full[1][-1].tobytes()
    # the default query: all free bodies
    d = ctx.ba_rig_covariance(arr, rig, **kw)
    assert d[0].tobytes() == full[0].tobytes() and d[1].shape == (0, 6, 6) and d[2].shape == (0, 3, 3)
