"""GPU: covariances of the rig posterior with free stereo extrinsics (vsl_ba_rig_ext_covariance; ba_rig.hip "EXTRINSICS:
COVARIANCES") against the long-double reference tests/ba_rig_ext_cov_ref.py on the cases of
tests/ba_rig_ext_ref.py.

Tolerance, every comparison with the reference: 64 * cond(H) * 2^-52 * max|Sigma| (ExtCovRef.tol, the rule of DESIGN.md
16 and 28).  Each test prints its figures (`pytest -s`)."""
import hashlib

import numpy as np
import pytest

import ba_rig_ext_cov_ref as ref
import ba_rig_ext_ref as xr
import ba_rig_ref as rr

pytestmark = pytest.mark.gpu

KEYS = ("cov_body", "cov_ext", "cov_body_ext", "cov_cam", "cov_point")


def _arrays(vsl, xp, nan_rig=True):
    """(BaArrays of the cameras, RigArrays, the extrinsics [2, 7]).  arr.poses is not read.  nan_rig: rig.T_b_c is NaN --
    the call must not read it."""
    rp = xp.rp
    arr = vsl.BaArrays(np.zeros((len(rp.cam_body), 7)), rp.cam_fixed[rp.cam_body], rp.cam_intr, rp.intr, rp.points, rp.obs_camera,
                       rp.obs_lm, rp.obs_uv, rp.cam_model)
    T = np.array(rp.T_b_c, np.float64).reshape(2, 7).copy()
    rig = vsl.RigArrays(rp.poses, rp.cam_fixed, rp.cam_body, np.full((2, 7), np.nan) if nan_rig else T.copy())
    return arr, rig, T


def _kw(xp):
    return dict(ext_free=xp.ext_free, use_huber=xp.rp.use_huber, huber=xp.rp.huber)


def _query(ctx, vsl, xp, bodies, cams, lms, **over):
    arr, rig, T = _arrays(vsl, xp)
    kw = _kw(xp)
    kw.update(over)
    out = ctx.ba_rig_ext_covariance(arr, rig, T, bodies=bodies, cams=cams, lms=lms, **kw)
    rp = xp.rp
    assert np.array_equal(rig.body_poses, rp.poses) and np.array_equal(arr.points, rp.points) and np.array_equal(T, rp.T_b_c)
    return out


def _err(blocks, want):
    return max([float(np.abs(b - w).max()) for b, w in zip(blocks, want)], default=0.0)


def _symmetric(out):
    for k in ("cov_body", "cov_cam", "cov_point"):
        assert np.array_equal(out[k], out[k].transpose(0, 2, 1), equal_nan=True), k
    assert np.array_equal(out["cov_ext"], out["cov_ext"].T)


@pytest.mark.parametrize("name", sorted(n for n in xr.cases() if n[0] in "abcdefghijk"))
def test_full_query_against_the_reference(ctx, vsl, name):
    """a - h: every free body, every camera with a free body or a free block, every landmark, cov_ext and the cross blocks.
    b: cov_ext is 12 x 12.  i: no free body (extrinsic, cameras of fixed bodies, landmarks).  j: 138 unknowns, past the
    small dense solver.  k: multi-segment gathers; ONE landmark (every landmark has 5 groups; the cap is per landmark, the
    reference for 520 of them is what takes long)."""
    xp = xr.cases()[name]
    R = ref.reference(name)
    bodies, cams, lms = ref.full_query(xp)
    if name[0] == "k":
        lms = np.array([7])
    out = _query(ctx, vsl, xp, bodies, cams, lms)
    m = xp.n_ext
    assert out["cov_ext"].shape == (6 * m, 6 * m) and out["cov_body_ext"].shape == (len(bodies), m, 6, 6)
    assert out["n_degenerate"] == 0
    eb = _err(out["cov_body"], [R.body_block(b) for b in bodies])
    ee = _err([out["cov_ext"]], [R.ext_block()])
    ex = _err([out["cov_body_ext"][q, j] for q in range(len(bodies)) for j in range(m)],
              [R.cross_block(b, j) for b in bodies for j in range(m)])
    ec = _err(out["cov_cam"], [R.cam_block(c) for c in cams])
    el = _err(out["cov_point"], [R.point_block(l) for l in lms])
    print("%s: body %.3g, extrinsic %.3g, cross %.3g, camera %.3g, landmark %.3g (tol %.3g, cond %.3g, max|Sigma| %.3g)"
          % (name, eb, ee, ex, ec, el, R.tol, R.cond, R.tol / (64.0 * R.cond * ref.EPS)))
    assert max(eb, ee, ex, ec, el) <= R.tol, (name, eb, ee, ex, ec, el, R.tol)
    _symmetric(out)


def _solve_digest(ctx, vsl, xp):
    arr, rig, T = _arrays(vsl, xp)
    s = ctx.bundle_adjust_rig_ext(arr, rig, T, max_iters=5, **_kw(xp))
    h = hashlib.sha256()
    for a in (rig.body_poses, T, arr.points, arr.poses, np.array([s.final_cost])):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _raises(vsl, code, call):
    with pytest.raises(vsl.VslError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))


def test_gauge_window_is_reported(ctx, vsl):
    """Case l: one fixed body, the length of the baseline is a gauge direction (cond(S) 1.7e18): VSL_ERR_NUMERIC from the
    2^-36 pivot rule, and the context is left as it was -- the solve returns the same bits before and after."""
    xp = xr.cases()["l_gauge_one_fixed"]
    before = _solve_digest(ctx, vsl, xp)
    bodies, cams, lms = ref.full_query(xp)
    _raises(vsl, -7, lambda: _query(ctx, vsl, xp, bodies, cams, lms))
    _raises(vsl, -7, lambda: _query(ctx, vsl, xp, [], [], []))                       # cov_ext alone
    assert _solve_digest(ctx, vsl, xp) == before
    good = xr.cases()["a_base"]
    out = _query(ctx, vsl, good, *ref.full_query(good))
    assert np.isfinite(out["cov_ext"]).all()


@pytest.mark.parametrize("name", ["a_base", "b_both_free"])
def test_bit_properties(ctx, vsl, name):
    xp = xr.cases()[name]
    rp = xp.rp
    bodies, cams, lms = ref.full_query(xp)
    full = _query(ctx, vsl, xp, bodies, cams, lms)
    _symmetric(full)
    again = _query(ctx, vsl, xp, bodies, cams, lms)
    assert all(full[k].tobytes() == again[k].tobytes() for k in KEYS)
    # a subset, permuted, with duplicates
    pb, pc, pl = [len(bodies) - 1, 0, len(bodies) - 1], [len(cams) - 1, 1, 1, 0], [len(lms) - 2, 0, len(lms) - 2, 3]
    sub = _query(ctx, vsl, xp, bodies[pb], cams[pc], lms[pl])
    assert sub["cov_body"].tobytes() == full["cov_body"][pb].tobytes()
    assert sub["cov_body_ext"].tobytes() == full["cov_body_ext"][pb].tobytes()
    assert sub["cov_cam"].tobytes() == full["cov_cam"][pc].tobytes()
    assert sub["cov_point"].tobytes() == full["cov_point"][pl].tobytes()
    assert sub["cov_ext"].tobytes() == full["cov_ext"].tobytes()
    # one block alone; the extrinsic alone
    assert _query(ctx, vsl, xp, bodies[:1], [], [])["cov_body"][0].tobytes() == full["cov_body"][0].tobytes()
    assert _query(ctx, vsl, xp, [], cams[-1:], [])["cov_cam"][0].tobytes() == full["cov_cam"][-1].tobytes()
    assert _query(ctx, vsl, xp, [], [], lms[-1:])["cov_point"][0].tobytes() == full["cov_point"][-1].tobytes()
    assert _query(ctx, vsl, xp, [], [], [])["cov_ext"].tobytes() == full["cov_ext"].tobytes()
    # a camera of a FIXED body in a free block returns the bits of that block's cov_ext (the diagonal 6 x 6 block of a
    # 12 x 12 one)
    j = 0
    for k in (0, 1):
        if not xp.ext_free[k]:
            continue
        cam = int(np.flatnonzero((rp.cam_fixed[rp.cam_body] != 0) & (rp.cam_intr == k))[0])
        one = _query(ctx, vsl, xp, [], [cam], [])
        assert one["cov_cam"][0].tobytes() == np.ascontiguousarray(full["cov_ext"][6 * j:6 * j + 6, 6 * j:6 * j + 6]).tobytes()
        assert one["cov_cam"][0].tobytes() == full["cov_cam"][list(cams).index(cam)].tobytes()
        j += 1
    # ext_free = (0, 0) with rig.T_b_c equal to the argument: the bytes of ba_rig_covariance
    fb = np.flatnonzero(rp.cam_fixed[rp.cam_body] == 0)
    arr, rig, T = _arrays(vsl, xp, nan_rig=False)
    kw = dict(use_huber=rp.use_huber, huber=rp.huber)
    held = ctx.ba_rig_ext_covariance(arr, rig, T, ext_free=(0, 0), bodies=bodies, cams=fb, lms=lms, **kw)
    cb, cc, cl, nd = ctx.ba_rig_covariance(arr, rig, bodies, fb, lms, **kw)
    assert held["cov_body"].tobytes() == cb.tobytes() and held["cov_cam"].tobytes() == cc.tobytes()
    assert held["cov_point"].tobytes() == cl.tobytes() and held["n_degenerate"] == nd
    assert held["cov_ext"].shape == (0, 0) and held["cov_body_ext"].shape == (len(bodies), 0, 6, 6)


def test_conditioning_on_the_extrinsic_understates(ctx, vsl):
    """Case a: freeing an unknown cannot shrink a marginal.  Every diagonal entry of a body's covariance from the new
    call is >= the one vsl_ba_rig_covariance reports at the same extrinsic, and at least one is strictly greater."""
    xp = xr.cases()["a_base"]
    rp = xp.rp
    bodies = np.flatnonzero(rp.cam_fixed == 0)
    free = _query(ctx, vsl, xp, bodies, [], [])["cov_body"]
    arr, rig, T = _arrays(vsl, xp, nan_rig=False)
    held = ctx.ba_rig_covariance(arr, rig, bodies, [], [], use_huber=rp.use_huber, huber=rp.huber)[0]
    df, dh = np.diagonal(free, axis1=1, axis2=2), np.diagonal(held, axis1=1, axis2=2)
    print("a_base: body variances with the extrinsic free / held, largest ratio %.4g, smallest %.4g" % ((df / dh).max(), (df / dh).min()))
    assert (df >= dh).all() and (df > dh).any()


def _raw(ctx, vsl, xp, bodies, cams, lms, ext_free=None, T=None, ext_out=True, mutate=None):
    """The C entry with sentinel-filled outputs: (return code, True when no output was written)."""
    C = vsl.C
    arr, rig, T0 = _arrays(vsl, xp)
    if mutate:
        mutate(arr, rig)
    T = T0 if T is None else np.ascontiguousarray(T, np.float64)
    st, rg = ctx._ba_rig_structs(arr, rig)
    o = ctx._ba_opts(xp.rp.use_huber, xp.rp.huber, 0, 0)
    ef = np.ascontiguousarray(xp.ext_free if ext_free is None else ext_free, np.uint8)
    b, c, l = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (bodies, cams, lms))
    outs = [np.full(36 * max(len(b), 1), 7.0), np.full(36 * max(len(c), 1), 7.0), np.full(9 * max(len(l), 1), 7.0), np.full(144, 7.0),
            np.full(72 * max(len(b), 1), 7.0)]
    nd = C.c_int(77)
    f64p, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rc = ctx.L.vsl_ba_rig_ext_covariance(ctx.h, C.byref(st), C.byref(rg), ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p), C.byref(o),
                                         b.ctypes.data_as(i32p), len(b), outs[0].ctypes.data_as(f64p), c.ctypes.data_as(i32p), len(c),
                                         outs[1].ctypes.data_as(f64p), l.ctypes.data_as(i32p), len(l), outs[2].ctypes.data_as(f64p),
                                         outs[3].ctypes.data_as(f64p) if ext_out else None,
                                         outs[4].ctypes.data_as(f64p) if ext_out else None, C.byref(nd))
    return rc, all((x == 7.0).all() for x in outs) and nd.value == 77


def test_errors_write_nothing(ctx, vsl):
    xp = xr.cases()["a_base"]                       # bodies 0, 1 fixed; block 1 free: camera 0 is (fixed body, held block)
    rp = xp.rp
    assert rp.cam_fixed[0] and rp.cam_body[0] == 0 and rp.cam_intr[0] == 0 and rp.cam_intr[1] == 1
    before = _solve_digest(ctx, vsl, xp)
    B, Cn, L = len(rp.poses), len(rp.cam_body), len(rp.points)
    assert _raw(ctx, vsl, xp, [2], [1, 4], [0]) == (0, False)
    table = [([0], [], []), ([B], [], []), ([-1], [], []),             # a fixed body; a body out of range
             ([2], [0], []), ([2], [Cn], []), ([2], [-1], []),         # fixed body and held block; a camera out of range
             ([2], [], [L]), ([2], [], [-1])]                          # a landmark out of range
    for q in table:
        assert _raw(ctx, vsl, xp, *q) == (-1, True), q
    # what vsl_ba_rig_ext_linearize refuses: cam_body out of range; two cameras of a body in one block; a free block no
    # camera carries (every camera moved to block 0 is refused earlier: use the one-camera scene); an extrinsic that is
    # not finite
    def bad_body(arr, rig):
        rig.cam_body[3] = B
    def shared_block(arr, rig):
        arr.cam_intr[3] = 0
    assert _raw(ctx, vsl, xp, [2], [], [], mutate=bad_body) == (-1, True)
    assert _raw(ctx, vsl, xp, [2], [], [], mutate=shared_block) == (-1, True)
    Tn = np.array(rp.T_b_c, np.float64).reshape(2, 7).copy()
    Tn[1, 5] = np.inf
    assert _raw(ctx, vsl, xp, [2], [], [], T=Tn) == (-1, True)
    mono = xr.ExtProblem(rr.rig_scene(4, 2, 9, 612, cams_of_body=[(0,)] * 4), (0, 1))
    assert _raw(ctx, vsl, mono, [2], [], []) == (-1, True)
    # no fixed body: VSL_ERR_NUMERIC before any device work
    def all_free(arr, rig):
        rig.body_fixed[:] = 0
    assert _raw(ctx, vsl, xp, [2], [], [], mutate=all_free) == (-7, True)
    # all counts zero and null extrinsic outputs: validates, launches nothing
    rc, untouched = _raw(ctx, vsl, xp, [], [], [], ext_out=False)
    assert rc == 0 and not untouched                                   # (*n_degenerate = 0 is written)
    assert _solve_digest(ctx, vsl, xp) == before


def test_group_cap(ctx, vsl):
    """A landmark seen by 256 free bodies of a free block has 257 groups: VSL_ERR_INVALID when it is queried, alone or
    after another.  The cap is per QUERIED landmark: the other one is not refused (two landmarks do not determine this
    window: VSL_ERR_NUMERIC is an answer here, VSL_ERR_INVALID is not)."""
    rp = rr.rig_scene(258, 2, 2, 613, cams_of_body=[(0,)] * 258)
    rp = rr._drop(rp, ~((rp.obs_lm == 1) & (rp.obs_camera > 20)))
    xp = xr.ExtProblem(rp, (1, 0))
    assert _raw(ctx, vsl, xp, [], [], [0]) == (-1, True)
    assert _raw(ctx, vsl, xp, [], [], [1, 0]) == (-1, True)
    assert _raw(ctx, vsl, xp, [], [], [1])[0] in (0, -7)
