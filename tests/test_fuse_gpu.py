"""GPU parity of vsl_fuse_search (visual-slam_amd/csrc/fuse.hip): for every view, its segment of pairs and its
n_projected must EQUAL what vsl_project_landmarks followed by vsl_find_matches_landmarks return on that view -- on the
device (the two operators as they are) and on the CPU oracle.  Every assertion is an equality.

Fixtures follow the planting recipe of tests/test_vo_gpu.py::_match_case with the roles turned round, because here
the projections come from 3-D points and not from a list of pixels: a planted keypoint sits on integer pixels within
+-12 px of the projection of a landmark of its view, and one observation of that landmark is a copy of the keypoint's
descriptor with 0 / 0 / 3 / 20 / 50 / 69 / 70 / 75 flipped bits (the same list: both sides of the threshold of 70)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 752, 480
INTR = {0: [351.0, 350.0, 365.9, 249.3, -0.2385, 0.5679, 0, 0], 1: [351.0, 350.0, 365.9, 249.3, 0, 0, 0, 0],
        2: [351.0, 350.0, 365.9, 249.3, 0.6, 1.1, 0, 0], 3: [351.0, 350.0, 365.9, 249.3, 0.01, -0.004, 0.002, -0.0005]}
PARAMS = (0.1, 20.0, 70, 1.2)  # cam_z_threshold, match_max_dist_2d, feature_match_threshold, feature_match_dist_2_best


def _case(ctx, synth, seed, model, kps, n_lms, max_obs, planted=0.6, away=()):
    """kps[v] keypoints in view v; the views look at one cloud of n_lms landmarks from poses a few degrees / decimetres
    apart; a view listed in `away` is turned by 180 degrees (nothing projects)."""
    rng = np.random.default_rng(seed)
    base = np.concatenate([synth.axis_angle_q(rng.normal(size=3), 0.3), rng.normal(0, 0.5, 3)])
    pc = np.stack([rng.uniform(-8, 8, n_lms), rng.uniform(-5, 5, n_lms), rng.uniform(-2, 12, n_lms)], -1)
    pw = pc @ synth.quat_R(base[:4]).T + base[4:]
    n_obs = rng.integers(0, max_obs + 1, n_lms)
    start = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    obs = synth.random_descriptors(rng, int(start[-1]))
    poses, kp_xy, kp_desc = [], [], []
    for v, n_kp in enumerate(kps):
        if v in away:  # 5 m behind the cloud (its depth is -2 .. 12 m in the base frame), facing backwards
            rel = np.concatenate([synth.axis_angle_q([0.0, 1.0, 0.0], np.pi), [0.0, 0.0, -5.0]])
        else:
            rel = np.concatenate([synth.axis_angle_q(rng.normal(size=3), 0.05), rng.normal(0, 0.1, 3)])
        pose = synth.se3_mul(base, rel)
        poses.append(pose)
        xy = np.stack([rng.integers(19, 733, n_kp), rng.integers(19, 461, n_kp)], -1).astype(np.float64)
        desc = synth.random_descriptors(rng, n_kp)
        uv, idx = ctx.project_landmarks(pose, model, INTR[model], W, H, pw, PARAMS[0])
        for k in range(n_kp):
            if len(idx) and rng.random() < planted:
                j = int(rng.integers(len(idx)))
                l = int(idx[j])
                if n_obs[l] == 0:
                    continue
                xy[k] = np.clip(np.round(uv[j] + rng.uniform(-12, 12, 2)), [0, 0], [W - 1, H - 1])
                o = int(start[l] + rng.integers(n_obs[l]))
                obs[o] = synth.flip_bits(rng, desc[k:k + 1], int(rng.choice([0, 0, 3, 20, 50, 69, 70, 75])))[0]
        kp_xy.append(xy)
        kp_desc.append(desc)
    return dict(poses=np.array(poses), model=model, intr=INTR[model], w=W, h=H, kp_xy=kp_xy, kp_desc=kp_desc, points=pw,
                start=start, obs=obs)


def _fused(ctx, c, params=PARAMS):
    return ctx.fuse_search(c["poses"], c["model"], c["intr"], c["w"], c["h"], c["kp_xy"], c["kp_desc"], c["points"],
                           c["start"], c["obs"], *params)


def _per_view(op, c, params=PARAMS):
    """the parent's way: project_landmarks + find_matches_landmarks, view by view, on `op` (the device context or the oracle)"""
    z, r, t, q = params
    pairs, n_proj = [], []
    for v in range(len(c["poses"])):
        uv, idx = op.project_landmarks(c["poses"][v], c["model"], c["intr"], c["w"], c["h"], c["points"], z)
        n_proj.append(len(idx))
        pairs.append(np.asarray(op.find_matches_landmarks(c["kp_xy"][v], c["kp_desc"][v], uv, idx, c["start"], c["obs"], r, t, q),
                                np.int32).reshape(-1, 2))
    return pairs, np.array(n_proj, np.int32)


def _check(ctx, orc, c, params=PARAMS):
    got, got_np = _fused(ctx, c, params)
    assert len(got) == len(c["poses"]) and got_np.dtype == np.int32
    for name, op in (("device operators", ctx), ("oracle", orc)):
        exp, exp_np = _per_view(op, c, params)
        assert np.array_equal(got_np, exp_np), name
        for v in range(len(exp)):
            assert got[v].dtype == np.int32 and got[v].shape == exp[v].shape and np.array_equal(got[v], exp[v]), (name, v)
    return got, got_np


def test_one_view_one_keypoint_one_landmark(ctx, orc, synth):
    for seed in range(4):  # planted or not, zero to three observations
        _check(ctx, orc, _case(ctx, synth, 10 + seed, 0, [1], 1, 3, planted=1.0))


def test_empty_view_chunk_boundary_and_odd_keypoint_count(ctx, orc, synth):
    c = _case(ctx, synth, 2, 0, [0, 257, 64], 1100, 20)
    got, n_proj = _check(ctx, orc, c)
    assert len(got[0]) == 0 and n_proj[0] > 0 and len(got[1]) > 0 and len(got[2]) > 0
    for params in ((0.1, 5.0, 70, 1.2), (0.1, 40.0, 100, 1.0), (3.0, 20.0, 1, 3.0)):
        _check(ctx, orc, c, params)


def test_sixteen_views(ctx, orc, synth):
    c = _case(ctx, synth, 3, 0, [290 + 3 * v for v in range(16)], 2500, 70)
    got, n_proj = _check(ctx, orc, c)
    assert max(len(p) for p in got) > 50 and n_proj.min() > 0


def test_view_that_looks_away(ctx, orc, synth):
    c = _case(ctx, synth, 4, 0, [64, 64, 64], 300, 20, away=(1,))
    got, n_proj = _check(ctx, orc, c)
    assert n_proj[1] == 0 and len(got[1]) == 0 and n_proj[0] > 0 and n_proj[2] > 0 and len(got[2]) > 0


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_each_camera_model(ctx, orc, synth, model):
    got, n_proj = _check(ctx, orc, _case(ctx, synth, 20 + model, model, [64, 64], 300, 20))
    assert 0 < n_proj.min() and n_proj.max() < 300 and sum(len(p) for p in got) > 0


def _pixel_case(kp, kp_desc, pts, start, obs):
    """View 1 of 2 sees the landmarks EXACTLY at the pixels pts: pinhole with fx = fy = 1, cx = cy = 0, the identity
    pose and points (u, v, 1) give u = 1 * u / 1 + 0 with no rounding.  View 0 looks at the same points with three
    keypoints of its own."""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    ident = [0.0, 0, 0, 1, 0, 0, 0]
    xy0 = np.array([[100.0, 100.0], [300.0, 200.0], [10.0, 10.0]])
    d0 = np.zeros((3, 4), np.uint64)
    d0[1] = 0xFFFF
    return dict(poses=np.array([ident, ident]), model=1, intr=[1.0, 1.0, 0, 0, 0, 0, 0, 0], w=100000, h=100000,
                kp_xy=[xy0, np.asarray(kp, np.float64)], kp_desc=[d0, np.asarray(kp_desc, np.uint64)],
                points=np.concatenate([pts, np.ones((len(pts), 1))], 1), start=np.asarray(start, np.int32), obs=obs)


def _bits(n):
    o = np.zeros(4, np.uint64)
    for b in range(n):
        o[b // 64] |= np.uint64(1) << np.uint64(b % 64)
    return o


def test_tie_semantics_in_view_one_of_two(ctx, orc):
    # the partial_sort tie cases of tests/test_vo_gpu.py::test_find_matches_tie_semantics
    z = np.zeros(4, np.uint64)
    for dists in ([0, 0], [0, 7, 0], [7, 0, 0], [0, 0, 0], [5, 0, 9, 0, 3], [3, 3], [4, 2, 2, 9, 2], [9, 8, 7, 6, 5, 5, 6, 5]):
        proj = [[100.0 + 0.1 * i, 100.0] for i in range(len(dists))]
        c = _pixel_case([[100.0, 100.0]], [z], proj, np.arange(len(dists) + 1), np.stack([_bits(v) for v in dists]))
        got, n_proj = _check(ctx, orc, c, (0.1, 20.0, 70, 1.0))
        assert n_proj.tolist() == [len(dists)] * 2 and len(got[1]) == 1, dists


def test_radius_boundary_in_view_one_of_two(ctx, orc):
    # the points of tests/test_vo_gpu.py::test_find_matches_radius_boundary: on the circle, one ulp inside / outside it
    z = np.zeros(4, np.uint64)
    for radius in (20.0, 5.0, 0.1, 19.999999999999996, 7.3, 1e-3, 123.456):
        pts = []
        for ang in np.linspace(0.0, 2 * np.pi, 97):
            for scale in (1.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 1 - 1e-15, 1 + 1e-15, 1 - 3e-16, 1 + 3e-16):
                pts.append([300.0 + radius * scale * np.cos(ang), 200.0 + radius * scale * np.sin(ang)])
        if radius == 20.0:
            pts += [[312.0, 216.0], [288.0, 184.0], [312.0, np.nextafter(216.0, 0)], [312.0, np.nextafter(216.0, 1e9)]]
        pts = np.asarray(pts)
        n = len(pts)
        obs = np.stack([_bits(i % 60) for i in range(n)])
        params = (0.1, radius, 70, 1.0)
        for sub in (slice(0, n), slice(n // 3, n), slice(0, n, 7), slice(5, n, 11)):
            m = len(pts[sub])
            _check(ctx, orc, _pixel_case([[300.0, 200.0]], [z], pts[sub], np.arange(m + 1), obs[sub]), params)
        for i in list(range(0, 97 * 7, 13)) + list(range(97 * 7, n)):  # hit / no hit, landmark by landmark
            _check(ctx, orc, _pixel_case([[300.0, 200.0]], [z], pts[i:i + 1], [0, 1], obs[:1]), params)


def test_two_runs_give_identical_bytes(ctx, synth):
    c = _case(ctx, synth, 2, 0, [0, 257, 64], 1100, 20)
    a, a_np = _fused(ctx, c)
    big = _case(ctx, synth, 5, 0, [300] * 4, 2500, 20)  # another shape in between: the scratch is reused
    _fused(ctx, big)
    b, b_np = _fused(ctx, c)
    assert a_np.tobytes() == b_np.tobytes()
    assert [p.tobytes() for p in a] == [p.tobytes() for p in b]


def test_empty_inputs(ctx, synth):
    c = _case(ctx, synth, 6, 0, [5, 7], 40, 3)
    e = dict(c, poses=np.zeros((0, 7)), kp_xy=[], kp_desc=[])
    got, n_proj = _fused(ctx, e)
    assert got == [] and len(n_proj) == 0
    e = dict(c, points=np.zeros((0, 3)), start=np.zeros(1, np.int32), obs=np.zeros((0, 4), np.uint64))
    got, n_proj = _fused(ctx, e)
    assert [len(p) for p in got] == [0, 0] and n_proj.tolist() == [0, 0]
    e = dict(c, kp_xy=[np.zeros((0, 2))] * 2, kp_desc=[np.zeros((0, 4), np.uint64)] * 2)
    got, n_proj = _fused(ctx, e)
    assert [len(p) for p in got] == [0, 0]
    assert n_proj.tolist() == [len(ctx.project_landmarks(p, 0, INTR[0], W, H, c["points"], 0.1)[1]) for p in c["poses"]]


def test_bad_arguments(vsl, ctx):
    L = ctx.L
    f64p, i32p, u64p = vsl.f64p, vsl.i32p, vsl.u64p
    pose = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (65, 1))
    intr = np.array(INTR[0])
    kp_start = np.array([0, 2] + [2] * 64, np.int32)
    xy = np.zeros((2, 2))
    desc = np.zeros((2, 4), np.uint64)
    pts = np.ones((3, 3))
    ls = np.array([0, 1, 2, 3], np.int32)
    od = np.zeros((3, 4), np.uint64)
    pairs = np.zeros((2, 2), np.int32)
    ps = np.zeros(66, np.int32)

    def call(n_views=1, pose=pose, kp_start=kp_start, xy=xy, desc=desc, n_lms=3, pts=pts, ls=ls, od=od, pairs=pairs, ps=ps):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
        return L.vsl_fuse_search(ctx.h, n_views, p(pose, f64p), 0, p(intr, f64p), W, H, p(kp_start, i32p), p(xy, f64p),
                                 p(desc, u64p), n_lms, p(pts, f64p), p(ls, i32p), p(od, u64p), C.c_double(0.1), C.c_double(20.0),
                                 70, C.c_double(1.2), p(pairs, i32p), p(ps, i32p), None)

    assert call() == 0  # the arguments are good (and a null n_projected is allowed)
    bad = [dict(pose=None), dict(kp_start=None), dict(xy=None), dict(desc=None), dict(pts=None), dict(ls=None), dict(od=None),
           dict(pairs=None), dict(ps=None), dict(n_views=65), dict(n_views=-1), dict(n_lms=-1),
           dict(n_views=2, kp_start=np.array([0, 2, 1], np.int32)), dict(ls=np.array([0, 2, 1, 3], np.int32))]
    for kw in bad:
        assert call(**kw) == -1, kw  # VSL_ERR_INVALID
        assert b"vsl_fuse_search" in L.vsl_last_error(ctx.h), kw
    assert call() == 0
