"""GPU: the device stereo stage (visual-slam_amd/csrc/stereo.hip: epipolar inliers + midpoint triangulation) against the
host restatement the pipeline runs (include/visnav_amd/harness/odometry.h find_inliers_essential, harness/pnp.h
triangulate_midpoint) -- through the host-buffer entry, the drop-in matching_utils.h, the frame store, and the headless
pipeline with --fused --device-stereo.  ds / pinhole / eucm: bit for bit (a NaN must meet a NaN); kb4 (device sin / cos):
bearings within 4 ulp, equal inlier decisions except within 1e-12 of the threshold, points within 4 ulp scaled by the
triangulation's condition number (DESIGN.md "Stereo inliers and triangulation")."""
import importlib
import json
import subprocess

import numpy as np
import pytest

import stereo_ref as sr
from stereo_ref import ROOT

pytestmark = pytest.mark.gpu

GOLD = ROOT / "tests" / "golden"
EXE = ROOT / "visual-slam_amd" / "slam_headless"


@pytest.fixture(scope="module")
def exe(tmp_path_factory, vsl):
    return sr.compile_stereo_test(tmp_path_factory.mktemp("stereo") / "stereo_test")


@pytest.fixture(scope="module")
def rig(exe):
    E, R, t = sr.essential(exe, sr.calib_pose7())
    return dict(E=E, R=R, t=t, ca=(sr.DS, sr.CAMS[sr.DS]), cb=(sr.DS, _ds_right()))


def _ds_right():
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    c = sq.CALIB["intrinsics"][1]
    return [c["fx"], c["fy"], c["cx"], c["cy"], c["p1"], c["p2"], 0.0, 0.0]


def _euroc():
    return [np.load(GOLD / ("euroc_pair%d.npz" % k)) for k in range(16)]


KB4_WORST = [0.0]   # largest kb4 point difference seen, in units of ulp(|p|) * cond


def _check(model, got_pairs, got_pts, want_pairs, want_pts, err=None, thr=None, cond=None, want_err_idx=None):
    """Exact for ds / pinhole / eucm; the kb4 tolerance otherwise.  Returns the number of near-threshold decisions."""
    if model != sr.KB4:
        assert np.array_equal(got_pairs, want_pairs)
        if want_pts is not None:
            assert sr.same_bits(got_pts, want_pts)
        return 0
    # kb4: decisions may differ only for matches whose |err| lies within 1e-12 of the threshold
    g = {tuple(p) for p in got_pairs}
    w = {tuple(p) for p in want_pairs}
    near = 0
    for p in g ^ w:
        k = want_err_idx[p]
        assert abs(abs(err[k]) - thr) <= 1e-12, (p, err[k], thr)
        near += 1
    common = [i for i, p in enumerate(map(tuple, want_pairs)) if p in g]
    gi = {p: i for i, p in enumerate(map(tuple, got_pairs))}
    gsel = [gi[tuple(want_pairs[i])] for i in common]
    if want_pts is not None and common:
        # a point is an ill-conditioned function of its two bearings: a one-ulp change of a bearing moves it by about
        # cond = |d1|^2 |d2|^2 / |den| ulp of |p| (thousands at an 11 cm baseline).  Bound: 16 ulp of |p| times cond.
        a, b = got_pts[gsel], want_pts[common]
        assert np.array_equal(np.isnan(a), np.isnan(b))
        fin = np.all(np.isfinite(b), axis=1)
        unit = np.spacing(np.linalg.norm(b[fin], axis=1)) * np.maximum(1.0, cond[common][fin])
        ratio = np.linalg.norm(a[fin] - b[fin], axis=1) / unit
        assert np.all(ratio <= 16), ratio.max()
        KB4_WORST[0] = max(KB4_WORST[0], float(ratio.max()) if len(ratio) else 0.0)
    return near


# ----------------------------------------------------------------------------------------- real data: 16 EuRoC pairs
def test_euroc_pairs_host_buffer_entry_and_dropin_are_the_host_s(exe, rig, tmp_path):
    total = 0
    for g in _euroc():
        got = sr.run_stereo_test(exe, tmp_path, sr.DS, rig["ca"][1], sr.DS, rig["cb"][1], rig["E"], rig["R"], rig["t"], 1e-3,
                                 g["xy0"].astype(np.float64), g["xy1"].astype(np.float64), g["matches"], device=True)
        hp, hx = got["host"]
        assert np.array_equal(got["dev"][0], hp) and sr.same_bits(got["dev"][1], hx)
        assert np.array_equal(got["dropin"], hp)
        assert 0 < len(hp) <= len(g["matches"])
        total += len(hp)
    assert total > 500


def _store_pass(vsl, ctx, imgs, pairs, F=1500, num_features=1500):
    fr = vsl.Frames(ctx, len(imgs), imgs[0].shape[1], imgs[0].shape[0], F, max(1, len(pairs)))
    fr.upload(0, np.stack(imgs))
    fr.detect_describe(0, len(imgs), num_features)
    fr.resolve_ties()
    fr.match(np.array(pairs, np.int32))
    return fr


def test_euroc_store_path_is_the_host_s(exe, rig, ctx, vsl, tmp_path):
    gs = _euroc()
    imgs = [g["img%d" % c] for g in gs for c in range(2)]
    fr = _store_pass(vsl, ctx, imgs, [(2 * k, 2 * k + 1) for k in range(16)])
    fr.stereo_inliers(0, 16, rig["ca"], rig["cb"], rig["E"], rig["R"], rig["t"], 1e-3)
    counts = fr.inlier_counts(16)
    for k in range(16):
        xa, xb = fr.keypoints(2 * k)[0], fr.keypoints(2 * k + 1)[0]
        m = fr.matches(k)
        host = sr.run_stereo_test(exe, tmp_path, sr.DS, rig["ca"][1], sr.DS, rig["cb"][1], rig["E"], rig["R"], rig["t"], 1e-3,
                                  xa, xb, m)["host"]
        p, x = fr.inliers(k)
        assert counts[k] == len(p)
        assert np.array_equal(p, host[0]) and sr.same_bits(x, host[1])
    fr.close()


# ----------------------------------------------------------------------------------------- synthetic rigs, every model
@pytest.mark.parametrize("model", [sr.DS, sr.PINHOLE, sr.EUCM, sr.KB4])
def test_synthetic_rigs_every_model(ctx, model):
    prm = sr.CAMS[model]
    near = 0
    for seed in range(4):
        r = sr.synthetic_rig(model, 100 + seed)
        for thr in (1e-3, 3e-3, 0.0, np.inf):
            gp, gx = ctx.find_inliers_essential((model, prm), (model, prm), r["E"], r["xy_a"], r["xy_b"], r["matches"], thr,
                                                r["R"], r["t"])
            wp, wx, err, cond = sr.stage(model, prm, model, prm, r["E"], r["R"], r["t"], thr, r["xy_a"], r["xy_b"], r["matches"])
            idx = {tuple(p): i for i, p in enumerate(map(tuple, r["matches"]))}
            near += _check(model, gp, gx, wp, wx, err, thr, cond, idx)
            if thr == np.inf:
                assert len(gp) == len(r["matches"])
            if thr == 1e-3:
                assert 0 < len(gp) < len(r["matches"])
            # inlier lists only
            gp2, gx2 = ctx.find_inliers_essential((model, prm), (model, prm), r["E"], r["xy_a"], r["xy_b"], r["matches"], thr)
            assert np.array_equal(gp2, gp) and gx2 is None
    print("model %d: %d near-threshold decisions differ; kb4 points so far within %.2f ulp(|p|) * cond" % (model, near, KB4_WORST[0]))


@pytest.mark.parametrize("model", [sr.DS, sr.PINHOLE, sr.EUCM, sr.KB4])
def test_parallel_rays_and_bearings(ctx, model):
    # identical pixels on both sides, R = I: identical bearings, den = 0 exactly, p = 1e6 * bearing -- the bearings themselves
    prm = sr.CAMS[model]
    xs, ys = np.meshgrid(np.arange(0, sr.W, 37.0), np.arange(0, sr.H, 29.0))
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    m = np.stack([np.arange(len(xy))] * 2, 1).astype(np.int32)
    gp, gx = ctx.find_inliers_essential((model, prm), (model, prm), np.zeros((3, 3)), xy, xy, m, 1e-3, np.eye(3), [0.11, 0, 0])
    assert len(gp) == len(m)
    b = np.stack(sr.unproject(model, prm, xy[:, 0], xy[:, 1]), 1)
    want = 1e6 * b
    if model == sr.KB4:
        u = sr.ulp_diff(gx.ravel(), want.ravel())
        print("kb4 bearings: max %d ulp" % u.max())
        assert u.max() <= 5   # 4 ulp on the bearing, one more rounding in the product with 1e6
    else:
        assert sr.same_bits(gx, want)


def test_nan_bearings_are_inliers(ctx):
    prm = list(sr.CAMS[sr.DS])
    prm[5] = 0.9  # alpha > 0.5: pixels outside the valid disc unproject to NaN
    rng = np.random.default_rng(5)
    xy = np.stack([rng.integers(-900, 1700, 300), rng.integers(-900, 1400, 300)], 1).astype(np.float64)
    m = np.stack([np.arange(300), rng.permutation(300)], 1).astype(np.int32)
    r = sr.synthetic_rig(sr.DS, 1)
    gp, gx = ctx.find_inliers_essential((sr.DS, prm), (sr.DS, prm), r["E"], xy, xy, m, 1e-3, r["R"], r["t"])
    wp, wx, err, _ = sr.stage(sr.DS, prm, sr.DS, prm, r["E"], r["R"], r["t"], 1e-3, xy, xy, m)
    assert np.isnan(err).sum() > 50
    assert np.array_equal(gp, wp) and sr.same_bits(gx, wx)
    assert np.isnan(gx).any()


def test_argument_errors(ctx, vsl):
    prm = sr.CAMS[sr.DS]
    xy = np.zeros((4, 2))
    with pytest.raises(vsl.VslError) as e:
        ctx.find_inliers_essential((7, prm), (sr.DS, prm), np.eye(3), xy, xy, [[0, 0]])
    assert e.value.code == -1
    with pytest.raises(vsl.VslError) as e:
        ctx.find_inliers_essential((sr.DS, prm), (sr.DS, prm), np.eye(3), xy, xy, [[0, 4]])
    assert e.value.code == -1
    p, x = ctx.find_inliers_essential((sr.DS, prm), (sr.DS, prm), np.eye(3), xy, xy, np.zeros((0, 2)), 1e-3, np.eye(3), [1, 0, 0])
    assert len(p) == 0 and len(x) == 0
    g = _euroc()[0]
    fr = _store_pass(vsl, ctx, [g["img0"], g["img1"]], [(0, 1)])
    with pytest.raises(vsl.VslError) as e:
        fr.inlier_counts(1)   # the stage has not run on this store
    assert e.value.code == -1
    with pytest.raises(vsl.VslError) as e:
        fr.stereo_inliers(0, 2, (sr.DS, prm), (sr.DS, prm), np.eye(3))   # max_pairs = 1
    assert e.value.code == -1
    with pytest.raises(vsl.VslError) as e:
        fr.stereo_inliers(0, 1, (4, prm), (sr.DS, prm), np.eye(3))
    assert e.value.code == -1
    fr.stereo_inliers(0, 1, (sr.DS, prm), (sr.DS, prm), np.zeros((3, 3)), triangulate=False)   # all inliers, no points
    with pytest.raises(vsl.VslError) as e:
        fr.inliers(0)   # points of a pair that was not triangulated
    assert e.value.code == -1
    p, _ = fr.inliers(0, points=False)
    assert np.array_equal(p, g["matches"])
    n = ctx.L.vsl_frames_download_inliers(ctx.h, fr.h, 0, 3, np.zeros(8, np.int32).ctypes.data_as(vsl.i32p), None,
                                          vsl.C.byref(vsl.C.c_int32()))
    assert n == -4   # VSL_ERR_CAPACITY
    fr.close()


# ----------------------------------------------------------------------------------------- scale, ranges, determinism
def test_store_1024_images_512_pairs(ctx, vsl, rig):
    gs = _euroc()
    base = [g["img%d" % c] for g in gs for c in range(2)]
    imgs = []
    for copy in range(32):
        for k in range(32):
            imgs.append(np.roll(base[k], 3 * copy, axis=1) if copy else base[k])
    imgs[1022] = np.zeros_like(imgs[0])   # a pair with no keypoints, hence no matches
    imgs[1023] = np.zeros_like(imgs[0])
    pairs = [(2 * k, 2 * k + 1) for k in range(512)]
    fr = _store_pass(vsl, ctx, imgs, pairs)
    kps = [fr.keypoints(s)[0] for s in range(1024)]
    ms = [fr.matches(k) for k in range(512)]
    assert len(ms[511]) == 0 and sum(len(m) for m in ms) > 40000
    runs = []
    for model in (sr.DS, sr.PINHOLE, sr.EUCM, sr.KB4):
        ca = (model, sr.CAMS[model]) if model != sr.DS else rig["ca"]
        cb = (model, sr.CAMS[model]) if model != sr.DS else rig["cb"]
        fr.stereo_inliers(0, 512, ca, cb, rig["E"], rig["R"], rig["t"], 1e-3)
        got = [fr.inliers(k) for k in range(512)]
        near = 0
        for k in range(512):
            wp, wx, err, cond = sr.stage(model, ca[1], model, cb[1], rig["E"], rig["R"], rig["t"], 1e-3, kps[2 * k], kps[2 * k + 1],
                                         ms[k])
            idx = {tuple(p): i for i, p in enumerate(map(tuple, ms[k]))}
            near += _check(model, got[k][0], got[k][1], wp, wx, err, 1e-3, cond, idx)
        print("1024-image store, model %d: %d inliers, %d near-threshold decisions differ, kb4 points within %.2f ulp(|p|) * cond"
              % (model, sum(len(g[0]) for g in got), near, KB4_WORST[0]))
        if model == sr.DS:
            runs.append(got)
    # determinism: the same launch again, byte for byte
    fr.stereo_inliers(0, 512, rig["ca"], rig["cb"], rig["E"], rig["R"], rig["t"], 1e-3)
    again = [fr.inliers(k) for k in range(512)]
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(runs[0], again))
    # a range that does not start at pair 0 leaves the other pairs alone
    before = fr.inlier_counts(512)
    fr.stereo_inliers(100, 64, rig["ca"], rig["cb"], rig["E"], rig["R"], rig["t"], np.inf)
    after = fr.inlier_counts(512)
    assert np.array_equal(after[:100], before[:100]) and np.array_equal(after[164:], before[164:])
    assert all(after[k] == len(ms[k]) for k in range(100, 164))
    for k in (100, 163):
        p, x = fr.inliers(k)
        wp, wx, _, _ = sr.stage(sr.DS, rig["ca"][1], sr.DS, rig["cb"][1], rig["E"], rig["R"], rig["t"], np.inf, kps[2 * k],
                                kps[2 * k + 1], ms[k])
        assert np.array_equal(p, wp) and sr.same_bits(x, wx)
    fr.close()


def test_full_store_capacity(ctx, vsl, rig):
    # a store of max_features = F whose image holds F keypoints, matched against itself
    g = _euroc()[3]
    F = 200
    img = g["img0"].copy()
    img[:24], img[-24:], img[:, :24], img[:, -24:] = 128, 128, 128, 128   # no corner is dropped by the border test
    fr = _store_pass(vsl, ctx, [img, g["img1"]], [(0, 0), (1, 0)], F=F, num_features=F)
    xa = fr.keypoints(0)[0]
    m = fr.matches(0)
    assert len(xa) == F and len(m) > F // 2, len(m)   # (the matcher's ratio test drops keypoints with near-twin descriptors)
    fr.stereo_inliers(0, 2, rig["ca"], rig["ca"], np.zeros((3, 3)), np.eye(3), rig["t"], 0.0)
    p, x = fr.inliers(0)
    wp, wx, _, _ = sr.stage(sr.DS, rig["ca"][1], sr.DS, rig["ca"][1], np.zeros((3, 3)), np.eye(3), rig["t"], 0.0, xa, xa, m)
    assert len(p) == len(m) and np.array_equal(p, wp) and sr.same_bits(x, wx)
    assert np.all(np.linalg.norm(x, axis=1) > 9e5)   # identical bearings, R = I: 1e6 * bearing everywhere
    print("store of F = %d: %d keypoints, %d self-matches" % (F, len(xa), len(m)))
    fr.close()


# ----------------------------------------------------------------------------------------- end to end
def _run(seq_dir, *extra):
    r = subprocess.run([str(EXE), "--dataset-path", str(seq_dir), "--cam-calib", str(seq_dir / "calib.json"), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _same_run(seq_dir, tmp_path, *extra):
    t0, t1 = tmp_path / "fused.csv", tmp_path / "device_stereo.csv"
    a = _run(seq_dir, "--traj", str(t0), "--fused", *extra)
    b = _run(seq_dir, "--traj", str(t1), "--fused", "--device-stereo", *extra)
    assert b["device_stereo"] is True and a["device_stereo"] is False
    assert t0.read_bytes() == t1.read_bytes()
    assert (a["keyframes"], a["landmarks"], a["active_landmarks"]) == (b["keyframes"], b["landmarks"], b["active_landmarks"])
    print("stage_ms_total fused:", a["stage_ms_total"], "device stereo:", b["stage_ms_total"], "keyframes", a["keyframes"])
    return a, b


def test_end_to_end_real_frames(tmp_path, vsl):
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    d = tmp_path / "real"
    stamps = []
    for c in range(2):
        (d / ("cam%d" % c) / "data").mkdir(parents=True)
    for k in range(6, 16):
        g = np.load(GOLD / ("euroc_pair%d.npz" % k))
        s = int(str(g["stamp"]))
        stamps.append(s)
        for c in range(2):
            sq.write_png(str(d / ("cam%d" % c) / "data" / ("%d.png" % s)), g["img%d" % c], level=1)
    for c in range(2):
        with open(d / ("cam%d" % c) / "data.csv", "w", newline="") as f:
            f.write("#timestamp [ns],filename\r\n")
            for s in stamps:
                f.write("%d,%d.png\r\n" % (s, s))
    sq.write_calibration(str(d / "calib.json"))
    a, _ = _same_run(d, tmp_path)
    assert a["frames"] == 10 and a["landmarks"] > 100


def test_end_to_end_rendered_sequence(tmp_path, vsl):
    sq = importlib.import_module("visual_slam_amd.synth_sequence")
    d = tmp_path / "seq"
    sq.render_sequence(str(d), n_frames=90, seed=1, step_m=0.04, radius=1.6)
    a, _ = _same_run(d, tmp_path, "--kf-min-inliers", "500")
    assert a["frames"] == 90 and a["keyframes"] >= 5
