"""Wide maps for the iterative-Schur tests: stereo keyframes on a circle looking INWARD at one small point cloud, so that
almost every camera pair is covisible and the reduced camera system has no narrow band (the direct route stores it
dense).  Built from visual-slam_amd/synth.py's helpers; plus the CPU reference of the solver under test: block-Jacobi
preconditioned conjugate gradients on a dense S in float64."""
import numpy as np


def wide(synth, seed, n_kf, n_lms, radius=6.0, max_obs_per_lm=None, pix_noise=0.5, outlier_frac=0.05,
         pose_noise=(0.02, 0.0087), point_noise=0.05):
    """Dict in the layout of synth.ba_problem.  max_obs_per_lm: keep at most that many observations of a landmark
    (chosen at random), for maps with more cameras than a landmark run of the recompute form takes."""
    rng = np.random.default_rng(seed)
    n_cams = 2 * n_kf
    poses = np.zeros((n_cams, 7))
    for k in range(n_kf):
        a = 2 * np.pi * k / n_kf
        q = synth.axis_angle_q([0, 1, 0], a + np.pi)  # optical axis towards the centre
        t = np.array([radius * np.sin(a), 0.05 * np.sin(5 * a), radius * np.cos(a)])
        poses[2 * k] = np.concatenate([q, t])
        poses[2 * k + 1] = synth.se3_mul(poses[2 * k], synth.T_0_1)
    pts = rng.uniform(-1, 1, (n_lms, 3)) * np.array([1.6, 1.0, 1.6])
    cam_intr = np.tile(np.array([0, 1], np.int32), n_kf)
    obs_cam, obs_lm, obs_uv = [], [], []
    for c in range(n_cams):
        R = synth.quat_R(poses[c, :4])
        pc = (pts - poses[c, 4:]) @ R
        uv, den = synth.ds_project(synth.DS_INTR[cam_intr[c]], pc)
        ok = (pc[:, 2] > 0.3) & (den > 0) & (uv[:, 0] >= 19) & (uv[:, 0] < synth.W - 19) & (uv[:, 1] >= 19) & \
             (uv[:, 1] < synth.H - 19)
        idx = np.nonzero(ok)[0]
        obs_cam.append(np.full(len(idx), c, np.int32))
        obs_lm.append(idx.astype(np.int32))
        obs_uv.append(uv[idx])
    obs_cam, obs_lm, obs_uv = np.concatenate(obs_cam), np.concatenate(obs_lm), np.concatenate(obs_uv)
    if max_obs_per_lm is not None:
        key = rng.random(len(obs_lm))
        order = np.lexsort((key, obs_lm))
        rank = np.arange(len(order)) - np.searchsorted(obs_lm[order], obs_lm[order], side="left")
        keep = np.zeros(len(order), bool)
        keep[order[rank < max_obs_per_lm]] = True
        obs_cam, obs_lm, obs_uv = obs_cam[keep], obs_lm[keep], obs_uv[keep]
    cnt = np.bincount(obs_lm, minlength=n_lms)
    keep = cnt >= 2
    remap = -np.ones(n_lms, np.int64)
    remap[keep] = np.arange(keep.sum())
    sel = keep[obs_lm]
    obs_cam, obs_lm, obs_uv = obs_cam[sel], remap[obs_lm[sel]].astype(np.int32), obs_uv[sel]
    pts = pts[keep]
    order = np.lexsort((obs_cam, obs_lm))
    obs_cam, obs_lm, obs_uv = obs_cam[order], obs_lm[order], obs_uv[order]
    noise = rng.normal(0, pix_noise, obs_uv.shape)
    out = rng.random(len(obs_uv)) < outlier_frac
    noise[out] = rng.normal(0, 20.0, (out.sum(), 2))
    obs_uv = np.rint(obs_uv + noise)
    cam_fixed = np.zeros(n_cams, np.uint8)
    cam_fixed[:2] = 1
    for c in range(2, n_cams):
        dq = synth.axis_angle_q(rng.normal(size=3), rng.normal(0, pose_noise[1]))
        poses[c] = np.concatenate([synth.quat_mul(poses[c, :4], dq), poses[c, 4:] + rng.normal(0, pose_noise[0], 3)])
        poses[c, :4] /= np.linalg.norm(poses[c, :4])
    pts = pts + rng.normal(0, point_noise, pts.shape)
    return dict(poses=poses, cam_fixed=cam_fixed, cam_intr=cam_intr, intr=synth.DS_INTR.copy(), points=pts,
                obs_cam=obs_cam, obs_lm=obs_lm, obs_uv=obs_uv, cam_model=(0, 0))


def arrays(orc, d):
    return orc.BaArrays(d["poses"], d["cam_fixed"], d["cam_intr"], d["intr"], d["points"], d["obs_cam"], d["obs_lm"],
                        d["obs_uv"], d["cam_model"])


def covisible_fraction(d):
    """Fraction of free-camera pairs that share a landmark."""
    free = np.flatnonzero(d["cam_fixed"] == 0)
    pos = -np.ones(len(d["cam_fixed"]), np.int64)
    pos[free] = np.arange(len(free))
    n_lms = int(d["obs_lm"].max()) + 1
    A = np.zeros((len(free), n_lms), np.float32)
    m = pos[d["obs_cam"]] >= 0
    A[pos[d["obs_cam"][m]], d["obs_lm"][m]] = 1
    cov = (A @ A.T) > 0
    n = len(free)
    return (cov.sum() - n) / float(n * (n - 1))


def assert_dense_when_off(ctx, orc, d):
    """What wide() claims about itself: with the switch off the direct route stores S dense."""
    ctx.set_diagnostic("ba_iterative_schur", 0)
    ctx.bundle_adjust(arrays(orc, d), max_iters=1)
    elems, form, _ = ctx.last_ba_layout()
    n = 6 * int((d["cam_fixed"] == 0).sum())
    assert form == 0 and elems == n * n, (elems, form, n)


def block_jacobi_pcg(S, b, tol, max_it):
    """x, iterations, ||r|| / ||b|| of PCG with the 6 x 6 diagonal blocks of S as preconditioner, recurrence residual
    (the algorithm of visual-slam_amd/csrc/ba_pcg.h, in numpy float64)."""
    n = len(b)
    Minv = np.zeros_like(S)
    for c in range(0, n, 6):
        Minv[c:c + 6, c:c + 6] = np.linalg.inv(S[c:c + 6, c:c + 6])
    x = np.zeros(n)
    r = b.copy()
    z = Minv @ r
    p = z.copy()
    rho = r @ z
    bb = b @ b
    it = 0
    if bb == 0 or max_it == 0:
        return x, 0, (0.0 if bb == 0 else 1.0)
    while True:
        q = S @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = Minv @ r
        rho1 = r @ z
        it += 1
        if r @ r <= tol * tol * bb or it >= max_it:
            return x, it, float(np.sqrt((r @ r) / bb))
        p = z + (rho1 / rho) * p
        rho = rho1
