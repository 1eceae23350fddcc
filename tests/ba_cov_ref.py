"""TEST INFRASTRUCTURE: numpy reference of vsl_ba_covariance (include/vslam_hip.h), in the style of orb_ref.py.

Per observation r, J_pose, J_point come from the oracle (pyoracle.ba_residual_jacobian); the Huber corrector is applied
here as vsl_ba_linearize documents it (residual and Jacobian scaled by sqrt(rho'), rho' = 1 for |r|^2 <= a^2 and
a / |r| beyond); the full dense H = J^T J over [free cameras (6 each, ascending camera id) | landmarks (3 each)] is
assembled and inverted with numpy.linalg.inv.  No Schur complement, no block formula, nothing from the device.

A landmark with fewer than two observations has a singular block of its own (rank <= 2): H is singular with it, the
device reports it as degenerate, and it is left out of H here (`Ref.degenerate`).  Exactly, such a landmark contributes
nothing to the reduced camera system (F^T (I - E E^+) F = 0 for a 2 x 3 E of full row rank), so the other blocks are
those of the problem without it.

Tolerance rule of the covariance tests: 64 * cond(H) * 2^-52 * max|Sigma| (`Ref.tol`).
"""
import numpy as np

EPS = 2.0 ** -52


class Ref:
    def __init__(self, orc, arr, use_huber=True, huber=1.0):
        self.free = [int(c) for c in np.flatnonzero(arr.cam_fixed == 0)]
        cam_pos = {c: k for k, c in enumerate(self.free)}
        n_lms = len(arr.points)
        cnt = np.bincount(arr.obs_lm, minlength=n_lms)
        self.degenerate = [int(l) for l in np.flatnonzero(cnt < 2)]
        kept = [int(l) for l in np.flatnonzero(cnt >= 2)]
        lm_pos = {l: k for k, l in enumerate(kept)}
        self.nc = 6 * len(self.free)
        N = self.nc + 3 * len(kept)
        J = np.zeros((2 * len(arr.obs_cam), N))
        for i, (c, l) in enumerate(zip(arr.obs_cam, arr.obs_lm)):
            c, l = int(c), int(l)
            if l not in lm_pos:
                continue
            k = int(arr.cam_intr[c])
            r, Jp, Jl = orc.ba_residual_jacobian(arr.cam_model[k], arr.poses[c], arr.points[l], arr.intr[k], arr.obs_uv[i])
            s = float(r @ r)
            sr = np.sqrt(huber / np.sqrt(s)) if (use_huber and s > huber * huber) else 1.0
            if c in cam_pos:
                J[2 * i:2 * i + 2, 6 * cam_pos[c]:6 * cam_pos[c] + 6] = sr * Jp
            J[2 * i:2 * i + 2, self.nc + 3 * lm_pos[l]:self.nc + 3 * lm_pos[l] + 3] = sr * Jl
        self.H = J.T @ J
        self.cond = float(np.linalg.cond(self.H))
        self.Sigma = np.linalg.inv(self.H)
        self.cam_pos, self.lm_pos = cam_pos, lm_pos
        self.tol = 64.0 * self.cond * EPS * float(np.abs(self.Sigma).max())

    def pose_block(self, cam):
        k = 6 * self.cam_pos[int(cam)]
        return self.Sigma[k:k + 6, k:k + 6]

    def point_block(self, lm):
        k = self.nc + 3 * self.lm_pos[int(lm)]
        return self.Sigma[k:k + 3, k:k + 3]

    def schur(self):
        """S = H_cc - H_cl H_ll^-1 H_lc (H_ll is block diagonal; inverted as a whole here)."""
        nc = self.nc
        Hcl = self.H[:nc, nc:]
        return self.H[:nc, :nc] - Hcl @ np.linalg.inv(self.H[nc:, nc:]) @ Hcl.T

    def landmark_own_inverse(self, lm):
        k = self.nc + 3 * self.lm_pos[int(lm)]
        return np.linalg.inv(self.H[k:k + 3, k:k + 3])


INTR = {0: [350.0, 348.0, 365.0, 249.0, -0.24, 0.57, 0, 0],
        1: [350.0, 348.0, 365.0, 249.0, 0, 0, 0, 0],
        2: [350.0, 348.0, 365.0, 249.0, 0.6, 1.1, 0, 0],
        3: [350.0, 348.0, 365.0, 249.0, 0.01, -0.004, 0.002, -0.0005]}


def problem(synth, seed, n_free, n_lms, model=0, outlier_frac=0.05):
    """A synth.ba_problem cut down to its first n_lms landmarks, with as many leading cameras fixed as leave n_free free
    ones (at least the first keyframe's two).  Returns the dict of arrays."""
    n_kf = (n_free + 2 + 1) // 2
    d = synth.ba_problem(seed, n_kf=n_kf, n_lms=12 * n_lms, outlier_frac=outlier_frac)
    assert len(d["points"]) >= n_lms
    sel = d["obs_lm"] < n_lms
    d["points"] = d["points"][:n_lms]
    for k in ("obs_cam", "obs_lm", "obs_uv"):
        d[k] = d[k][sel]
    n_cams = len(d["poses"])
    d["cam_fixed"] = np.zeros(n_cams, np.uint8)
    d["cam_fixed"][:n_cams - n_free] = 1
    if model:
        d["intr"] = np.array([INTR[model], INTR[model]])
        d["cam_model"] = (model, model)
    return d


def arrays(mod, d):
    """mod: pyoracle or the package (both have BaArrays)."""
    return mod.BaArrays(d["poses"], d["cam_fixed"], d["cam_intr"], d["intr"], d["points"], d["obs_cam"], d["obs_lm"],
                        d["obs_uv"], d["cam_model"])


def drop_observations(d, mask):
    """The problem without the observations where mask is True."""
    e = dict(d)
    for k in ("obs_cam", "obs_lm", "obs_uv"):
        e[k] = d[k][~mask]
    return e
