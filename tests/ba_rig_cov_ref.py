"""TEST INFRASTRUCTURE: long-double reference of the covariances in rig form (vsl_ba_rig_covariance,
vsl_ba_rig_relative_pose_covariance; include/vslam_hip.h).  Imports ba_rig_ref.py, ba_ref.py and ba_relpose_ref.py
unchanged; imports neither the package nor the oracle.

  Sigma     the inverse of the dense H of ba_rig_ref.linearize(rp) (Lin.H: free bodies in ascending id, 6 each, then the
            landmarks, 3 each), by a long-double Cholesky factorisation and two triangular solves.  No Schur
            complement, no block formula, nothing from the device.
  camera    Ad Sigma_bb Ad^T with Ad = ba_rig_ref.adjoint(se3_inv(T_b_c)), b = cam_body[c]
  relative  ba_relpose_ref's scheme on the BODIES: joint = the body-body blocks of Sigma, meas and J from the long-double
            pose-graph reference, cov = J joint J^T symmetrised, info = its inverse

A landmark with fewer than two observations has a singular block of its own (rank <= 2): H is singular with it, the
device reports it as degenerate, and it is left out of H here (`Ref.degenerate`).  Exactly, such a landmark contributes
nothing to the reduced body system, so the other blocks are those of the problem without it; cond and max|Sigma| of the
tolerance are taken over the system without it.

Tolerance rule of the covariance tests: 64 * cond(H) * 2^-52 * max|Sigma| (`Ref.tol`); twice that where
two device results are compared with each other.
"""
import numpy as np

import ba_ref
import ba_relpose_ref
import ba_rig_ref as rr
from pgo_ref import LD, _ld, se3_inv

EPS = 2.0 ** -52


def cholesky_inverse(H):
    """H^-1 of a symmetric positive definite H in long double (None when a pivot is not positive)."""
    H = np.asarray(H, LD)
    n = len(H)
    Lm = np.zeros((n, n), LD)
    for j in range(n):
        d = H[j, j] - np.sum(Lm[j, :j] ** 2)
        if not d > 0:
            return None
        Lm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lm[j + 1:, j] = (H[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    Y = np.zeros((n, n), LD)                                   # L Y = I
    for j in range(n):
        e = np.zeros(n, LD)
        e[j] = 1
        Y[j] = (e - Lm[j, :j] @ Y[:j]) / Lm[j, j]
    X = np.zeros((n, n), LD)                                   # L^T X = Y
    for j in reversed(range(n)):
        X[j] = (Y[j] - Lm[j + 1:, j] @ X[j + 1:]) / Lm[j, j]
    return (X + X.T) / 2


class Ref:
    def __init__(self, rp, lin=None):
        self.rp = rp
        R = rr.linearize(rp) if lin is None else lin
        self.lin = R
        self.free = [int(b) for b in np.flatnonzero(rp.cam_fixed == 0)]
        self.cam_pos = {b: k for k, b in enumerate(self.free)}             # (the name ba_relpose_ref.RelRef reads)
        L = len(rp.points)
        cnt = np.bincount(rp.obs_lm, minlength=L)
        self.degenerate = [int(l) for l in np.flatnonzero(cnt < 2)]
        kept = [int(l) for l in np.flatnonzero(cnt >= 2)]
        self.lm_pos = {l: k for k, l in enumerate(kept)}
        self.nc = 6 * len(self.free)
        idx = list(range(self.nc)) + [self.nc + 3 * l + j for l in kept for j in range(3)]
        self.H = R.H[np.ix_(idx, idx)]
        self.Sigma_ld = cholesky_inverse(self.H)
        self.singular = self.Sigma_ld is None
        self.cond = float(np.linalg.cond(self.H.astype(np.float64)))
        if not self.singular:
            self.Sigma = self.Sigma_ld.astype(np.float64)
            self.tol = 64.0 * self.cond * EPS * float(np.abs(self.Sigma).max())

    def body_block(self, body, ld=False):
        k = 6 * self.cam_pos[int(body)]
        return (self.Sigma_ld if ld else self.Sigma)[k:k + 6, k:k + 6]

    def cam_adjoint(self, cam):
        return rr.adjoint(se3_inv(_ld(self.rp.T_b_c[self.rp.cam_intr[int(cam)]])))

    def cam_block(self, cam, ld=False):
        Ad = self.cam_adjoint(cam)
        M = Ad @ self.body_block(self.rp.cam_body[int(cam)], ld=True) @ Ad.T
        M = (M + M.T) / 2
        return M if ld else M.astype(np.float64)

    def point_block(self, lm, ld=False):
        k = self.nc + 3 * self.lm_pos[int(lm)]
        return (self.Sigma_ld if ld else self.Sigma)[k:k + 3, k:k + 3]

    def schur_point_block(self, lm):
        """The block formula of the contract in long double: P^-1 + P^-1 W^T [S^-1] W P^-1, W = H[bodies, landmark] (a
        body's column block of W is its group's sum; zero where the body has no group)."""
        nc = self.nc
        k = nc + 3 * self.lm_pos[int(lm)]
        Hll_inv = np.zeros((len(self.H) - nc,) * 2, LD)
        for j in range(0, len(self.H) - nc, 3):
            Hll_inv[j:j + 3, j:j + 3] = ba_ref._inv3(self.H[nc + j:nc + j + 3, nc + j:nc + j + 3])
        Hcl = self.H[:nc, nc:]
        Sinv = cholesky_inverse(self.H[:nc, :nc] - Hcl @ Hll_inv @ Hcl.T)
        Pi = ba_ref._inv3(self.H[k:k + 3, k:k + 3])
        W = self.H[:nc, k:k + 3]
        return Pi + Pi @ W.T @ Sinv @ W @ Pi

    def relpose(self):
        """ba_relpose_ref.RelRef on the bodies (pair(a, b): joint, meas, cov, info and their tolerances)."""
        return ba_relpose_ref.RelRef(self, self.rp.poses, self.rp.cam_fixed)


def _build_extra():
    T = {}
    T["j_identity_is_free"] = rr.rig_scene(4, 2, 9, 509, cams_of_body=[(0,)] * 4, identity=True)
    rp = rr.rig_scene(3, 1, 9, 510)
    T["k_one_observation"] = rr._drop(rp, ~((rp.obs_lm == 5) & (rp.obs_camera != 0)))
    T["m_sparse_groups"] = rr.rig_scene(6, 1, 12, 511, window=2)
    for name, rp in T.items():
        rp.name = name
    return T


_CASES = None
_REF = {}


def cases():
    """name -> RigProblem: ba_rig_ref.cases() (a-i) plus j, k, m; built once, read-only."""
    global _CASES
    if _CASES is None:
        _CASES = dict(rr.cases())
        _CASES.update(_build_extra())
    return _CASES


def reference(name):
    """Ref(cases()[name]), computed once and shared (read-only)."""
    if name not in _REF:
        lin = rr.reference(name) if name in rr.cases() else None
        _REF[name] = Ref(cases()[name], lin)
    return _REF[name]
