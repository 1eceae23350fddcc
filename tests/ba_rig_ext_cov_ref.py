"""TEST INFRASTRUCTURE: long-double reference of the covariances of the rig posterior with free stereo extrinsics
(vsl_ba_rig_ext_covariance; include/vslam_hip.h).  Imports ba_rig_ext_ref.py, ba_rig_cov_ref.py and
ba_rig_ref.py unchanged; imports neither the package nor the oracle.

  H         dense, over [free bodies, 6 each | free blocks in ascending k, 6 each | landmarks, 3 each], assembled from
            ba_rig_ext_ref.linearize's Hcc (pose part), W (pose-landmark part) and P (landmark blocks): Huber corrector,
            no scaling, no damping
  Sigma     H^-1 by ba_rig_cov_ref.cholesky_inverse (long-double Cholesky, two triangular solves).  No Schur complement,
            no block formula, nothing from the device.
  camera    A Sigma_pose A^T with the explicit 6 x nt matrix A: Ad(T_b_c^-1) at the body's slot when the body is free, I_6
            at the block's slot when the block is free

A landmark with fewer than two observations is left out of H as in ba_rig_cov_ref (`ExtCovRef.degenerate`).

dense=False (case k_multi_segment only: 1572 unknowns, whose long-double inverse by Python loops takes minutes): the
pose part of H^-1 and the landmark blocks by exact block elimination in long double (ExtCovRef.schur_*), the identity
tests/test_ba_rig_ext_cov_ref_cpu.py checks against the dense inverse on every other case; cond(H) and max|Sigma| of the
tolerance, magnitudes only, from float64 numpy on the same dense H.

Tolerance rule: 64 * cond(H) * 2^-52 * max|Sigma| (`ExtCovRef.tol`).
"""
import numpy as np

import ba_ref
import ba_rig_ext_ref as xr
import ba_rig_ref as rr
from ba_rig_cov_ref import EPS, cholesky_inverse
from pgo_ref import LD, _ld, se3_inv

PIVOT_TOL = 2.0 ** -36


class ExtCovRef:
    def __init__(self, xp, lin=None, dense=True):
        self.xp, rp = xp, xp.rp
        R = xr.linearize(xp) if lin is None else lin
        self.lin = R
        self.nt = nt = xp.nt
        self.nfb = xp.n_free_bodies
        self.body_slot = rp.free_index()
        self.ext_slot = xp.ext_slot()
        L = len(rp.points)
        cnt = np.bincount(rp.obs_lm, minlength=L)
        self.degenerate = [int(l) for l in np.flatnonzero(cnt < 2)]
        kept = [int(l) for l in np.flatnonzero(cnt >= 2)]
        self.lm_pos = {l: k for k, l in enumerate(kept)}
        n = nt + 3 * len(kept)
        H = np.zeros((n, n), LD)
        H[:nt, :nt] = R.Hcc
        for k, l in enumerate(kept):
            H[:nt, nt + 3 * k:nt + 3 * k + 3] = R.W[l]
            H[nt + 3 * k:nt + 3 * k + 3, :nt] = R.W[l].T
            H[nt + 3 * k:nt + 3 * k + 3, nt + 3 * k:nt + 3 * k + 3] = R.P[l]
        self.H = H
        self.dense = dense
        self.cond = float(np.linalg.cond(H.astype(np.float64)))
        if dense:
            self.Sigma_ld = cholesky_inverse(H)
            self.singular = self.Sigma_ld is None
            if not self.singular:
                self.Sigma = self.Sigma_ld.astype(np.float64)
                self.tol = 64.0 * self.cond * EPS * float(np.abs(self.Sigma).max())
        else:
            self.Sigma_ld = self.schur_pose_inverse()          # the pose part only
            self.singular = self.Sigma_ld is None
            if not self.singular:
                self.Sigma = self.Sigma_ld.astype(np.float64)
                self.tol = 64.0 * self.cond * EPS * float(np.abs(np.linalg.inv(H.astype(np.float64))).max())

    # ---- blocks of H^-1
    def _blk(self, i, j, ld=False):
        return (self.Sigma_ld if ld else self.Sigma)[6 * i:6 * i + 6, 6 * j:6 * j + 6]

    def body_block(self, body, ld=False):
        s = self.body_slot[int(body)]
        return self._blk(s, s, ld)

    def ext_block(self, ld=False):
        """the joint block over the free extrinsic slots (they are adjacent, behind the free bodies)"""
        a = 6 * self.nfb
        return (self.Sigma_ld if ld else self.Sigma)[a:self.nt, a:self.nt]

    def cross_block(self, body, j, ld=False):
        """[S^-1] at (body slot, j-th free block)"""
        return self._blk(self.body_slot[int(body)], self.nfb + j, ld)

    def cam_matrix(self, cam):
        """A [6, nt]: xi_c = Ad(T_b_c^-1) delta_b + eps_k to first order"""
        rp = self.xp.rp
        k = rp.cam_intr[int(cam)]
        s, e = self.body_slot[rp.cam_body[int(cam)]], self.ext_slot[k]
        if s < 0 and e < 0:
            raise ValueError("camera %d: its body is fixed and its block is held" % cam)
        A = np.zeros((6, self.nt), LD)
        if s >= 0:
            A[:, 6 * s:6 * s + 6] = rr.adjoint(se3_inv(_ld(rp.T_b_c[k])))
        if e >= 0:
            A[:, 6 * e:6 * e + 6] = np.eye(6, dtype=LD)
        return A

    def cam_block(self, cam, ld=False):
        A = self.cam_matrix(cam)
        M = A @ self.Sigma_ld[:self.nt, :self.nt] @ A.T
        M = (M + M.T) / 2
        return M if ld else M.astype(np.float64)

    def point_block(self, lm, ld=False):
        if not self.dense:
            M = self.schur_point_block(lm, self.Sigma_ld)
            return M if ld else M.astype(np.float64)
        k = self.nt + 3 * self.lm_pos[int(lm)]
        return (self.Sigma_ld if ld else self.Sigma)[k:k + 3, k:k + 3]

    # ---- the Schur form of the contract, in long double
    def reduced(self):
        """S = Hcc - sum_l W_l P_l^-1 W_l^T over the kept landmarks"""
        R = self.lin
        S = np.array(R.Hcc, LD)
        for l in self.lm_pos:
            S -= R.W[l] @ ba_ref._inv3(R.P[l]) @ R.W[l].T
        return S

    def schur_pose_inverse(self):
        return cholesky_inverse(self.reduced())

    def schur_point_block(self, lm, Sinv=None):
        """P^-1 + P^-1 (sum_s sum_s' W_s^T [S^-1]_ss' W_s') P^-1: with W [nt, 3] holding a slot's group sum in the slot's
        rows (zero where the slot has no group) the double sum is W^T S^-1 W"""
        R = self.lin
        Sinv = self.schur_pose_inverse() if Sinv is None else Sinv
        Pi = ba_ref._inv3(R.P[int(lm)])
        W = R.W[int(lm)]
        return Pi + Pi @ W.T @ Sinv @ W @ Pi


def pivot_ratio(S, dtype=np.float64):
    """min_i L_ii^2 / S_ii of the Cholesky factorisation of S in `dtype` (invariant under a diagonal scaling of S): the
    quantity the 2^-36 rule of the covariance chain tests.  None when a pivot is not positive (the factorisation breaks
    down)."""
    S = np.asarray(S, dtype)
    n = len(S)
    Lm = np.zeros((n, n), dtype)
    worst = np.inf
    for j in range(n):
        d = S[j, j] - np.sum(Lm[j, :j] ** 2)
        if not d > 0:
            return None
        worst = min(worst, float(d / S[j, j]))
        Lm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lm[j + 1:, j] = (S[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    return worst


def full_query(xp):
    """(free bodies, every camera with a free body or a free block, every landmark)"""
    rp = xp.rp
    return np.flatnonzero(rp.cam_fixed == 0), np.flatnonzero(xp.cam_free_mask()), np.arange(len(rp.points))


_REF = {}


def reference(name):
    """ExtCovRef(ba_rig_ext_ref.cases()[name]) on the shared linearisation, computed once (read-only)."""
    if name not in _REF:
        _REF[name] = ExtCovRef(xr.cases()[name], xr.reference(name), dense=name != "k_multi_segment")
    return _REF[name]
