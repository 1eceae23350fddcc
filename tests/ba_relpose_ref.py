"""TEST INFRASTRUCTURE: reference of vsl_ba_relative_pose_covariance, combined from two references that exist:

  joint   the pose-pose blocks of ba_cov_ref.Ref.Sigma (numpy.linalg.inv of the full dense H from the oracle's Jacobians);
          rows and columns of a fixed camera are zero
  meas, J the long-double pose-graph reference (pgo_ref.residual_jacobian, the function behind
          pgo_joint_ref.edge_terms, evaluated for all pairs of a problem in one batch): log(T_a^-1 T_b) and the
          Jacobians of the functor's residual with respect to the right perturbations of the two poses, at a zero
          measurement (they do not depend on it); a fixed camera's half of J is zero
  cov     Sigma_r = J joint J^T, symmetrised;  info = numpy.linalg.inv(Sigma_r)

Tolerances (derived; Ref.tol = 64 cond(H) 2^-52 max|Sigma| is the rule of the covariance tests):
  joint   Ref.tol
  cov     144 max|J|^2 Ref.tol: each entry is a sum of 144 products J Sigma J
  info    36 max|Omega_ref|^2 tol_cov + 64 cond(Sigma_r,ref) 2^-52 max|Omega_ref|: the first-order perturbation of an
          inverse (dOmega = -Omega dSigma Omega, 36 products per entry) plus the inversion's own rounding
  meas    pgo_ref.GPU_TOL x max|log(T_a^-1 T_b)|.  GPU_TOL is the relative tolerance the pose-graph GPU tests allow the
          functor's linearisation (residual, Jacobians, H, g) against pgo_ref (test_pgo_edges_gpu.py; test_pgo_gpu.py
          itself compares its edge measurements with atol 1e-6, which is looser); taken on the logarithm it is the
          bound test_pgo_edge_consistency_gpu.py puts on the same device code's residual
"""
import numpy as np

import pgo_ref as pg

EPS = 2.0 ** -52


class _Graph:
    """The part of a pgo_joint_ref case that its edge terms read: the poses."""

    def __init__(self, poses):
        self.poses = poses


class _Case:
    def __init__(self, poses):
        self.g = _Graph(poses)


class Pair:
    """joint [12, 12], meas [6], J [6, 12], cov, info [6, 6] (float64) and tol_joint, tol_cov, tol_info, tol_meas."""


class RelRef:
    def __init__(self, ref, poses, cam_fixed):
        """ref: ba_cov_ref.Ref of the problem; poses [n_cams, 7]; cam_fixed [n_cams]."""
        self.ref = ref
        self.case = _Case(np.asarray(poses, np.float64))
        self.fixed = np.asarray(cam_fixed).astype(bool)
        self._pairs = {}

    def _slice(self, cam):
        return None if self.fixed[cam] else slice(6 * self.ref.cam_pos[int(cam)], 6 * self.ref.cam_pos[int(cam)] + 6)

    def joint(self, a, b):
        out = np.zeros((12, 12))
        for x, cx in enumerate((a, b)):
            for y, cy in enumerate((a, b)):
                ix, iy = self._slice(cx), self._slice(cy)
                if ix is not None and iy is not None:
                    out[6 * x:6 * x + 6, 6 * y:6 * y + 6] = self.ref.Sigma[ix, iy]
        return out

    def jacobians(self, pairs):
        """(meas [n, 6], J [n, 6, 12]) in long double, one batched evaluation of pgo_ref.residual_jacobian (what
        pgo_joint_ref.edge_terms evaluates pair by pair); a fixed camera's half of J zeroed."""
        pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
        P = pg._ld(self.case.g.poses)
        r, Ja, Jb, _ = pg.residual_jacobian(P[pairs[:, 0]], P[pairs[:, 1]], np.zeros((len(pairs), 6)))
        Ja[self.fixed[pairs[:, 0]]] = 0
        Jb[self.fixed[pairs[:, 1]]] = 0
        return r, np.concatenate([Ja, Jb], axis=2)

    def prepare(self, pairs):
        """Fills the cache for the pairs not seen yet."""
        todo = sorted({(int(a), int(b)) for a, b in pairs} - set(self._pairs))
        if not todo:
            return
        meas, J = self.jacobians(todo)
        for k, (a, b) in enumerate(todo):
            p = Pair()
            p.joint = self.joint(a, b)
            p.meas, p.J = np.asarray(meas[k], np.float64), np.asarray(J[k], np.float64)
            M = np.asarray(J[k] @ pg._ld(p.joint) @ J[k].T, np.float64)
            p.cov = (M + M.T) / 2
            p.info = np.linalg.inv(p.cov)
            p.info = (p.info + p.info.T) / 2
            p.tol_joint = self.ref.tol
            p.tol_cov = 144.0 * float(np.abs(p.J).max()) ** 2 * self.ref.tol
            om = float(np.abs(p.info).max())
            p.tol_info = 36.0 * om * om * p.tol_cov + 64.0 * float(np.linalg.cond(p.cov)) * EPS * om
            p.tol_meas = pg.GPU_TOL * float(np.abs(p.meas).max())
            self._pairs[(a, b)] = p

    def pair(self, a, b):
        self.prepare([(a, b)])
        return self._pairs[(int(a), int(b))]


def brute_force_jacobian(Ta, Tb, h=3e-4):
    """The brute-force route: perturb both poses on the right by +-h and +-h / 2 along every tangent direction,
    difference the residual (long double) and cancel the h^2 term.  The steps are not those of pgo_ref.residual_jacobian
    (1e-4, 5e-5, 2.5e-5), so the two evaluations share no sample.  Ta, Tb: [..., 7]; returns [..., 6, 12]."""
    Ta, Tb = pg._ld(Ta), pg._ld(Tb)
    return (4 * pg._central(Ta, Tb, h / 2) - pg._central(Ta, Tb, h)) / 3


def all_pairs(cam_fixed):
    """Every ordered-once pair (a < b) of cameras that are not both fixed."""
    fixed = np.asarray(cam_fixed).astype(bool)
    n = len(fixed)
    return [(a, b) for a in range(n) for b in range(a + 1, n) if not (fixed[a] and fixed[b])]
