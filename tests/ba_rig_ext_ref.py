"""TEST INFRASTRUCTURE: long-double numpy reference of the rig bundle adjustment with the stereo extrinsics as unknowns
(ba_rig.hip "EXTRINSICS", include/vslam_hip.h vsl_bundle_adjust_rig_ext).  Imports ba_ref.py and ba_rig_ref.py unchanged;
imports neither the package nor the oracle.

  unknowns    [free bodies in ascending id, 6 each | free extrinsic blocks in ascending k, 6 each | landmarks, 3 each]
  Jacobians   per observation J = [F_b | F_x | E]: F_b, E and r from ba_rig_ref.RigProblem.blocks (finite differences along
              T_w_b exp(d) T_b_c), F_x = ba_ref's own camera Jacobian (RigProblem.last_F_c: finite differences along
              T_w_c exp(d), which IS T_w_b T_b_c exp(d))
  assembly, scaling, damping, reduction, magnitudes A_S / A_g, cond_S, the LM step: the scheme of ba_ref.linearize /
              ba_ref.lm_step, with an observation that touches up to TWO pose slots (so the pose part of H has off-diagonal
              blocks and A_S their magnitudes)
  expanded()  the free problem P of the same cameras, camera c free iff its body is free or ext_free[cam_intr[c]];
  fold_matrix() the A with S = A^T S_P A, g = A^T g_P: block (c, body of c) = Ad(T_b_c^-1) if that body is free,
              block (c, block of c) = I_6 if that block is free.

ORACLE_FOLD_VS_REF_K: measured by tests/test_ba_rig_ext_ref_cpu.py (x86-64, 80-bit long double) as
ba_rig_ref.ORACLE_FOLD_VS_REF_K was: the CPU oracle's ba_linearize of P, folded with A in float64 numpy, against this
reference, entrywise in units of 2^-52 A_S / 2^-52 A_g.  The device is allowed K_EXT_GPU = min(8 x that, 64).
"""
import numpy as np

import ba_ref
import ba_rig_ref
from ba_rig_ref import adjoint
from pgo_ref import LD, _ld, se3_exp, se3_inv, se3_mul

U = ba_ref.U

# measured 2.93 (S of case j_22_free; its g 1.11; the multi-segment case 0.40 / 0.11; every small case below 0.9),
# recorded rounded up
ORACLE_FOLD_VS_REF_K = 3.0
K_EXT_GPU = min(8.0 * ORACLE_FOLD_VS_REF_K, 64.0)


class ExtProblem:
    """A RigProblem (bodies, points, extrinsics rp.T_b_c: the linearisation point) plus which extrinsic blocks are free."""

    def __init__(self, rp, ext_free, name=""):
        self.rp, self.ext_free, self.name = rp, tuple(int(bool(f)) for f in ext_free), name or rp.name
        self._blocks = None

    @property
    def n_free_bodies(self):
        return self.rp.n_free

    @property
    def n_ext(self):
        return sum(self.ext_free)

    @property
    def nt(self):
        return 6 * (self.n_free_bodies + self.n_ext)

    def ext_slot(self):
        """slot of block k (behind the free bodies), -1 when held"""
        out, s = [], self.n_free_bodies
        for k in (0, 1):
            out.append(s if self.ext_free[k] else -1)
            s += self.ext_free[k]
        return np.array(out)

    def obs_slots(self):
        """(body slot, extrinsic slot) per observation, -1 where the observation has no such column"""
        rp = self.rp
        return rp.free_index()[rp.obs_cam], self.ext_slot()[rp.cam_intr[rp.obs_camera]]

    def blocks(self):
        """raw r [O, 2], F_b [O, 2, 6], F_x [O, 2, 6], E [O, 2, 3], finite-difference disagreement [O]; computed once"""
        if self._blocks is None:
            r, Fb, E, dis = self.rp.blocks()
            self._blocks = (r, Fb, self.rp.last_F_c, E, dis)
        return self._blocks

    def with_state(self, bodies=None, points=None, T_b_c=None):
        rp = self.rp
        new = ba_rig_ref.RigProblem(rp.poses if bodies is None else bodies, rp.cam_fixed, rp.cam_body, rp.cam_intr,
                                    rp.T_b_c if T_b_c is None else T_b_c, rp.intr, rp.points if points is None else points,
                                    rp.obs_camera, rp.obs_lm, rp.obs_uv, rp.cam_model, rp.name, use_huber=rp.use_huber, huber=rp.huber)
        return ExtProblem(new, self.ext_free, self.name)

    # ---- the free problem P of the same cameras and the fold
    def cam_free_mask(self):
        rp = self.rp
        return (rp.cam_fixed[rp.cam_body] == 0) | (np.array(self.ext_free)[rp.cam_intr] != 0)

    def expanded(self):
        rp = self.rp
        return ba_ref.Problem(rp.cameras().astype(np.float64), (~self.cam_free_mask()).astype(np.uint8), rp.cam_intr, rp.intr, rp.points,
                              rp.obs_camera, rp.obs_lm, rp.obs_uv, rp.cam_model, self.name + "/expanded", use_huber=rp.use_huber,
                              huber=rp.huber)

    def fold_matrix(self):
        """A [6 free cameras of P, nt] (long double)."""
        rp = self.rp
        slot, es = rp.free_index(), self.ext_slot()
        cams = np.flatnonzero(self.cam_free_mask())
        A = np.zeros((6 * len(cams), self.nt), LD)
        for fc, c in enumerate(cams):
            s, e = slot[rp.cam_body[c]], es[rp.cam_intr[c]]
            if s >= 0:
                A[6 * fc:6 * fc + 6, 6 * s:6 * s + 6] = adjoint(se3_inv(_ld(rp.T_b_c[rp.cam_intr[c]])))
            if e >= 0:
                A[6 * fc:6 * fc + 6, 6 * e:6 * e + 6] = np.eye(6, dtype=LD)
        return A


def linearize(xp, inv_radius=None):
    """The fields of ba_ref.linearize (a ba_ref.Lin) over [free bodies | free blocks | landmarks]: r, F (= F_b), Fx, E (raw),
    outlier, fd_disagreement, cost, D [nt + 3 L], damp, S, g, A_S, A_g, kappa, and for a scaled system dc, dl, cond_S.
    inv_radius None: the plain system; a number: columns scaled by D, the scaled diagonal damped."""
    rp = xp.rp
    out = ba_ref.Lin()
    L, O, nt = len(rp.points), len(rp.obs_lm), xp.nt
    out.r, out.F, out.Fx, out.E, dis = xp.blocks()
    out.fd_disagreement = float(dis.max())
    r, Fb, E, cost, out.outlier = ba_ref.huber_correct(out.r, out.F, out.E, rp.use_huber, rp.huber)
    Fx = ba_ref.huber_correct(out.r, out.Fx, out.E, rp.use_huber, rp.huber)[1]
    out.cost = float(np.sum(cost))
    sb, se = xp.obs_slots()
    # the pose row of every observation over all nt columns (at most two non-zero blocks)
    Hcc, bc = np.zeros((nt, nt), LD), np.zeros(nt, LD)
    P, W, bl = np.zeros((L, 3, 3), LD), np.zeros((L, nt, 3), LD), np.zeros((L, 3), LD)
    rows = []
    for i in range(O):
        cols, J = [], []
        if sb[i] >= 0:
            cols.append(np.arange(6 * sb[i], 6 * sb[i] + 6))
            J.append(Fb[i])
        if se[i] >= 0:
            cols.append(np.arange(6 * se[i], 6 * se[i] + 6))
            J.append(Fx[i])
        l = rp.obs_lm[i]
        P[l] += E[i].T @ E[i]
        bl[l] += E[i].T @ r[i]
        if cols:
            c, Jp = np.concatenate(cols), np.concatenate(J, axis=1)
            Hcc[np.ix_(c, c)] += Jp.T @ Jp
            bc[c] += Jp.T @ r[i]
            W[l][c] += Jp.T @ E[i]
            rows.append((c, Jp, i))
    out.Hcc, out.bc, out.P, out.W, out.bl = Hcc, bc, P, W, bl
    Dc, Dl = np.ones(nt, LD), np.ones((L, 3), LD)
    dampc, dampl = np.zeros(nt, LD), np.zeros((L, 3), LD)
    diag_l = np.stack([np.diag(P[l]) for l in range(L)])
    if inv_radius is not None:
        Dc, Dl = 1 / (1 + np.sqrt(np.diag(Hcc))), 1 / (1 + np.sqrt(diag_l))
        dampc = np.clip(Dc * np.diag(Hcc) * Dc, LD(1e-6), LD(1e32)) * LD(inv_radius)
        dampl = np.clip(Dl * diag_l * Dl, LD(1e-6), LD(1e32)) * LD(inv_radius)
    out.D, out.damp = np.concatenate([Dc, Dl.ravel()]), np.concatenate([dampc, dampl.ravel()])
    S = Dc[:, None] * Hcc * Dc[None, :] + np.diag(dampc)
    g = Dc * bc
    A_S, A_g = np.zeros((nt, nt), LD), np.zeros(nt, LD)
    for c, Jp, i in rows:
        Ja = np.abs(Jp) * Dc[c][None, :]
        A_S[np.ix_(c, c)] += Ja.T @ Ja
        A_g[c] += Ja.T @ np.abs(r[i])
    A_S += np.diag(dampc)
    out.kappa = np.zeros(L)
    seen = np.bincount(rp.obs_lm, minlength=L)
    Pinv, Ws, bls = {}, {}, {}
    for l in range(L):
        Pl = Dl[l][:, None] * P[l] * Dl[l][None, :] + np.diag(dampl[l])
        Wl, bll = Dc[:, None] * W[l] * Dl[l][None, :], Dl[l] * bl[l]
        if not seen[l] and not np.any(Pl):
            continue
        Pi = Pinv[l] = ba_ref._inv3(Pl)
        Ws[l], bls[l] = Wl, bll
        if not np.any(Wl):
            continue
        out.kappa[l] = np.linalg.cond(P[l].astype(np.float64))       # of the PLAIN block, whatever the variables
        S -= Wl @ Pi @ Wl.T
        g -= Wl @ Pi @ bll
        A_S += LD(out.kappa[l]) * (np.abs(Wl) @ np.abs(Pi) @ np.abs(Wl).T)
        A_g += LD(out.kappa[l]) * (np.abs(Wl) @ np.abs(Pi) @ np.abs(bll))
    out.S, out.g, out.A_S, out.A_g = S, g, A_S, A_g
    out.dc = out.dl = None
    if inv_radius is not None:
        out.cond_S = float(np.linalg.cond(S.astype(np.float64)))
        x = ba_ref._cholesky_solve(S, g)
        out.dc = None if x is None else -x
        out.dl = np.zeros((L, 3), LD)
        for l, Pi in Pinv.items() if x is not None else ():
            out.dl[l] = -Pi @ (bls[l] + Ws[l].T @ out.dc)
    return out


def apply_step(xp, step, step_l):
    """(bodies, T_b_c, points) in long double after T * exp(step) on the free bodies / blocks and p + step_l."""
    rp = xp.rp
    nfb = xp.n_free_bodies
    step = _ld(step).reshape(-1, 6)
    bodies, T = _ld(rp.poses).copy(), _ld(rp.T_b_c).copy()
    free = np.flatnonzero(rp.cam_fixed == 0)
    if len(free):
        new = se3_mul(bodies[free], se3_exp(step[:nfb]))
        new[:, :4] /= np.sqrt(np.sum(new[:, :4] ** 2, axis=1, keepdims=True))
        bodies[free] = new
    for k, s in enumerate(xp.ext_slot()):
        if s >= 0:
            new = se3_mul(T[k], se3_exp(step[s]))
            new[:4] /= np.sqrt(np.sum(new[:4] ** 2))
            T[k] = new
    return bodies, T, _ld(rp.points) + _ld(step_l)


def lm_step(xp, inv_radius=1e-4):
    """One LM step: (candidate bodies, candidate T_b_c, candidate points, pose step [slots, 6], landmark step, Lin)."""
    R = linearize(xp, inv_radius)
    nt = xp.nt
    step = (R.D[:nt] * R.dc).reshape(-1, 6)
    step_l = R.D[nt:].reshape(-1, 3) * R.dl
    return apply_step(xp, step, step_l) + (step, step_l, R)


def gauge_direction(xp):
    """One fixed body, one free block k: the direction of the scaling about the centre p0 of the fixed body's HELD-block
    camera, in the unknowns [free bodies | block k | landmarks] (first order in s - 1):
      landmarks        dX = X - p0
      a free body b    its held-block camera centre c_b moves by c_b - p0 and nothing rotates: T_w_b exp((u, 0)) moves the
                       held camera centre by R_b u, so u = R_b^T (c_b - p0)
      block k          the free camera's centre in the body frame t_k -> t_h + s (t_k - t_h): T_b_c exp((u, 0)) moves it by
                       R_k u, so u = R_k^T (t_k - t_h)
    Every residual is unchanged along it."""
    rp = xp.rp
    assert xp.n_ext == 1 and int((rp.cam_fixed != 0).sum()) == 1
    k = int(np.flatnonzero(xp.ext_free)[0])
    h = 1 - k
    T = _ld(rp.T_b_c)
    bodies = _ld(rp.poses)
    fixed = int(np.flatnonzero(rp.cam_fixed != 0)[0])
    centre = lambda b: se3_mul(bodies[b], T[h])[4:]
    p0 = centre(fixed)
    v = np.zeros(xp.nt + 3 * len(rp.points), LD)
    slot = rp.free_index()
    for b in range(len(bodies)):
        if slot[b] >= 0:
            v[6 * slot[b]:6 * slot[b] + 3] = ba_rig_ref._rot(bodies[b, :4]).T @ (centre(b) - p0)
    e = xp.ext_slot()[k]
    v[6 * e:6 * e + 3] = ba_rig_ref._rot(T[k, :4]).T @ (T[k, 4:] - T[h, 4:])
    v[xp.nt:] = (_ld(rp.points) - p0).ravel()
    return v


def jacobian_times(xp, v):
    """J v per observation [O, 2] with the raw (uncorrected) blocks."""
    rp = xp.rp
    r, Fb, Fx, E, _ = xp.blocks()
    sb, se = xp.obs_slots()
    out = np.zeros((len(rp.obs_lm), 2), LD)
    for i in range(len(rp.obs_lm)):
        l = xp.nt + 3 * rp.obs_lm[i]
        out[i] = E[i] @ v[l:l + 3]
        if sb[i] >= 0:
            out[i] += Fb[i] @ v[6 * sb[i]:6 * sb[i] + 6]
        if se[i] >= 0:
            out[i] += Fx[i] @ v[6 * se[i]:6 * se[i] + 6]
    return out


# ----------------------------------------------------------------------------------------------------------- fixtures
def base_scene(seed=600, **kw):
    """4 bodies x 2 cameras, bodies 0 and 1 fixed, 9 landmarks; a few observations missing so that the blocks are not
    uniform (cameras 4, 5 are body 2, cameras 6, 7 body 3)."""
    rp = ba_rig_ref.rig_scene(4, 2, 9, seed, **kw)
    cam, lm = rp.obs_camera, rp.obs_lm
    return ba_rig_ref._drop(rp, ~(((cam == 5) & (lm == 1)) | ((cam == 6) & (lm == 2)) | ((cam == 1) & (lm == 6)) | ((cam == 4) & (lm == 7))))


def _build_cases():
    T = {}
    T["a_base"] = ExtProblem(base_scene(), (0, 1))
    # both blocks free: THREE fixed bodies.  With two, a rigid motion G that commutes with their relative pose (the screw
    # about its axis, 2 dof) maps T_b_c[k] -> T_b^-1 G T_b T_b_c[k] for both fixed bodies alike and moves the landmarks
    # and free bodies along: the undamped system is singular by construction (measured cond 6e17), whatever the seed
    T["b_both_free"] = ExtProblem(ba_rig_ref.rig_scene(5, 3, 9, 601), (1, 1))
    T["c_block0_free"] = ExtProblem(base_scene(602), (1, 0))
    rp = ba_rig_ref.rig_scene(4, 2, 9, 603)                      # landmark 3: fixed bodies only -> it reaches only the border
    T["d_fixed_bodies_only"] = ExtProblem(ba_rig_ref._drop(rp, ~((rp.obs_lm == 3) & (rp.cam_body[rp.obs_camera] >= 2))), (0, 1))
    rp = ba_rig_ref.rig_scene(4, 2, 9, 604)                      # landmark 4: block-0 cameras only -> no extrinsic group
    T["e_block0_cameras_only"] = ExtProblem(ba_rig_ref._drop(rp, ~((rp.obs_lm == 4) & (rp.cam_intr[rp.obs_camera] == 1))), (0, 1))
    T["f_single_camera_body"] = ExtProblem(ba_rig_ref.rig_scene(4, 2, 9, 605, cams_of_body=[(0, 1), (0, 1), (0, 1), (1,)]), (0, 1))
    T["g_models"] = ExtProblem(ba_rig_ref.rig_scene(4, 2, 9, 606, models=(0, 3)), (0, 1))
    rp = ba_rig_ref.rig_scene(4, 2, 9, 607, use_huber=True, huber=1.0)
    i0 = int(np.flatnonzero((rp.obs_camera == 4) & (rp.obs_lm == 1))[0])
    i1 = int(np.flatnonzero((rp.obs_camera == 7) & (rp.obs_lm == 5))[0])
    rp.obs_uv[i0] += [35.0, -22.0]
    rp.obs_uv[i1] += [-28.0, 41.0]
    rp.outliers = (i0, i1)
    T["h_huber_outliers"] = ExtProblem(rp, (0, 1))
    T["i_no_free_body"] = ExtProblem(ba_rig_ref.rig_scene(4, 4, 9, 608), (0, 1))          # nt = 6
    # 22 free bodies + 1 block = 138 unknowns, past the 128 of the small dense solver
    T["j_22_free"] = ExtProblem(ba_rig_ref.rig_scene(24, 2, 24, 609, window=3), (0, 1))
    # 2 fixed + 1 free body x 2 cameras x 520 landmarks, everything seen by everything: 1040 observations in the free body's
    # list, 1560 in the extrinsic slot's (4 segments of the block sums), 520 groups per slot (2 segments of the gather)
    T["k_multi_segment"] = ExtProblem(ba_rig_ref.rig_scene(3, 2, 520, 610), (0, 1))
    T["l_gauge_one_fixed"] = ExtProblem(ba_rig_ref.rig_scene(3, 1, 9, 611), (0, 1))
    for name, xp in T.items():
        xp.name = xp.rp.name = name
    return T


GAUGE_CASES = ("l_gauge_one_fixed",)
_CASES = None
_LIN = {}


def cases():
    """name -> ExtProblem, built once (treat as read-only)."""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


def reference(name, inv_radius=None):
    """linearize(cases()[name], inv_radius), computed once and shared (read-only)."""
    key = (name, inv_radius)
    if key not in _LIN:
        _LIN[key] = linearize(cases()[name], inv_radius)
    return _LIN[key]


def jac_tol(name):
    """Jacobian-block tolerance of a case, relative to the block's largest entry: ba_ref's rule."""
    return min(max(8.0 * ba_ref.ORACLE_VS_REF_JAC, 10.0 * reference(name).fd_disagreement), 1e-9)


def perturbed_extrinsic(T_b_c, k=1, mm=5.0, deg=0.3):
    """T_b_c with block k moved by exp((mm * u, deg * w)), u and w fixed unit vectors."""
    u = np.array([0.6, -0.48, 0.64]) * mm * 1e-3
    w = np.array([-0.36, 0.48, 0.8]) * np.deg2rad(deg)
    T = np.array(T_b_c, np.float64).reshape(2, 7).copy()
    new = se3_mul(_ld(T[k]), se3_exp(_ld(np.concatenate([u, w]))))
    new[:4] /= np.sqrt(np.sum(new[:4] ** 2))
    T[k] = new.astype(np.float64)
    return T
