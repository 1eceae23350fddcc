"""TEST INFRASTRUCTURE: long-double numpy reference of the RIG-constrained bundle adjustment (ba_rig.hip): one body pose
per stereo frame, T_w_c = T_w_b * T_b_c[cam_intr], unknowns [free bodies in ascending id, 6 each | landmarks].  Imports
ba_ref.py and pgo_ref.py unchanged; imports neither the package nor the oracle.

  cameras     T_w_c composed in long double from the float64 bodies and extrinsics (never rounded to double)
  Jacobians   F_b = d r / d (upsilon, omega) along T_w_b * exp(d) * T_b_c by ba_ref's scheme -- central differences in
              long double acting on the camera-frame point, Richardson extrapolated (4 D(h/2) - D(h)) / 3, ba_ref's step
              and its projection -- NOT by the adjoint formula: the body perturbation moves the body-frame point
              p_b = T_b_c p_c to exp(d)^-1 p_b, which goes back through T_b_c^-1.  E and r are ba_ref's own.
  assembly, reduction with the entrywise magnitudes A_S / A_g, the scaled and damped form, the LM step:
              ba_ref.linearize / ba_ref.lm_step themselves, run on a view of the problem whose "cameras" are the bodies
              (RigProblem quacks like ba_ref.Problem).  Two observations of one landmark from the two cameras of a body
              simply add into the same body block.
  expanded()  the FREE problem of the same cameras (ba_ref.Problem, camera poses rounded to double,
              cam_fixed = body_fixed[cam_body]) and fold_matrix() the A with S_rig = A^T S_free A, g_rig = A^T g_free
              (block (camera, its body) = Ad(T_b_c^-1) in the (upsilon, omega) order).

ORACLE_FOLD_VS_REF_K: measured by tests/test_ba_rig_ref_cpu.py (x86-64, 80-bit long double): the CPU oracle's
ba_linearize of the expanded problem, folded with A in float64 numpy, against this reference, entrywise in units of
2^-52 A (A = the reference's magnitudes A_S, A_g).  The device is allowed K_RIG_GPU = min(8 x that, 64), the rule of
ba_ref.py.  Measured figures: see the constant below.
"""
import numpy as np

import ba_ref
from pgo_ref import LD, _ld, q_conj, q_rot, se3_exp, se3_inv, se3_mul

# measured 2.63 (S of case h_23_free; its g 1.50; every 3-body case below 0.9), recorded rounded up
ORACLE_FOLD_VS_REF_K = 3.0
K_RIG_GPU = min(8.0 * ORACLE_FOLD_VS_REF_K, 64.0)


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], LD)


def _rot(q):
    return np.stack([q_rot(_ld(q), _ld(e)) for e in np.eye(3)], axis=1)


def adjoint(T):
    """Ad(T) of T = (q, t) in the (upsilon, omega) order: [[R, [t]x R], [0, R]]."""
    R = _rot(T[:4])
    A = np.zeros((6, 6), LD)
    A[:3, :3], A[3:, 3:], A[:3, 3:] = R, R, _skew(_ld(T[4:])) @ R
    return A


class RigProblem:
    """A vsl_ba_problem + vsl_ba_rig.  For ba_ref.linearize / lm_step the POSE BLOCKS are the bodies: poses = body poses,
    cam_fixed = body_fixed, obs_cam = the body of each observation."""

    def __init__(self, body_poses, body_fixed, cam_body, cam_intr, T_b_c, intr, points, obs_camera, obs_lm, obs_uv, cam_model,
                 name="", use_huber=True, huber=1.0):
        self.poses = np.ascontiguousarray(body_poses, np.float64).reshape(-1, 7).copy()
        self.cam_fixed = np.ascontiguousarray(body_fixed, np.uint8).copy()
        self.cam_body = np.ascontiguousarray(cam_body, np.int32).copy()
        self.cam_intr = np.ascontiguousarray(cam_intr, np.int32).copy()
        self.T_b_c = np.ascontiguousarray(T_b_c, np.float64).reshape(2, 7).copy()
        self.intr = np.ascontiguousarray(intr, np.float64).reshape(2, 8).copy()
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
        self.obs_camera = np.ascontiguousarray(obs_camera, np.int32).copy()
        self.obs_lm = np.ascontiguousarray(obs_lm, np.int32).copy()
        self.obs_uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2).copy()
        self.cam_model = tuple(int(m) for m in cam_model)
        self.name, self.use_huber, self.huber, self.fd_step = name, bool(use_huber), float(huber), ba_ref.FD_STEP

    # ---- what ba_ref.linearize / lm_step read
    @property
    def obs_cam(self):
        return self.cam_body[self.obs_camera]

    @property
    def n_free(self):
        return int((self.cam_fixed == 0).sum())

    def free_index(self):
        free = np.cumsum(self.cam_fixed == 0) - 1
        free[self.cam_fixed != 0] = -1
        return free

    def cameras(self, bodies=None):
        """T_w_c [C, 7] in long double."""
        b = _ld(self.poses if bodies is None else bodies)
        T = se3_mul(b[self.cam_body], _ld(self.T_b_c)[self.cam_intr])
        T[:, :4] /= np.sqrt(np.sum(T[:, :4] ** 2, axis=1, keepdims=True))
        return T

    def obs_model(self):
        return np.asarray(self.cam_model)[self.cam_intr[self.obs_camera]]

    def blocks(self, poses=None, points=None, jac=True):
        """r, F_b, E, FD disagreement per observation (jac=False: r alone) at (bodies, points)."""
        P = self.cameras(poses)[self.obs_camera]
        X = _ld(self.points if points is None else points)[self.obs_lm]
        k = self.cam_intr[self.obs_camera]
        ip, model = _ld(self.intr)[k], self.obs_model()
        if not jac:
            return ba_ref.residual(model, ip, P, X, self.obs_uv)
        r, F_c, E, dis_c = ba_ref.residual_jacobian(model, ip, P, X, self.obs_uv, self.fd_step)
        Tbc = _ld(self.T_b_c)[k]
        pc = ba_ref.camera_point(P, X)
        dist = np.sqrt(np.sum(pc * pc, axis=-1))
        D = [self._central_body(model, ip, Tbc, pc, LD(self.fd_step) * dist / s, np.full(dist.shape, LD(self.fd_step) / s))
             for s in (1, 2, 4)]
        J, Jh = (4 * D[1] - D[0]) / 3, (4 * D[2] - D[1]) / 3
        dis = np.maximum(dis_c, np.abs(J - Jh).max(axis=(-1, -2)) / np.abs(J).max(axis=(-1, -2)))
        self.last_F_c = F_c
        return r, J, E, dis

    @staticmethod
    def _central_body(model, ip, Tbc, pc, h_t, h_r):
        """D(h) [O, 2, 6] of -project along T_w_b * exp(d) * T_b_c, acting on the camera-frame point pc."""
        pb = q_rot(Tbc[..., :4], pc) + Tbc[..., 4:]
        qcb = q_conj(Tbc[..., :4])
        cols = []
        for k in range(6):
            h = h_t if k < 3 else h_r
            d = np.zeros(pc.shape[:-1] + (6,), LD)
            d[..., k] = h
            out = []
            for sign in (1, -1):
                e = se3_exp(sign * d)
                pb2 = q_rot(q_conj(e[..., :4]), pb - e[..., 4:])
                out.append(-ba_ref.project(model, ip, q_rot(qcb, pb2 - Tbc[..., 4:])))
            cols.append((out[0] - out[1]) / (2 * h)[..., None])
        return np.stack(cols, axis=-1)

    def cost(self, poses=None, points=None):
        r = self.blocks(poses, points, jac=False)
        z6, z3 = np.zeros(r.shape + (6,), LD), np.zeros(r.shape + (3,), LD)
        return float(np.sum(ba_ref.huber_correct(r, z6, z3, self.use_huber, self.huber)[3]))

    # ---- the free problem of the same cameras
    def expanded(self, bodies=None, points=None):
        cams = self.cameras(bodies).astype(np.float64)
        return ba_ref.Problem(cams, self.cam_fixed[self.cam_body], self.cam_intr, self.intr,
                              self.points if points is None else points, self.obs_camera, self.obs_lm, self.obs_uv, self.cam_model,
                              self.name + "/expanded", use_huber=self.use_huber, huber=self.huber)

    def fold_matrix(self):
        """A [6 free cameras, 6 free bodies] (long double)."""
        slot = self.free_index()
        cam_free = np.flatnonzero(self.cam_fixed[self.cam_body] == 0)
        A = np.zeros((6 * len(cam_free), 6 * self.n_free), LD)
        for fc, c in enumerate(cam_free):
            s = slot[self.cam_body[c]]
            A[6 * fc:6 * fc + 6, 6 * s:6 * s + 6] = adjoint(se3_inv(_ld(self.T_b_c[self.cam_intr[c]])))
        return A

    def adjoint_jacobian(self):
        """F_c Ad(T_b_c^-1) per observation, F_c from ba_ref (call blocks() first): the closed form of the definition."""
        Ad = np.stack([adjoint(se3_inv(_ld(self.T_b_c[k]))) for k in (0, 1)])
        return self.last_F_c @ Ad[self.cam_intr[self.obs_camera]]


def linearize(rp, inv_radius=None):
    """ba_ref.linearize over [free bodies | landmarks]: S, g, A_S, A_g, cost, D, dc, dl, cond_S, ... (a ba_ref.Lin)."""
    return ba_ref.linearize(rp, inv_radius)


def lm_step(rp, inv_radius=1e-4):
    """One LM step: (candidate bodies, candidate points, body step, landmark step, cost, candidate cost, Lin)."""
    return ba_ref.lm_step(rp, inv_radius)


# ----------------------------------------------------------------------------------------------------------- fixtures
def extrinsics(identity=False):
    """Block 0: 1 cm and 0.5 degrees off the body frame; block 1: a 0.11 m baseline plus a 2 degree rotation ([t]x R counts)."""
    if identity:
        return np.array([ba_ref.IDENT, ba_ref.IDENT])
    e0 = np.concatenate([se3_exp(_ld([0, 0, 0, 0.004, -0.007, 0.003]))[:4], [0.006, -0.005, 0.006]]).astype(np.float64)
    w = np.deg2rad(2.0) * np.array([0.36, 0.8, -0.48])
    e1 = np.concatenate([se3_exp(_ld([0, 0, 0, *w]))[:4], [0.11, 0.004, -0.003]]).astype(np.float64)
    return np.array([e0, e1])


def rig_scene(n_bodies, n_fixed, n_lms, seed, models=(0, 0), cams_of_body=None, identity=False, window=None, seen_by_all=0,
              noise=0.5, drift_t=0.01, drift_r=0.01, name="", T_b_c=None, **kw):
    """Bodies on an arc of radius 4 looking at a cloud of landmarks round the origin; body b carries the cameras
    cams_of_body[b] (intrinsics blocks; default both).  window None: every camera sees every landmark; a number: landmark
    l is seen by the fixed bodies and by `window` consecutive free bodies from free body l on (wrapping), the first
    `seen_by_all` landmarks by everything.  The bodies handed in are the true ones * exp((drift_t N, drift_r N)), the
    points the true ones + drift_t N; the observations are the true projections + noise px.  T_b_c overrides the
    extrinsics."""
    rng = np.random.default_rng(seed)
    bodies = []
    for b in range(n_bodies):
        a = -0.25 + 0.5 * (b + 0.5) / n_bodies
        pos = np.array([4 * np.sin(a), 0.3 * np.sin(5.0 * b), -4 * np.cos(a)])
        T = np.concatenate([[0, -np.sin(a / 2), 0, np.cos(a / 2)], pos])
        bodies.append(se3_mul(_ld(T), se3_exp(_ld(np.concatenate([np.zeros(3), 0.05 * rng.normal(size=3)])))).astype(np.float64))
    bodies = np.array(bodies)
    bodies[:, :4] /= np.linalg.norm(bodies[:, :4], axis=1, keepdims=True)
    points = rng.uniform(-0.4, 0.4, (n_lms, 3))
    if cams_of_body is None:
        cams_of_body = [(0, 1)] * n_bodies
    cam_body = np.array([b for b, ks in enumerate(cams_of_body) for _ in ks])
    cam_intr = np.array([k for ks in cams_of_body for k in ks])
    body_fixed = np.zeros(n_bodies, np.uint8)
    body_fixed[:n_fixed] = 1
    C = len(cam_body)
    oc, ol = np.tile(np.arange(C), n_lms), np.repeat(np.arange(n_lms), C)
    if window is not None:
        nf = n_bodies - n_fixed
        ob = cam_body[oc]
        keep = (ob < n_fixed) | (ol < seen_by_all) | (((ob - n_fixed) - ol) % nf < window)
        oc, ol = oc[keep], ol[keep]
    intr = np.array([ba_ref.INTR[models[0]], ba_ref.INTR[models[1]]])
    rp = RigProblem(bodies, body_fixed, cam_body, cam_intr, extrinsics(identity) if T_b_c is None else T_b_c, intr, points, oc, ol, np.zeros((len(oc), 2)), models,
                    name, **kw)
    rp.obs_uv = (-rp.blocks(jac=False) + _ld(noise * rng.normal(size=(len(oc), 2)))).astype(np.float64)
    d = np.concatenate([drift_t * rng.normal(size=(n_bodies, 3)), drift_r * rng.normal(size=(n_bodies, 3))], axis=1)
    d[body_fixed != 0] = 0
    moved = se3_mul(_ld(rp.poses), se3_exp(_ld(d))).astype(np.float64)
    moved[:, :4] /= np.linalg.norm(moved[:, :4], axis=1, keepdims=True)
    rp.poses = moved
    rp.points = rp.points + drift_t * rng.normal(size=rp.points.shape)
    return rp


def _drop(rp, keep):
    rp.obs_camera, rp.obs_lm, rp.obs_uv = rp.obs_camera[keep].copy(), rp.obs_lm[keep].copy(), rp.obs_uv[keep].copy()
    return rp


def base_case(name="a_base", seed=500, **kw):
    """3 bodies x 2 cameras, body 0 fixed, 9 landmarks; a few observations missing so that the blocks are not uniform."""
    rp = rig_scene(3, 1, 9, seed, name=name, **kw)
    cam, lm = rp.obs_camera, rp.obs_lm
    return _drop(rp, ~(((cam == 3) & (lm == 1)) | ((cam == 4) & (lm == 2)) | ((cam == 1) & (lm == 6)) | ((cam == 2) & (lm == 7))))


def _build_cases():
    T = {}
    T["a_base"] = base_case()
    T["b_all_see_all"] = rig_scene(3, 1, 9, 501)
    rp = rig_scene(3, 1, 9, 502)
    T["c_fixed_body_only"] = _drop(rp, ~((rp.obs_lm == 3) & (rp.cam_body[rp.obs_camera] != 0)))
    rp = rig_scene(3, 1, 9, 503)
    T["d_one_body_left_right"] = _drop(rp, ~((rp.obs_lm == 4) & (rp.cam_body[rp.obs_camera] != 1)))
    T["e_single_camera_body"] = rig_scene(3, 1, 9, 504, cams_of_body=[(0, 1), (0, 1), (1,)])
    T["f_models"] = rig_scene(3, 1, 9, 505, models=(0, 3))
    rp = rig_scene(3, 1, 9, 506, use_huber=True, huber=1.0)
    i0 = int(np.flatnonzero((rp.obs_camera == 2) & (rp.obs_lm == 1))[0])
    i1 = int(np.flatnonzero((rp.obs_camera == 5) & (rp.obs_lm == 5))[0])
    rp.obs_uv[i0] += [35.0, -22.0]
    rp.obs_uv[i1] += [-28.0, 41.0]
    rp.outliers = (i0, i1)
    T["g_huber_outliers"] = rp
    # 23 free bodies = 138 unknowns (past the 128 of the small dense solver); landmark 0 seen by the 2 cameras of the
    # fixed body and of 14 free bodies = 30 cameras, every other landmark by the fixed body and 3 free bodies
    rp = rig_scene(24, 1, 24, 507, window=3)
    have = set(rp.obs_camera[rp.obs_lm == 0].tolist())
    extra_c = np.array([c for c in range(len(rp.cam_body)) if 4 <= rp.cam_body[c] <= 14 and c not in have])
    rp.obs_camera = np.concatenate([rp.obs_camera, extra_c]).astype(np.int32)
    rp.obs_lm = np.concatenate([rp.obs_lm, np.zeros(len(extra_c), np.int32)]).astype(np.int32)
    rp.obs_uv = np.concatenate([rp.obs_uv, np.zeros((len(extra_c), 2))])
    true_uv = rp.obs_uv - rp.blocks(jac=False).astype(np.float64)        # projections at the handed-in point
    rng = np.random.default_rng(5071)
    rp.obs_uv[-len(extra_c):] = true_uv[-len(extra_c):] + 0.5 * rng.normal(size=(len(extra_c), 2))
    T["h_23_free"] = rp
    T["i_identity_single"] = rig_scene(4, 1, 9, 508, cams_of_body=[(0,)] * 4, identity=True)
    for name, rp in T.items():
        rp.name = name
    return T


_CASES = None
_LIN = {}


def cases():
    """name -> RigProblem, built once (treat as read-only; copy() what a solve changes)."""
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
