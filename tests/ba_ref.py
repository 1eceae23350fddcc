"""TEST INFRASTRUCTURE: plain high-precision numpy reference of one bundle-adjustment linearisation and one
Levenberg-Marquardt step (ba.hip, ba_fused.hip, ba_large.h, orc_ba.cpp), in the style of pgo_ref.py.  numpy only,
np.longdouble throughout; imports neither the package nor the oracle (the SE(3) helpers are pgo_ref's).

  projection  the four camera models from their definitions (0 double sphere, 1 pinhole, 2 EUCM, 3 Kannala-Brandt 4);
              the KB4 value on the axis is (cx, cy)
  residual    r = uv - project(R^T (p - t)), pose = qx qy qz qw tx ty tz (T_w_c)
  Jacobians   F = d r / d (upsilon, omega) along T * exp(delta) and E = d r / d p by central differences D(h) in long
              double, Richardson extrapolated: J = (4 D(h/2) - D(h)) / 3 -- nothing of the kernels' closed forms.  The step
              is h radians for omega and h * |p_c| (the point's distance from the camera) for upsilon and p, h = 3e-4
              (at 1e-4 the rounding of the 85 degree cases is 1.8e-14, at 1e-3 their truncation 1.1e-13; they stay
              > 0.1 rad inside their domain), applied to the camera-frame point so that nothing is rounded at the size
              of t or p.  The
              function repeats itself at half the step and reports max|J(h) - J(h/2)| / max|block| per observation.
  Huber       r and J scaled by sqrt(rho'); rho' = 1 for s <= a^2, a / sqrt(s) beyond; cost = rho / 2
  assembly    dense H = J^T J, b = J^T r over [free cameras in ascending id, 6 each | landmarks, 3 each]
  reduction   S = H_cc - sum_l W_l P_l^-1 W_l^T, g = b_c - sum_l W_l P_l^-1 b_l, landmark by landmark in long double
              (a landmark no free camera sees contributes nothing), and beside them the entrywise magnitudes
                A_S = sum_obs |F|^T |F| (+ |damping|) + sum_l kappa_l |W_l| |P_l^-1| |W_l|^T,   kappa_l = cond_2(P_l)
                A_g = sum_obs |F|^T |r|               + sum_l kappa_l |W_l| |P_l^-1| |b_l|
              an entry of a double-precision S passes when |S - S_ref| <= K * 2^-52 * A_S (ratio(): the K it needs)
  fused form  column scale D = 1 / (1 + sqrt(diag H)) and damping clamp(diag, 1e-6, 1e32) * inv_radius on the scaled
              diagonal, cameras and landmarks alike; then the same reduction.  kappa_l stays cond_2 of the PLAIN P_l,
              whatever the variables: at 1 / radius = 0 the system is D_c S D_c, D_c g of the plain one and the bound is
              D_c A_S D_c, D_c A_g.  (Column scaling equilibrates P_l and would shrink kappa_l, but the blocks F, E that
              P_l is built from are accurate relative to their largest entry only, which scaling a column does not
              improve.)
  LM step     the damped scaled system solved in long double (Cholesky of S', back-substitution), unscaled; candidate
              poses T * exp(step_c), candidate points p + step_l

Cases dropped from the MEASUREMENT of the constants because the oracle alone cannot hold them (Problem.oracle says what
is left of each); the GPU tests still run them, under the constants measured on the rest:
  * the Jacobian -- and so S, g -- of the KB4 point exactly on the axis: orc_ba.cpp differentiates with dual numbers,
    where `sqrt(0)` has a NaN derivative and the r == 0 branch a constant one.  Its residual stays in.
  * far1e3 (camera and points 1e3 from the origin), everything: the oracle forms R^T p + R^T (-t), two numbers of 1e3
    that cancel: residuals off by 5e-11 px, S / g by up to 460 units.
  * S, g and cost of structure/cams64 and cams65: 15 to 21 units in S, in entries that are all W P^-1 W^T of the
    landmark that 64 / 65 cameras see (sums of 64 terms); their residuals and Jacobian blocks stay in.  So
    ORACLE_VS_REF_K is measured without the two, and the device's 8 x it is what they are held to.
  * the shallow-depth rig stands 0.02 from the origin: 2 m away the rounding of the oracle's p_c alone is 2.5e-12 px
    at 3500 px / m (17 units in g).
Out of scope: a landmark with a single observation (P_l singular by construction).
"""
import numpy as np

from pgo_ref import LD, _ld, q_conj, q_rot, se3_exp, se3_mul

U = 2.0 ** -52

# ---- measured by tests/test_ba_ref_cpu.py (x86-64, 80-bit long double) over every table below; it prints the figures
# and asserts that none exceeds its constant.  Recorded rounded up.  The GPU tests allow 8 x each (caps beside them).
# S, g entrywise in units of 2^-52 A: measured 6.26 (g of obs/ds/rot_identity; Huber table 0.85, structure table 3.37)
ORACLE_VS_REF_K = 6.5
K_GPU = min(8.0 * ORACLE_VS_REF_K, 64.0)
# residuals, px absolute: measured 3.13e-13 (obs/ds/angle60)
ORACLE_VS_REF_RES = 4.0e-13
RES_GPU = min(8.0 * ORACLE_VS_REF_RES, 1e-11)
# cost, relative: measured 9.42e-14 (obs/ds/negz)
ORACLE_VS_REF_COST = 1.0e-13
COST_GPU = 8.0 * ORACLE_VS_REF_COST
# Jacobian blocks, relative to the block's largest entry: measured 3.28e-15 (obs/ds/negz)
ORACLE_VS_REF_JAC = 3.5e-15
# The reference's own resolution: the step-halving disagreement of its finite differences, PER CASE.  A Jacobian
# tolerance below 10 x that would test the reference, not the kernels, so a case's tolerance is jac_tol(name) =
# max(8 x ORACLE_VS_REF_JAC, 10 x that case's own disagreement), at most 1e-9.  FD_RESOLUTION is the largest
# disagreement over all cases, recorded rounded up (measured 4.92e-15, obs/kb4/angle85; the 60 / 85 degree and z < 0 cases are the ones above 2.8e-15, i.e. with a
# tolerance of their own, at most 4.9e-14): no case's tolerance exceeds
# max(8 x ORACLE_VS_REF_JAC, 10 x FD_RESOLUTION), and test_ba_ref_cpu.py asserts both.
FD_RESOLUTION = 5.0e-15

FD_STEP = 3e-4
INTR = {0: [350.0, 348.0, 365.0, 249.0, -0.24, 0.57, 0, 0],
        1: [350.0, 348.0, 365.0, 249.0, 0, 0, 0, 0],
        2: [350.0, 348.0, 365.0, 249.0, 0.6, 1.1, 0, 0],
        3: [350.0, 348.0, 365.0, 249.0, 0.01, -0.004, 0.002, -0.0005]}
MODEL_NAMES = {0: "ds", 1: "pinhole", 2: "eucm", 3: "kb4"}


# ------------------------------------------------------------------------------------------------------ projection
def _project_one(model, ip, p):
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    fx, fy, cx, cy = ip[..., 0], ip[..., 1], ip[..., 2], ip[..., 3]
    if model == 1:
        return np.stack([fx * x / z + cx, fy * y / z + cy], axis=-1)
    if model == 2:
        alpha, beta = ip[..., 4], ip[..., 5]
        den = alpha * np.sqrt(beta * (x * x + y * y) + z * z) + (1 - alpha) * z
        return np.stack([fx * x / den + cx, fy * y / den + cy], axis=-1)
    if model == 3:
        r = np.sqrt(x * x + y * y)
        th = np.arctan2(r, z)
        t2 = th * th
        d = th * (1 + t2 * (ip[..., 4] + t2 * (ip[..., 5] + t2 * (ip[..., 6] + t2 * ip[..., 7]))))
        safe = np.where(r > 0, r, LD(1))
        return np.stack([np.where(r > 0, fx * d * x / safe, LD(0)) + cx, np.where(r > 0, fy * d * y / safe, LD(0)) + cy], axis=-1)
    xi, alpha = ip[..., 4], ip[..., 5]
    d1 = np.sqrt(x * x + y * y + z * z)
    k = xi * d1 + z
    den = alpha * np.sqrt(x * x + y * y + k * k) + (1 - alpha) * k
    return np.stack([fx * x / den + cx, fy * y / den + cy], axis=-1)


def project(model, ip, p):
    """model [O] (or a scalar), ip [O, 8], p [O, 3] in the camera frame -> uv [O, 2]."""
    ip, p = _ld(ip), _ld(p)
    model = np.broadcast_to(np.asarray(model), p.shape[:-1])
    out = np.zeros(p.shape[:-1] + (2,), LD)
    for m in np.unique(model):
        k = model == m
        out[k] = _project_one(int(m), np.broadcast_to(ip, p.shape[:-1] + (8,))[k], p[k])
    return out


def camera_point(pose, pw):
    pose, pw = _ld(pose), _ld(pw)
    return q_rot(q_conj(pose[..., :4]), pw - pose[..., 4:])


def residual(model, ip, pose, pw, uv):
    return _ld(uv) - project(model, ip, camera_point(pose, pw))


def _central(model, ip, pose, pc, h_t, h_r):
    """D(h) [O, 2, 9] of -project about the camera-frame point pc.  The perturbations act ON pc, which is what they do to
    R^T (p - t) exactly: T * exp(d) moves it to exp(d)^-1 pc, p + d to pc + R^T d.  (Perturbing pose and point
    themselves rounds t + h and p + h at the size of t and p: 1e3 from the origin that alone was a disagreement of
    4e-13.)"""
    cols = []
    qc = q_conj(pose[..., :4])
    for k in range(9):
        if k < 6:
            h = h_t if k < 3 else h_r
            d = np.zeros(pc.shape[:-1] + (6,), LD)
            d[..., k] = h
            out = []
            for sign in (1, -1):
                e = se3_exp(sign * d)
                out.append(-project(model, ip, q_rot(q_conj(e[..., :4]), pc - e[..., 4:])))
        else:
            h = h_t
            d = np.zeros(pc.shape, LD)
            d[..., k - 6] = h
            rd = q_rot(qc, d)
            out = [-project(model, ip, pc + rd), -project(model, ip, pc - rd)]
        cols.append((out[0] - out[1]) / (2 * h)[..., None])
    return np.stack(cols, axis=-1)          # [O, 2, 9]


def residual_jacobian(model, ip, pose, pw, uv, h=FD_STEP):
    """r [O, 2], F [O, 2, 6], E [O, 2, 3] and the step-halving disagreement per observation [O], all vectorised."""
    ip, pose, pw = _ld(ip), _ld(pose), _ld(pw)
    pc = camera_point(pose, pw)
    dist = np.sqrt(np.sum(pc * pc, axis=-1))
    D = [_central(model, ip, pose, pc, LD(h) * dist / s, np.full(dist.shape, LD(h) / s)) for s in (1, 2, 4)]
    J, Jh = (4 * D[1] - D[0]) / 3, (4 * D[2] - D[1]) / 3
    dis = np.maximum(np.abs(J - Jh)[..., :6].max(axis=(-1, -2)) / np.abs(J[..., :6]).max(axis=(-1, -2)),
                     np.abs(J - Jh)[..., 6:].max(axis=(-1, -2)) / np.abs(J[..., 6:]).max(axis=(-1, -2)))
    return residual(model, ip, pose, pw, uv), J[..., :6], J[..., 6:], dis


def huber_correct(r, F, E, use_huber, huber):
    s = np.sum(r * r, axis=-1)
    a = LD(huber)
    out = bool(use_huber) & (s > a * a)
    rt = np.sqrt(np.where(out, s, LD(1)))
    k = np.sqrt(np.where(out, a / rt, LD(1)))
    rho = np.where(out, 2 * a * rt - a * a, s)
    return k[..., None] * r, k[..., None, None] * F, k[..., None, None] * E, rho / 2, out


# --------------------------------------------------------------------------------------------------------- problems
class Problem:
    """The numpy fields of vsl_ba_problem (what Context._ba_struct and orc.BaArrays take) and how to linearise it."""

    def __init__(self, poses, cam_fixed, cam_intr, intr, points, obs_cam, obs_lm, obs_uv, cam_model, name="", use_huber=True,
                 huber=1.0, fd_step=FD_STEP, oracle="all"):
        self.poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7).copy()
        self.cam_fixed = np.ascontiguousarray(cam_fixed, np.uint8).copy()
        self.cam_intr = np.ascontiguousarray(cam_intr, np.int32).copy()
        self.intr = np.ascontiguousarray(intr, np.float64).reshape(2, 8).copy()
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
        self.obs_cam = np.ascontiguousarray(obs_cam, np.int32).copy()
        self.obs_lm = np.ascontiguousarray(obs_lm, np.int32).copy()
        self.obs_uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2).copy()
        self.cam_model = tuple(int(m) for m in cam_model)
        self.name, self.use_huber, self.huber, self.fd_step = name, bool(use_huber), float(huber), fd_step
        # what the oracle is measured on: "all"; "blocks" (residuals and Jacobians, not S / g / cost); "not_special" (blocks
        # of every observation but `special`, whose residual alone counts); "none"
        self.oracle = oracle
        self.special = None          # index of the observation a table row is about

    @property
    def n_free(self):
        return int((self.cam_fixed == 0).sum())

    def free_index(self):
        free = np.cumsum(self.cam_fixed == 0) - 1
        free[self.cam_fixed != 0] = -1
        return free

    def obs_model(self):
        return np.asarray(self.cam_model)[self.cam_intr[self.obs_cam]]

    def blocks(self, poses=None, points=None, jac=True):
        """Raw r, F, E, FD disagreement of every observation at (poses, points) (default: the problem's own)."""
        P = _ld(self.poses if poses is None else poses)[self.obs_cam]
        X = _ld(self.points if points is None else points)[self.obs_lm]
        ip = _ld(self.intr)[self.cam_intr[self.obs_cam]]
        if not jac:
            return residual(self.obs_model(), ip, P, X, self.obs_uv)
        return residual_jacobian(self.obs_model(), ip, P, X, self.obs_uv, self.fd_step)

    def cost(self, poses=None, points=None):
        r = self.blocks(poses, points, jac=False)
        z6, z3 = np.zeros(r.shape + (6,), LD), np.zeros(r.shape + (3,), LD)
        return float(np.sum(huber_correct(r, z6, z3, self.use_huber, self.huber)[3]))


def _inv3(P):
    a, b, c, d, e, f = P[0, 0], P[0, 1], P[0, 2], P[1, 1], P[1, 2], P[2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    return np.array([[c00, c01, c02], [c01, a * f - c * c, b * c - a * e], [c02, b * c - a * e, a * d - b * b]], LD) / det


def _cholesky_solve(S, b):
    """x with S x = b for a symmetric positive definite S, in long double."""
    n = len(b)
    Lm = np.zeros((n, n), LD)
    for j in range(n):
        d = S[j, j] - np.sum(Lm[j, :j] ** 2)
        if not d > 0:
            return None                      # not positive definite (an undamped window whose scale is free)
        Lm[j, j] = np.sqrt(d)
        if j + 1 < n:
            Lm[j + 1:, j] = (S[j + 1:, j] - Lm[j + 1:, :j] @ Lm[j, :j]) / Lm[j, j]
    y = np.zeros(n, LD)
    for j in range(n):
        y[j] = (b[j] - np.sum(Lm[j, :j] * y[:j])) / Lm[j, j]
    x = np.zeros(n, LD)
    for j in reversed(range(n)):
        x[j] = (y[j] - np.sum(Lm[j + 1:, j] * x[j + 1:])) / Lm[j, j]
    return x


class Lin:
    """One linearisation.  Everything is long double unless named otherwise; see linearize()."""


def linearize(prob, inv_radius=None):
    """inv_radius None: the plain system (vsl_ba_linearize: no scaling, no damping).  A number: the system the fused
    kernels build -- columns scaled by D, the scaled diagonal damped.  Fields: r, F, E (raw blocks), outlier (Huber
    branch per observation), fd_disagreement, cost, H, b (dense, before scaling), D (ones when unscaled), S, g, A_S, A_g,
    kappa [L] (cond_2 of the plain landmark blocks, 0 where not reduced), and for a damped or well-posed system
    dc, dl (the solution of S dc = -g with the back-substituted landmarks, in the scaled variables), cond_S, cond_H."""
    out = Lin()
    nf, L, O = prob.n_free, len(prob.points), len(prob.obs_cam)
    nc, N = 6 * nf, 6 * nf + 3 * L
    out.r, out.F, out.E, dis = prob.blocks()
    out.fd_disagreement = float(dis.max())
    r, F, E, cost, out.outlier = huber_correct(out.r, out.F, out.E, prob.use_huber, prob.huber)
    out.cost = float(np.sum(cost))
    free = prob.free_index()
    fc = free[prob.obs_cam]
    H, b = np.zeros((N, N), LD), np.zeros(N, LD)
    for i in range(O):
        l = nc + 3 * prob.obs_lm[i]
        H[l:l + 3, l:l + 3] += E[i].T @ E[i]
        b[l:l + 3] += E[i].T @ r[i]
        if fc[i] >= 0:
            c = 6 * fc[i]
            H[c:c + 6, c:c + 6] += F[i].T @ F[i]
            H[c:c + 6, l:l + 3] += F[i].T @ E[i]
            H[l:l + 3, c:c + 6] += E[i].T @ F[i]
            b[c:c + 6] += F[i].T @ r[i]
    out.H, out.b = H, b
    D = np.ones(N, LD)
    damp = np.zeros(N, LD)
    if inv_radius is not None:
        D = 1 / (1 + np.sqrt(np.diag(H)))
        damp = np.clip(D * np.diag(H) * D, LD(1e-6), LD(1e32)) * LD(inv_radius)
    out.D, out.damp = D, damp
    Hs, bs = D[:, None] * H * D[None, :] + np.diag(damp), D * b
    # magnitudes: sum over observations of |F|^T |F| and |F|^T |r| in the variables of the system
    A_S, A_g = np.zeros((nc, nc), LD), np.zeros(nc, LD)
    for i in range(O):
        if fc[i] >= 0:
            c = 6 * fc[i]
            Fa = np.abs(F[i]) * D[c:c + 6][None, :]
            A_S[c:c + 6, c:c + 6] += Fa.T @ Fa
            A_g[c:c + 6] += Fa.T @ np.abs(r[i])
    A_S += np.diag(damp[:nc])
    S, g = Hs[:nc, :nc].copy(), bs[:nc].copy()
    out.kappa = np.zeros(L)
    Pinv = {}
    seen = np.bincount(prob.obs_lm, minlength=L)
    for l in range(L):
        s = slice(nc + 3 * l, nc + 3 * l + 3)
        P, W, bl = Hs[s, s], Hs[:nc, s], bs[s]
        if not seen[l] and not np.any(P):
            continue                                            # no observation, no damping: nothing to eliminate
        Pi = Pinv[l] = _inv3(P)
        if not np.any(W):
            continue
        out.kappa[l] = np.linalg.cond(H[s, s].astype(np.float64))       # of the PLAIN block, whatever the variables
        S -= W @ Pi @ W.T
        g -= W @ Pi @ bl
        A_S += LD(out.kappa[l]) * (np.abs(W) @ np.abs(Pi) @ np.abs(W).T)
        A_g += LD(out.kappa[l]) * (np.abs(W) @ np.abs(Pi) @ np.abs(bl))
    out.S, out.g, out.A_S, out.A_g, out.Hs, out.bs = S, g, A_S, A_g, Hs, bs
    out.dc = out.dl = None
    if nc and (inv_radius is not None):
        out.cond_S = float(np.linalg.cond(S.astype(np.float64)))
        live = np.flatnonzero(np.diag(Hs) != 0)
        out.cond_H = float(np.linalg.cond(Hs[np.ix_(live, live)].astype(np.float64)))
        x = _cholesky_solve(S, g)
        out.dc = None if x is None else -x
        out.dl = np.zeros((L, 3), LD)
        for l, Pi in Pinv.items() if x is not None else ():
            s = slice(nc + 3 * l, nc + 3 * l + 3)
            out.dl[l] = -Pi @ (bs[s] + Hs[:nc, s].T @ out.dc)
    return out


def lm_step(prob, inv_radius=1e-4):
    """One Levenberg-Marquardt step from the problem's poses / points: (candidate poses [C, 7], candidate points [L, 3],
    unscaled camera step [n_free, 6], unscaled landmark step [L, 3], cost before, cost at the candidate, Lin)."""
    R = linearize(prob, inv_radius)
    nc = 6 * prob.n_free
    step_c = (R.D[:nc] * R.dc).reshape(-1, 6)
    step_l = R.D[nc:].reshape(-1, 3) * R.dl
    poses = _ld(prob.poses).copy()
    free = np.flatnonzero(prob.cam_fixed == 0)
    if len(free):
        new = se3_mul(poses[free], se3_exp(step_c))
        new[:, :4] /= np.sqrt(np.sum(new[:, :4] ** 2, axis=1, keepdims=True))
        poses[free] = new
    points = _ld(prob.points) + step_l
    return poses, points, step_c, step_l, R.cost, prob.cost(poses, points), R


def ratio(x, ref, A):
    """The K an array needs under |x - ref| <= K * 2^-52 * A; where A is zero the entry has to be equal (else inf)."""
    x, ref, A = np.asarray(x, LD), np.asarray(ref, LD), np.asarray(A, LD)
    if x.size == 0:
        return 0.0
    err = np.abs(x - ref)
    k = np.where(A > 0, err / np.where(A > 0, LD(U) * A, LD(1)), np.where(err > 0, LD(np.inf), LD(0)))
    return float(k.max())


def block_error(J, Jref):
    """max|J - Jref| / max|Jref| per block [O] (trailing two axes)."""
    return (np.abs(np.asarray(J, LD) - Jref).max(axis=(-1, -2)) / np.abs(Jref).max(axis=(-1, -2))).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------- fixtures
def _unit(rng, k=3):
    v = rng.normal(size=k)
    return v / np.linalg.norm(v)


def _pose_mul(T, rel):
    return se3_mul(_ld(T), _ld(rel))


def rig_problem(model, pc, n_cams=4, n_fixed=1, n_lms=9, T1=None, baseline=0.2, spread=0.1, seed=0, noise=0.5, name="",
                exact_first=False, **kw):
    """Camera `n_fixed` (the first free one) at T1 sees landmark 0 at pc in ITS frame; the other cameras stand beside it
    (baseline * |pc| apart, up to 0.02 rad turned), the other landmarks lie within spread * |pc| of landmark 0.  Every
    camera sees every landmark; uv = the projection (long double) + N(0, noise) px.  exact_first: T1 is used bit for bit
    and landmark 0 is pc itself (T1 the identity: the camera-frame point is exact in any arithmetic)."""
    rng = np.random.default_rng(seed)
    pc = np.asarray(pc, np.float64)
    dist = float(np.linalg.norm(pc))
    if T1 is None:
        T1 = np.concatenate([_unit(rng, 4), rng.uniform(-2, 2, 3)])
    T1 = np.asarray(T1, np.float64)
    poses = []
    for c in range(n_cams):
        if c == n_fixed:
            poses.append(T1)
            continue
        w = 0.02 * rng.normal(size=3)
        off = baseline * dist * np.array([np.cos(2.4 * c + 0.3), np.sin(2.4 * c + 0.3), 0.05 * rng.normal()])
        rel = np.concatenate([se3_exp(np.concatenate([np.zeros(3), w]))[:4].astype(np.float64), off])
        poses.append(_pose_mul(T1, rel).astype(np.float64))
    poses = np.array(poses)
    local = [pc] + [pc + spread * dist * rng.uniform(-1, 1, 3) for _ in range(n_lms - 1)]
    points = np.array([(q_rot(_ld(T1[:4]), _ld(p)) + _ld(T1[4:])).astype(np.float64) for p in local])
    if exact_first:
        points[0] = pc
    cam_fixed = np.zeros(n_cams, np.uint8)
    cam_fixed[:n_fixed] = 1
    cam_intr = np.arange(n_cams) % 2
    intr = np.array([INTR[model], INTR[model]])
    oc, ol = np.repeat(np.arange(n_cams), n_lms), np.tile(np.arange(n_lms), n_cams)
    order = np.argsort(ol, kind="stable")       # landmark-major, as the application hands them over
    oc, ol = oc[order], ol[order]
    p = Problem(poses, cam_fixed, cam_intr, intr, points, oc, ol, np.zeros((len(oc), 2)), (model, model), name, **kw)
    uv = -p.blocks(jac=False)
    p.obs_uv = (uv + _ld(noise * rng.normal(size=uv.shape))).astype(np.float64)
    p.special = int(np.flatnonzero((oc == n_fixed) & (ol == 0))[0])
    return p


def _at_angle(deg, dist=4.0, az=0.7):
    a = np.deg2rad(deg)
    return dist * np.array([np.sin(a) * np.cos(az), np.sin(a) * np.sin(az), np.cos(a)])


IDENT = np.array([0, 0, 0, 1.0, 0, 0, 0])


def observation_table():
    """name -> Problem.  Per model: a point exactly on the axis; off-axis ratios r / z of 1e-12, 1e-8, 1e-4 (camera at the
    identity: the ratio is exact); depths 0.1 and 1e3; rotation near the identity and with qw ~ 0; camera and point 1e3
    away from the origin (p - t cancels); two cameras 1 mm apart seeing points 1e3 away (P_l ill-conditioned).  ds, eucm,
    kb4: field angles of 60 and 85 degrees.  ds: a point with z < 0 inside the validity cone (100 degrees)."""
    T = {}
    for m in range(4):
        mn = MODEL_NAMES[m]

        def add(kind, p):
            p.name = "obs/%s/%s" % (mn, kind)
            T[p.name] = p

        add("axis", rig_problem(m, [0, 0, 4.0], T1=IDENT, exact_first=True, seed=10 + m, oracle="not_special" if m == 3 else "all"))
        for e in (12, 8, 4):
            add("ratio1e-%d" % e, rig_problem(m, [4.0 * 0.6 * 10.0 ** -e, 4.0 * 0.8 * 10.0 ** -e, 4.0], T1=IDENT, exact_first=True,
                                              seed=20 + m))
        rng = np.random.default_rng(30 + m)      # (the camera 0.02 from the origin: at 2 m the rounding of p - t alone is 1e-12 px)
        add("depth0.1", rig_problem(m, [0.01, -0.02, 0.1], T1=np.concatenate([_unit(rng, 4), 0.02 * _unit(rng)]), seed=30 + m))
        add("depth1e3", rig_problem(m, [100.0, -150.0, 1e3], seed=40 + m))
        add("rot_identity", rig_problem(m, [0.4, -0.3, 4.0], T1=np.array([1e-9, -2e-9, 3e-9, 1.0, 0.5, -0.3, 0.2]), seed=50 + m))
        add("rot_qw0", rig_problem(m, [0.4, -0.3, 4.0], T1=np.array([0.6, 0.64, 0.48, 1e-9, 0.5, -0.3, 0.2]), seed=60 + m))
        rng = np.random.default_rng(70 + m)
        add("far1e3", rig_problem(m, [0.4, -0.3, 4.0], T1=np.concatenate([_unit(rng, 4), 1e3 * _unit(rng)]), seed=70 + m, oracle="none"))
        add("pair1mm", rig_problem(m, [100.0, -150.0, 1e3], n_cams=2, n_fixed=0, n_lms=4, baseline=1e-6, spread=0.05, seed=80 + m))
        if m != 1:
            add("angle60", rig_problem(m, _at_angle(60), seed=90 + m, spread=0.05))
            add("angle85", rig_problem(m, _at_angle(85), seed=100 + m, spread=0.03, baseline=0.1))
        if m == 0:
            add("negz", rig_problem(m, _at_angle(100), seed=110, spread=0.03, baseline=0.1))
    return T


HUBER_A = 5.0
HUBER_ROWS = ("at", "above", "below", "zero", "huge")


def huber_table():
    """Pinhole; the first free camera is the identity and landmarks 0 .. 4 lie ON its axis, so that their projection is
    (cx, cy) exactly in any arithmetic and r = uv - (cx, cy) is exact in fp64: (3, 4) with a = 5 (s == a^2: the inlier
    branch), one ulp of the observation above and below, r = 0, |r| = 1e6 -- with the Huber loss and without."""
    T = {}
    cx, cy = INTR[1][2], INTR[1][3]
    uvs = [(cx + 3, cy + 4), (np.nextafter(cx + 3, np.inf), cy + 4), (np.nextafter(cx + 3, -np.inf), cy + 4), (cx, cy),
           (cx + 6e5, cy + 8e5)]
    for on in (True, False):
        p = rig_problem(1, [0, 0, 4.0], T1=IDENT, exact_first=True, n_lms=8, seed=200, use_huber=on, huber=HUBER_A)
        rows = []
        for k, uv in enumerate(uvs):
            p.points[k] = [0, 0, 3.0 + 0.5 * k]
            i = int(np.flatnonzero((p.obs_cam == 1) & (p.obs_lm == k))[0])
            rows.append(i)
        # re-observe the moved landmarks from every camera, then plant the exact rows
        rng = np.random.default_rng(201)
        p.obs_uv[:] = 0
        p.obs_uv = (-p.blocks(jac=False) + _ld(0.5 * rng.normal(size=p.obs_uv.shape))).astype(np.float64)
        for i, uv in zip(rows, uvs):
            p.obs_uv[i] = uv
        p.rows = dict(zip(HUBER_ROWS, rows))
        p.name = "huber/%s" % ("on" if on else "off")
        T[p.name] = p
    return T


def scene_problem(n_cams, n_fixed, n_lms, seed, model=0, name="", noise=0.5, drift=0.01, window=None, **kw):
    """Cameras on an arc of radius 4 looking at a cloud of landmarks around the origin.  window None: everything sees
    everything; a number: landmark l is seen by the fixed cameras and by `window` consecutive free ones from free camera
    2 l on (wrapping round), landmark 0 by every camera.  The poses handed in are the true ones times
    exp(drift * N(0, 1)), the points the true ones + drift * N(0, 1)."""
    rng = np.random.default_rng(seed)
    poses = []
    for c in range(n_cams):
        a = -0.25 + 0.5 * (c + 0.5) / n_cams
        pos = np.array([4 * np.sin(a), 0.3 * np.sin(5.0 * c), -4 * np.cos(a)])
        q = np.array([0, -np.sin(a / 2), 0, np.cos(a / 2)])         # z axis towards the origin
        T = np.concatenate([q, pos])
        poses.append(_pose_mul(T, se3_exp(np.concatenate([np.zeros(3), 0.05 * rng.normal(size=3)]))).astype(np.float64))
    poses = np.array(poses)
    points = rng.uniform(-0.4, 0.4, (n_lms, 3))
    cam_fixed = np.zeros(n_cams, np.uint8)
    cam_fixed[:n_fixed] = 1
    oc, ol = np.tile(np.arange(n_cams), n_lms), np.repeat(np.arange(n_lms), n_cams)
    if window is not None:
        nf = n_cams - n_fixed
        keep = (oc < n_fixed) | (ol == 0) | (((oc - n_fixed) - 2 * ol) % nf < window)
        oc, ol = oc[keep], ol[keep]
    intr = np.array([INTR[model], INTR[model]])
    p = Problem(poses, cam_fixed, np.arange(n_cams) % 2, intr, points, oc, ol, np.zeros((len(oc), 2)), (model, model), name, **kw)
    p.obs_uv = (-p.blocks(jac=False) + _ld(noise * rng.normal(size=(len(oc), 2)))).astype(np.float64)
    p.poses = se3_mul(_ld(p.poses), se3_exp(drift * rng.normal(size=(n_cams, 6)))).astype(np.float64)
    p.poses[:, :4] /= np.linalg.norm(p.poses[:, :4], axis=1, keepdims=True)
    p.points = p.points + drift * rng.normal(size=p.points.shape)
    return p


def _drop(p, keep):
    p.obs_cam, p.obs_lm, p.obs_uv = p.obs_cam[keep].copy(), p.obs_lm[keep].copy(), p.obs_uv[keep].copy()
    return p


def structure_table():
    """name -> Problem: n_free of 1, 8 (padded size 48), 16 (96), 21 (n = 126) and 22 (132 unknowns: the large-system
    kernels); one landmark in the whole problem; 32 landmarks of 3 observations in ONE workgroup (chunks of 31 + 1: a
    ragged last chunk); a landmark seen by fixed cameras only and a landmark with no observation; a camera observing one
    landmark twice, and five cameras observing one six times each (the fused plan declines both); one landmark observed by 64 cameras; 65 cameras (the fused plan declines)."""
    T = {}
    for nf, L in ((1, 12), (8, 20), (16, 24), (21, 30), (22, 24)):
        T["structure/n%d" % nf] = scene_problem(nf + 2, 2, L, 300 + nf, window=None if nf < 8 else 4)
    T["structure/one_landmark"] = scene_problem(4, 2, 1, 330)
    T["structure/ragged_chunk"] = scene_problem(3, 1, 32, 331)
    p = scene_problem(5, 2, 12, 332)
    _drop(p, ~((p.obs_lm == 3) & (p.obs_cam >= 2)) & ~(p.obs_lm == 7))         # 3: fixed cameras only; 7: unobserved
    T["structure/fixed_only_and_unobserved"] = p
    p = scene_problem(4, 1, 10, 333)
    k = int(np.flatnonzero((p.obs_lm == 4) & (p.obs_cam == 2))[0])
    p.obs_cam, p.obs_lm = np.insert(p.obs_cam, k, p.obs_cam[k]), np.insert(p.obs_lm, k, p.obs_lm[k])
    p.obs_uv = np.insert(p.obs_uv, k, p.obs_uv[k] + 0.25, axis=0)
    T["structure/observed_twice"] = p
    # landmark 2 seen six times by each of five free cameras: 30 free-camera observations, more than the small Schur
    # kernel's 24 slots -- the host plan has to send the problem to the large-system kernels although n = 30
    p = scene_problem(6, 1, 6, 336)
    rng = np.random.default_rng(337)
    for c in range(1, 6):
        k = int(np.flatnonzero((p.obs_lm == 2) & (p.obs_cam == c))[0])
        p.obs_cam, p.obs_lm = np.insert(p.obs_cam, [k] * 5, c), np.insert(p.obs_lm, [k] * 5, 2)
        p.obs_uv = np.insert(p.obs_uv, [k] * 5, p.obs_uv[k] + 0.3 * rng.normal(size=(5, 2)), axis=0)
    T["structure/observed_30_times"] = p
    T["structure/cams64"] = scene_problem(64, 60, 6, 334, window=2, oracle="blocks")
    T["structure/cams65"] = scene_problem(65, 61, 6, 335, window=2, oracle="blocks")
    for name, p in T.items():
        p.name = name
    return T


_CASES = None


def cases():
    """Every problem the tests linearise, built once: name -> Problem.  Both test files take their cases from here, so
    the constants are measured on what the GPU tests run."""
    global _CASES
    if _CASES is None:
        C = {}
        C.update(observation_table())
        C.update(huber_table())
        C.update(structure_table())
        _CASES = C
    return _CASES


def jac_tol(name):
    """The Jacobian-block tolerance of a case, relative to the block's largest entry (see FD_RESOLUTION)."""
    return min(max(8.0 * ORACLE_VS_REF_JAC, 10.0 * reference(name).fd_disagreement), 1e-9)


_LIN = {}


def reference(name, inv_radius=None):
    """linearize(cases()[name], inv_radius), computed once and shared (treat it as read-only)."""
    key = (name, inv_radius)
    if key not in _LIN:
        _LIN[key] = linearize(cases()[name], inv_radius)
    return _LIN[key]
