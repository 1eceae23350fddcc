"""TEST INFRASTRUCTURE: plain long-double numpy reference of one linearisation and one Levenberg-Marquardt step of bundle
adjustment WITH the two intrinsics blocks free (vsl_bundle_adjust_intrinsics / vsl_ba_intrinsics_system, ba.hip from
"optimize_intrinsics" on), in the style of ba_ref.py, whose projection, residual, pose / landmark finite differences,
Huber rule and helpers it uses unchanged.  numpy only; imports neither the package nor the oracle.

  r, F, E     ba_ref.residual_jacobian (long double central differences, Richardson extrapolated)
  G           d r / d intrinsics (2 x 8 per observation) by central differences on the intrinsics vector in long double,
              Richardson extrapolated as in ba_ref: G = (4 D(h/2) - D(h)) / 3, nothing of the kernels' closed forms.  The
              projection is linear in fx fy cx cy and in KB4's k1..k4: those columns take the step 1 and are exact for any
              step.  xi, alpha (double sphere) and alpha, beta (EUCM) take FD_STEP_INTR = 5e-4, chosen from the sweep that
              test_ba_intr_ref_cpu.py prints (step_sweep() below; worst disagreement over the table 7.9e-13 at 1e-4,
              2.7e-13 at 3e-4, 1.8e-13 at 5e-4, 7.3e-13 at 1e-3, 1.2e-11 at 2e-3: rounding ~ 1 / h below, truncation
              ~ h^4 above).  The columns a
              model does not use are exactly zero (they are never differenced), and so is every column but cx, cy of a
              KB4 point exactly on the axis (its projection is (cx, cy) whatever the other parameters: the differences are
              of equal numbers, the cx / cy ones of cx +- h, exact).  The function repeats itself at half the step and reports max|G(h) - G(h/2)| /
              max|block| per observation.
  assembly    dense H = J^T J, b = J^T r over [free cameras in ascending id, 6 each | intrinsics block 0, 8 | block 1, 8 |
              landmarks, 3 each], J = [F | G | E] per observation with ba_ref.huber_correct's factor on all three blocks.
              An observation in a FIXED camera has no F but keeps its G and E.
  reduction   the landmarks eliminated one by one in long double: S ((n + 16)^2), g, and the entrywise magnitudes by
              ba_ref's rule with [F | G] in the place of F:
                A_S = sum_obs |J_c|^T |J_c| (+ |damping|) + sum_l kappa_l |W_l| |P_l^-1| |W_l|^T,  kappa_l = cond_2(plain P_l)
                A_g = sum_obs |J_c|^T |r|                 + sum_l kappa_l |W_l| |P_l^-1| |b_l|
  scaled,     D = 1 / (1 + sqrt(diag H)) over ALL columns (a zero column: D = 1), damping clamp(diag(D H D), 1e-6, 1e32) *
  damped      inv_radius on the scaled diagonal, then the same reduction: the system the solver factorises
  LM step     d (n + 16) and dl in the scaled variables by a long-double Cholesky; candidate poses T exp(D d_c), candidate
              intrinsics intr + D d_i, candidate points p + D dl; cond_2 of S; cost, candidate cost, model change and the
              gain ratio the LM policy judges

Cases (cases()): each the smallest shape that still reaches the seam it names; see _build_cases.  Unless it says
otherwise a case has 3 cameras (0 fixed on block 0, 1 free on block 1, 2 free on block 0).  At 1 / radius = 0 the
reduced system of every case whose models leave a parameter unused (all but KB4 on both blocks) has a zero row and
column there, and with one fixed camera the scale of the scene is free as well: those systems are singular whatever
the kernels do, the factorisation has to report it (chol_ok == 0), and their undamped step is not compared
(UNDAMPED_SOLVABLE lists the cases whose step IS compared undamped; test_ba_intr_ref_cpu.py holds it to the reference).
At 1 / radius = 1e-4 every case is solvable.

Cases dropped from the MEASUREMENT of the constants because the oracle alone cannot hold them; the GPU tests still run
them, under the constants measured on the rest:
  * G, S and g of kb4_awkward: it contains a KB4 point exactly on the axis; orc_ba.cpp differentiates with dual numbers,
    where `sqrt(0)` has a NaN derivative.  G of its other observations stays in.
Out of scope: a landmark with a single observation (P_l singular by construction); extrinsics; the rig / global /
iterative routes (none has an intrinsics variant).
"""
import numpy as np

import ba_ref
from ba_ref import U, INTR, IDENT, Problem, _at_angle, _cholesky_solve, _inv3, block_error, ratio  # noqa: F401 (re-exported)
from pgo_ref import LD, _ld, se3_exp, se3_mul

# ---- measured by tests/test_ba_intr_ref_cpu.py (x86-64, 80-bit long double) over cases(); it prints the figures and
# asserts that none exceeds its constant.  Recorded rounded up.
# S, g entrywise in units of 2^-52 A: measured 12.03 (i_seam_18_free; the oracle's blocks are summed and reduced by float64
# numpy there, 134 observations in matrix-product order)
ORACLE_VS_REF_K_INTR = 12.5
K_INTR_GPU = min(8.0 * ORACLE_VS_REF_K_INTR, 64.0)
# G relative to the block's largest entry: measured 6.96e-14 (g_eucm_60: the finite differences of alpha / beta, not the
# oracle's dual numbers, set it -- see the sweep)
ORACLE_VS_REF_JAC_INTR = 7.0e-14
# the largest step-halving disagreement of the finite differences (F, E and G): measured 1.71e-13 (a_eucm).  A case's
# Jacobian tolerance is jac_tol(name) = min(max(8 x ORACLE_VS_REF_JAC_INTR, 10 x its own disagreement), 1e-9)
FD_RESOLUTION_INTR = 1.8e-13

FD_STEP_INTR = 5e-4
N_USED = {0: 6, 1: 4, 2: 6, 3: 8}        # parameters a model reads; the rest of its block are never touched
NONLINEAR = {0: (4, 5), 1: (), 2: (4, 5), 3: ()}
LM_MIN_RELATIVE_DECREASE = 1e-3          # lm_policy.h: a step is accepted when cost change / model change exceeds it


# ---------------------------------------------------------------------------------------------- intrinsics Jacobian
def _central_intr(model, ip, pc, h_nl):
    """D(h) [O, 2, 8] of -project over the intrinsics of ONE model; h_nl the step of the non-linear parameters."""
    out = np.zeros(pc.shape[:-1] + (2, 8), LD)
    for k in range(N_USED[model]):
        h = LD(h_nl) if k in NONLINEAR[model] else LD(1)
        d = np.zeros(8, LD)
        d[k] = h
        out[..., k] = (-ba_ref.project(model, ip + d, pc) + ba_ref.project(model, ip - d, pc)) / (2 * h)
    return out


def intrinsics_jacobian(model, ip, pose, pw, h=FD_STEP_INTR):
    """model [O], ip [O, 8], pose [O, 7], pw [O, 3] -> G [O, 2, 8] = d (uv - projection) / d intrinsics and the
    step-halving disagreement per observation [O]."""
    ip, pc = _ld(ip), ba_ref.camera_point(pose, pw)
    model = np.broadcast_to(np.asarray(model), pc.shape[:-1])
    G, dis = np.zeros(pc.shape[:-1] + (2, 8), LD), np.zeros(pc.shape[:-1])
    for m in np.unique(model):
        k = model == m
        D = [_central_intr(int(m), ip[k], pc[k], LD(h) / s) for s in (1, 2, 4)]
        J, Jh = (4 * D[1] - D[0]) / 3, (4 * D[2] - D[1]) / 3
        G[k] = J
        dis[k] = (np.abs(J - Jh).max(axis=(-1, -2)) / np.abs(J).max(axis=(-1, -2))).astype(np.float64)
    return G, dis


def step_sweep(steps=(1e-4, 3e-4, 5e-4, 1e-3, 2e-3)):
    """step -> the largest step-halving disagreement of G over every case: what FD_STEP_INTR was chosen from."""
    out = {}
    for h in steps:
        worst = 0.0
        for p in cases().values():
            worst = max(worst, float(intrinsics_jacobian(p.obs_model(), _ld(p.intr)[p.cam_intr[p.obs_cam]], p.poses[p.obs_cam],
                                                         p.points[p.obs_lm], h)[1].max()))
        out[h] = worst
    return out


# ------------------------------------------------------------------------------------------------------ linearisation
def blocks(prob, poses=None, points=None, intr=None):
    """Raw r, F, E, G and the FD disagreement per observation (the larger of ba_ref's and G's)."""
    P = _ld(prob.poses if poses is None else poses)[prob.obs_cam]
    X = _ld(prob.points if points is None else points)[prob.obs_lm]
    ip = _ld(prob.intr if intr is None else intr).reshape(2, 8)[prob.cam_intr[prob.obs_cam]]
    r, F, E, dis = ba_ref.residual_jacobian(prob.obs_model(), ip, P, X, prob.obs_uv, prob.fd_step)
    G, disg = intrinsics_jacobian(prob.obs_model(), ip, P, X)
    return r, F, E, G, np.maximum(dis.astype(np.float64), disg)


def cost(prob, poses=None, points=None, intr=None):
    P = _ld(prob.poses if poses is None else poses)[prob.obs_cam]
    X = _ld(prob.points if points is None else points)[prob.obs_lm]
    ip = _ld(prob.intr if intr is None else intr).reshape(2, 8)[prob.cam_intr[prob.obs_cam]]
    r = ba_ref.residual(prob.obs_model(), ip, P, X, prob.obs_uv)
    z6, z3 = np.zeros(r.shape + (6,), LD), np.zeros(r.shape + (3,), LD)
    return float(np.sum(ba_ref.huber_correct(r, z6, z3, prob.use_huber, prob.huber)[3]))


class Lin:
    """One linearisation; long double unless named otherwise.  See linearize()."""


def reduce_system(H, b, Jc, r, D, damp, obs_lm, nt, L):
    """Eliminates the landmarks of the scaled, damped D H D + diag(damp), D b one by one.  Jc [O, 2, nt]: the camera-side
    rows [F | G] (Huber applied, unscaled), r [O, 2].  Returns S, g, A_S, A_g, kappa, Pinv {l: P_l^-1}, Hs, bs."""
    Hs, bs = D[:, None] * H * D[None, :] + np.diag(damp), D * b
    Ja = np.abs(Jc) * D[:nt][None, None, :]
    A_S = np.einsum("oki,okj->ij", Ja, Ja) + np.diag(damp[:nt])
    A_g = np.einsum("oki,ok->i", Ja, np.abs(r))
    S, g = Hs[:nt, :nt].copy(), bs[:nt].copy()
    kappa, Pinv = np.zeros(L), {}
    seen = np.bincount(obs_lm, minlength=L)
    for l in range(L):
        s = slice(nt + 3 * l, nt + 3 * l + 3)
        P, W, bl = Hs[s, s], Hs[:nt, s], bs[s]
        if not seen[l] and not np.any(P):
            continue
        Pi = Pinv[l] = _inv3(P)
        if not np.any(W):
            continue
        kappa[l] = np.linalg.cond(H[s, s].astype(np.float64))       # of the PLAIN block, whatever the variables
        S -= W @ Pi @ W.T
        g -= W @ Pi @ bl
        A_S += LD(kappa[l]) * (np.abs(W) @ np.abs(Pi) @ np.abs(W).T)
        A_g += LD(kappa[l]) * (np.abs(W) @ np.abs(Pi) @ np.abs(bl))
    return S, g, A_S, A_g, kappa, Pinv, Hs, bs


def assemble(prob, r, F, E, G):
    """Dense H, b and the camera-side rows Jc [O, 2, nt] from Huber-corrected blocks (any float type)."""
    nf, L, O = prob.n_free, len(prob.points), len(prob.obs_cam)
    n, nt = 6 * nf, 6 * nf + 16
    N = nt + 3 * L
    J = np.zeros((O, 2, N), r.dtype)
    fc = prob.free_index()[prob.obs_cam]
    for i in range(O):
        if fc[i] >= 0:
            J[i, :, 6 * fc[i]:6 * fc[i] + 6] = F[i]
        k = n + 8 * prob.cam_intr[prob.obs_cam[i]]
        J[i, :, k:k + 8] = G[i]
        l = nt + 3 * prob.obs_lm[i]
        J[i, :, l:l + 3] = E[i]
    J2 = J.reshape(2 * O, N)
    return J2.T @ J2, J2.T @ r.reshape(-1), J[:, :, :nt]


def linearize(prob, inv_radius=None):
    """inv_radius None: the plain system (no scaling, no damping).  A number: the system the solver factorises.  Fields:
    r, F, E, G (raw blocks), outlier, fd_disagreement, cost, H, b (before scaling), D, damp, Hs, bs, S, g, A_S, A_g, kappa,
    cond_S, and where the Cholesky of S succeeds d [nt], dl [L, 3] in the scaled variables (else None)."""
    out = Lin()
    L = len(prob.points)
    nt = 6 * prob.n_free + 16
    out.r, out.F, out.E, out.G, dis = blocks(prob)
    out.fd_disagreement = float(dis.max())
    r, F, E, c, out.outlier = ba_ref.huber_correct(out.r, out.F, out.E, prob.use_huber, prob.huber)
    k = np.sqrt(np.where(out.outlier, LD(prob.huber) / np.sqrt(np.where(out.outlier, np.sum(out.r * out.r, axis=-1), LD(1))), LD(1)))
    G = k[:, None, None] * out.G
    out.cost = float(np.sum(c))
    H, b, Jc = assemble(prob, r, F, E, G)
    out.H, out.b, out.rw, out.Jc = H, b, r, Jc
    N = len(b)
    D, damp = np.ones(N, LD), np.zeros(N, LD)
    if inv_radius is not None:
        D = 1 / (1 + np.sqrt(np.diag(H)))
        damp = np.clip(D * np.diag(H) * D, LD(1e-6), LD(1e32)) * LD(inv_radius)
    out.D, out.damp = D, damp
    out.S, out.g, out.A_S, out.A_g, out.kappa, Pinv, out.Hs, out.bs = reduce_system(H, b, Jc, r, D, damp, prob.obs_lm, nt, L)
    with np.errstate(all="ignore"):
        out.cond_S = float(np.linalg.cond(out.S.astype(np.float64)))
    out.d = out.dl = None
    if inv_radius is not None:
        x = _cholesky_solve(out.S, out.g)
        if x is not None:
            out.d = -x
            out.dl = np.zeros((L, 3), LD)
            for l, Pi in Pinv.items():
                s = slice(nt + 3 * l, nt + 3 * l + 3)
                out.dl[l] = -Pi @ (out.bs[s] + out.Hs[:nt, s].T @ out.d)
    return out


class Step:
    """One LM step of the reference; see lm_step()."""


def lm_step(prob, inv_radius=1e-4):
    """One Levenberg-Marquardt step: fields lin (the Lin), d, dl (scaled), step_c [n_free, 6], step_i [2, 8], step_l [L, 3]
    (unscaled), poses, intr, points (the candidates), cost, cand_cost, model_change, gain (= cost change / model change)
    and accepted (what lm_policy.h decides from them)."""
    R = linearize(prob, inv_radius)
    out = Step()
    out.lin = R
    n = 6 * prob.n_free
    nt = n + 16
    assert R.d is not None, prob.name
    out.d, out.dl = R.d, R.dl
    out.step_c = (R.D[:n] * R.d[:n]).reshape(-1, 6)
    out.step_i = (R.D[n:nt] * R.d[n:]).reshape(2, 8)
    out.step_l = R.D[nt:].reshape(-1, 3) * R.dl
    poses = _ld(prob.poses).copy()
    free = np.flatnonzero(prob.cam_fixed == 0)
    if len(free):
        new = se3_mul(poses[free], se3_exp(out.step_c))
        new[:, :4] /= np.sqrt(np.sum(new[:, :4] ** 2, axis=1, keepdims=True))
        poses[free] = new
    out.poses, out.intr, out.points = poses, _ld(prob.intr) + out.step_i, _ld(prob.points) + out.step_l
    out.cost, out.cand_cost = R.cost, cost(prob, out.poses, out.points, out.intr)
    # the model's decrease: -(m . (r + m / 2)) summed, m = J delta in the scaled variables (Huber-corrected rows)
    y = np.concatenate([R.d, R.dl.reshape(-1)])
    Js = np.zeros((len(prob.obs_cam), 2, len(y)), LD)
    Js[:, :, :nt] = R.Jc
    _, _, E, _, _ = ba_ref.huber_correct(R.r, R.F, R.E, prob.use_huber, prob.huber)
    for i in range(len(prob.obs_cam)):
        l = nt + 3 * prob.obs_lm[i]
        Js[i, :, l:l + 3] = E[i]
    m = (Js * R.D[None, None, :]) @ y
    out.model_change = float(-np.sum(m * (R.rw + m / 2)))
    out.gain = (out.cost - out.cand_cost) / out.model_change
    out.accepted = out.model_change > 0 and out.gain > LM_MIN_RELATIVE_DECREASE
    return out


# ----------------------------------------------------------------------------------------------------------- fixtures
def _perturb_intr(true, models, seed):
    """The true blocks with every parameter its model uses 1 to 2 % off (sign at random)."""
    rng = np.random.default_rng(seed)
    out = np.array(true, np.float64).reshape(2, 8).copy()
    for k in range(2):
        u = N_USED[models[k]]
        out[k, :u] *= 1 + rng.choice([-1, 1], u) * rng.uniform(0.01, 0.02, u)
    return out


def _observe(p, true_intr, noise, seed):
    """obs_uv = the long-double projection of the problem as it stands through true_intr + N(0, noise) px."""
    rng = np.random.default_rng(seed)
    keep = p.intr
    p.intr = np.array(true_intr, np.float64).reshape(2, 8)
    p.obs_uv = np.zeros((len(p.obs_cam), 2))
    p.obs_uv = (-p.blocks(jac=False) + _ld(noise * rng.normal(size=p.obs_uv.shape))).astype(np.float64)
    p.intr = keep


def scene(n_cams, n_fixed, n_lms, seed, models=(0, 0), cam_intr=None, window=None, noise=0.5, drift=0.01, drop=(), **kw):
    """ba_ref.scene_problem's geometry (cameras on an arc of radius 4 looking at a cloud round the origin; window: landmark
    l is seen by the fixed cameras and `window` consecutive free ones from free camera 2 l on, landmark 0 by all) with a
    model per intrinsics block, the assignment cam_intr (default c % 2) and intrinsics handed in 1 - 2 % off the ones the
    observations were made with.  drop: (camera, landmark) observations left out."""
    base = ba_ref.scene_problem(n_cams, n_fixed, n_lms, seed, model=models[0], noise=0.0, drift=0.0, window=window, **kw)
    rng = np.random.default_rng(seed + 7919)
    true = np.array([INTR[models[0]], INTR[models[1]]], np.float64)
    ci = np.arange(n_cams) % 2 if cam_intr is None else np.asarray(cam_intr)
    keep = np.ones(len(base.obs_cam), bool)
    for c, l in drop:
        keep &= ~((base.obs_cam == c) & (base.obs_lm == l))
    p = Problem(base.poses, base.cam_fixed, ci, true, base.points, base.obs_cam[keep], base.obs_lm[keep],
                np.zeros((int(keep.sum()), 2)), models, **kw)
    _observe(p, true, noise, seed + 1)
    d = drift * rng.normal(size=(n_cams, 6))
    d[p.cam_fixed != 0] = 0
    p.poses = se3_mul(_ld(p.poses), se3_exp(_ld(d))).astype(np.float64)
    p.poses[:, :4] /= np.linalg.norm(p.poses[:, :4], axis=1, keepdims=True)
    p.points = p.points + drift * rng.normal(size=p.points.shape)
    p.intr = _perturb_intr(true, models, seed + 2)
    return p


def pointed(model, specials, seed, n_lms=9, noise=0.5):
    """Camera 1 (free, block 1, the identity bit for bit) sees landmarks 0.. at `specials` in ITS frame, exactly; cameras
    0 (block 0) and 3 (block 1) are fixed, camera 2 (block 0) is free, all three stand 0.8 beside camera 1 and see every landmark too.
    The other landmarks lie 3 to 5 in front.  Both blocks have `model`.  Only cameras 0, 2, 3 and the ordinary landmarks are moved off the
    truth, so that the special camera-frame points stay what their names say."""
    rng = np.random.default_rng(seed)
    poses = np.array([np.concatenate([se3_exp(_ld([0, 0, 0, 0.01, -0.02, 0.015]))[:4].astype(np.float64), [-0.8, 0.1, 0.0]]),
                      IDENT,
                      np.concatenate([se3_exp(_ld([0, 0, 0, -0.015, 0.01, 0.02]))[:4].astype(np.float64), [0.7, -0.2, 0.05]]),
                      np.concatenate([se3_exp(_ld([0, 0, 0, 0.02, 0.015, -0.01]))[:4].astype(np.float64), [0.1, 0.8, -0.05]])])
    points = np.array([np.asarray(s, np.float64) for s in specials] +
                      [np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(3, 5)]) for _ in range(n_lms - len(specials))])
    oc, ol = np.tile(np.arange(4), n_lms), np.repeat(np.arange(n_lms), 4)
    true = np.array([INTR[model], INTR[model]], np.float64)
    p = Problem(poses, [1, 0, 0, 1], [0, 1, 0, 1], true, points, oc, ol, np.zeros((len(oc), 2)), (model, model))
    _observe(p, true, noise, seed + 1)
    d = 0.01 * rng.normal(size=(4, 6))
    d[[0, 1, 3]] = 0
    p.poses = se3_mul(_ld(p.poses), se3_exp(_ld(d))).astype(np.float64)
    p.poses[:, :4] /= np.linalg.norm(p.poses[:, :4], axis=1, keepdims=True)
    p.poses[1] = IDENT
    p.points[len(specials):] += 0.01 * rng.normal(size=(n_lms - len(specials), 3))
    p.intr = _perturb_intr(true, (model, model), seed + 2)
    p.special = [int(np.flatnonzero((oc == 1) & (ol == k))[0]) for k in range(len(specials))]
    return p


BASE = dict(n_cams=3, n_fixed=1)      # camera 0 (block 0) fixed, 1 (block 1) and 2 (block 0) free
FIX2 = dict(n_cams=4, n_fixed=2)      # cameras 0 (block 0) and 1 (block 1) fixed, 2 (block 0) and 3 (block 1) free


def _build_cases():
    T = {}
    # one per model and a mixed pair; a few observations missing so that the blocks are not uniform; 9 and 13 landmarks:
    # the last workgroup of bai_border_kernel (4 landmarks each) holds one
    drop = ((2, 1), (1, 6), (0, 7))
    T["a_base_ds"] = scene(n_lms=9, seed=700, models=(0, 0), drop=drop, **BASE)
    T["a_pinhole"] = scene(n_lms=13, seed=701, models=(1, 1), drop=drop, **BASE)
    T["a_eucm"] = scene(n_lms=9, seed=702, models=(2, 2), drop=drop, **BASE)
    T["a_kb4"] = scene(n_lms=13, seed=703, models=(3, 3), drop=drop, **BASE)
    T["a_models_0_3"] = scene(n_lms=9, seed=704, models=(0, 3), drop=drop, **BASE)
    # every camera on block 0: columns n + 8 .. n + 15 are zero (one fixed camera is enough here: the case is about the
    # structure of S, and its undamped system is singular by construction anyway)
    T["b_unobserved_block"] = scene(3, 1, 9, 705, cam_intr=[0, 0, 0], drop=((1, 3),))
    # block 1 is seen by the fixed camera 0 only: it lives in the border alone, no pose row meets it
    T["c_fixed_camera_border"] = scene(n_lms=9, seed=706, cam_intr=[1, 0, 0], drop=drop[:2], **BASE)
    # 4 cameras, 0 and 1 fixed: landmark 3 is seen by the two fixed cameras only: it contributes to S_ii and to nothing in the pose rows
    T["d_fixed_only_landmark"] = scene(n_lms=9, seed=707, drop=((2, 3), (3, 3)), **FIX2)
    # 4 cameras, 0 and 1 fixed: landmarks 0 .. 3 by the cameras of block 0 only (0 and 2), 4 .. 7 by those of block 1 only (1 and 3): two
    # observations each, W of the other block is zero
    T["e_single_block_landmarks"] = scene(n_lms=11, seed=708, **FIX2,
                                          drop=tuple((c, l) for l in range(4) for c in (1, 3)) + tuple((c, l) for l in range(4, 8) for c in (0, 2)))
    p = scene(n_lms=9, seed=709, drop=drop, **BASE)
    i0 = int(np.flatnonzero((p.obs_cam == 2) & (p.obs_lm == 4))[0])       # block 0
    i1 = int(np.flatnonzero((p.obs_cam == 1) & (p.obs_lm == 5))[0])       # block 1
    p.obs_uv[i0] += [31.0, -14.0]
    p.obs_uv[i1] += [-22.0, 28.0]
    p.outliers = (i0, i1)
    T["f_huber_outliers"] = p
    # KB4: exactly on the axis (r == 0: only cx, cy columns), r = 1e-9 z, 85 degrees; double sphere and EUCM at 60
    T["g_kb4_awkward"] = pointed(3, ([0, 0, 4.0], [4.0 * 0.6e-9, 4.0 * 0.8e-9, 4.0], _at_angle(85)), 710)
    T["g_kb4_awkward"].oracle = "not_special"
    T["g_ds_60"] = pointed(0, (_at_angle(60),), 711)
    T["g_eucm_60"] = pointed(2, (_at_angle(60),), 712)
    # 4 cameras, 255 / 256 / 257 observations: the last workgroup of the per-observation kernels is full less one, full,
    # and a second one holds a single observation
    T["h_tail_255"] = scene(4, 1, 64, 713, drop=((3, 63),))
    T["h_tail_256"] = scene(4, 1, 64, 714)
    T["h_tail_257"] = scene(4, 1, 65, 715, drop=((2, 62), (3, 63), (2, 64)))
    # 18 free cameras: nt = 124, the small dense kernel; 19: nt = 130, the general solver although n = 114 <= 128
    T["i_seam_18_free"] = scene(19, 1, 24, 716, window=4)
    T["i_seam_19_free"] = scene(20, 1, 24, 717, window=4)
    # every pose fixed: nt = 16, calibration against fixed poses
    T["j_no_free_camera"] = scene(3, 3, 9, 718, drop=drop[:2])
    for name, p in T.items():
        p.name = name
    return T


# the cases whose UNDAMPED reduced system is solvable (see the module docstring)
UNDAMPED_SOLVABLE = ("g_kb4_awkward",)

_CASES = None
_LIN = {}


def cases():
    """name -> Problem, built once (read-only; copy what a solve changes)."""
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


_STEP = {}


def reference_step(name, inv_radius=1e-4):
    if (name, inv_radius) not in _STEP:
        _STEP[(name, inv_radius)] = lm_step(cases()[name], inv_radius)
    return _STEP[(name, inv_radius)]


def solvable(R):
    """The step of a reference system is checked where 64 cond 2^-52 < 1e-3 and its Cholesky went through."""
    return R.d is not None and 64 * R.cond_S * U < 1e-3


def jac_tol(name):
    """Jacobian tolerance of a case, relative to the block's largest entry: ba_ref's rule on this file's constants."""
    return min(max(8.0 * ORACLE_VS_REF_JAC_INTR, 10.0 * reference(name).fd_disagreement), 1e-9)
