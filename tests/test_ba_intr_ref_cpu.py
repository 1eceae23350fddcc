"""CPU: pins tests/ba_intr_ref.py (the long-double reference of bundle adjustment with free intrinsics) and measures the
oracle (oracle/orc_ba.cpp: dual-number Jacobians, blocks assembled and reduced here in float64 numpy) against it on every
case the GPU tests of test_ba_intr_edges_gpu.py use.  The largest figures are printed (`pytest -s`) and must not exceed
the constants recorded in ba_intr_ref.py, from which the device allowances are derived by ba_ref.py's rules."""
import numpy as np

import ba_intr_ref as ref
import ba_ref

LD = np.longdouble
U = ref.U


def test_constants_follow_the_rules():
    assert ref.K_INTR_GPU == min(8 * ref.ORACLE_VS_REF_K_INTR, 64)
    for name in ref.cases():
        R = ref.reference(name)
        assert ref.jac_tol(name) == min(max(8 * ref.ORACLE_VS_REF_JAC_INTR, 10 * R.fd_disagreement), 1e-9)
        assert R.fd_disagreement <= ref.FD_RESOLUTION_INTR, name


def test_step_sweep_of_the_nonlinear_parameters():
    sweep = ref.step_sweep()
    print("finite-difference step of xi / alpha / beta -> worst step-halving disagreement of G over the table:")
    for h, v in sweep.items():
        print("  h = %-7g %.3g%s" % (h, v, "   <- FD_STEP_INTR" if h == ref.FD_STEP_INTR else ""))
    assert ref.FD_STEP_INTR in sweep and sweep[ref.FD_STEP_INTR] == min(sweep.values())


def test_intrinsics_jacobian_against_closed_forms():
    # pinhole: d u / d fx = x / z, d u / d cx = 1 (G is of the RESIDUAL: the signs flip); unused columns exactly zero
    p = ref.cases()["a_pinhole"]
    R = ref.reference(p.name)
    pc = ba_ref.camera_point(p.poses[p.obs_cam], p.points[p.obs_lm])
    want = np.zeros_like(R.G)
    want[:, 0, 0], want[:, 1, 1] = -pc[:, 0] / pc[:, 2], -pc[:, 1] / pc[:, 2]
    want[:, 0, 2] = want[:, 1, 3] = -1
    assert np.abs(R.G - want).max() < 5e-17      # (linear columns: exact but for the rounding of the projection)
    assert not R.G[:, :, 4:].any()
    for name, p in ref.cases().items():
        G = ref.reference(name).G
        for i in range(len(p.obs_cam)):
            assert not G[i, :, ref.N_USED[p.cam_model[p.cam_intr[p.obs_cam[i]]]]:].any()
    # KB4 with the point on the axis: -1 in cx / cy, nothing else, exactly
    p = ref.cases()["g_kb4_awkward"]
    want = np.zeros((2, 8), LD)
    want[0, 2] = want[1, 3] = -1
    assert np.array_equal(ref.reference(p.name).G[p.special[0]], want)


def test_table_holds_its_premises():
    C = ref.cases()
    for name, p in C.items():
        assert np.bincount(p.obs_lm, minlength=len(p.points)).min() >= 2, name
        assert np.abs(p.intr / np.where(p.intr != 0, [ba_ref.INTR[m] for m in p.cam_model], 1) - 1)[p.intr != 0].max() <= 0.02 + 1e-12
        if name[0] in "abcf":
            assert len(p.poses) == 3 and list(p.cam_fixed) == [1, 0, 0] and 9 <= len(p.points) <= 13, name
    assert [C[k].cam_model for k in ("a_base_ds", "a_pinhole", "a_eucm", "a_kb4", "a_models_0_3")] == [(0, 0), (1, 1), (2, 2), (3, 3), (0, 3)]
    assert not C["b_unobserved_block"].cam_intr.any()
    p = C["c_fixed_camera_border"]
    assert list(np.flatnonzero(p.cam_intr == 1)) == [0] and p.cam_fixed[0] and (p.obs_cam == 0).any()
    p = C["d_fixed_only_landmark"]
    assert p.cam_fixed[p.obs_cam[p.obs_lm == 3]].all() and (p.obs_lm == 3).sum() == 2
    p = C["e_single_block_landmarks"]
    for l in range(8):
        assert (p.obs_lm == l).sum() == 2 and len(set(p.cam_intr[p.obs_cam[p.obs_lm == l]])) == 1
    assert {int(p.cam_intr[p.obs_cam[p.obs_lm == l]][0]) for l in range(8)} == {0, 1}
    p = C["f_huber_outliers"]
    R = ref.reference(p.name)
    norms = np.sqrt(np.sum(R.r * R.r, axis=1).astype(np.float64))
    assert all(30 <= norms[i] <= 40 and R.outlier[i] for i in p.outliers), norms[list(p.outliers)]
    assert sorted(p.cam_intr[p.obs_cam[list(p.outliers)]]) == [0, 1]
    p = C["g_kb4_awkward"]
    pc = ba_ref.camera_point(p.poses[p.obs_cam[p.special]], p.points[p.obs_lm[p.special]])
    rz = (np.hypot(pc[:, 0], pc[:, 1]) / pc[:, 2]).astype(np.float64)
    assert rz[0] == 0.0 and abs(rz[1] / 1e-9 - 1) < 1e-12 and abs(np.degrees(np.arctan(rz[2])) - 85) < 1e-9
    for name in ("g_ds_60", "g_eucm_60"):
        p = C[name]
        pc = ba_ref.camera_point(p.poses[p.obs_cam[p.special[0]]], p.points[p.obs_lm[p.special[0]]])
        assert abs(float(np.degrees(np.arctan2(np.hypot(pc[0], pc[1]), pc[2]))) - 60) < 1e-9
    assert [len(C["h_tail_%d" % k].obs_cam) for k in (255, 256, 257)] == [255, 256, 257]
    assert all(len(C["h_tail_%d" % k].poses) == 4 for k in (255, 256, 257))
    assert {len(C[k].points) % 4 for k in ("a_base_ds", "a_pinhole")} == {1} and len(C["a_base_ds"].points) == 9 and len(C["a_pinhole"].points) == 13
    assert 6 * C["i_seam_18_free"].n_free + 16 == 124 and 6 * C["i_seam_19_free"].n_free + 16 == 130 and len(C["i_seam_19_free"].points) == 24
    assert C["j_no_free_camera"].n_free == 0
    assert max(len(p.poses) for p in C.values()) == len(C["i_seam_19_free"].poses)


def test_solvability_and_gain_of_the_table():
    skipped = []
    for name in ref.cases():
        R0, s = ref.reference(name, 0.0), ref.reference_step(name, 1e-4)
        assert ref.solvable(s.lin), (name, s.lin.cond_S)              # every case at 1 / radius = 1e-4
        assert ref.solvable(R0) == (name in ref.UNDAMPED_SOLVABLE), (name, R0.cond_S)
        if not ref.solvable(R0):
            skipped.append(name)
        assert abs(s.gain - ref.LM_MIN_RELATIVE_DECREASE) > 1e-6, (name, s.gain)
        print("%-26s cond_S %.3g (1 / radius 1e-4), %.3g (0); gain %.4f -> %s" % (name, s.lin.cond_S, R0.cond_S, s.gain,
                                                                                 "accepted" if s.accepted else "rejected"))
    print("undamped step not compared (singular by construction): " + ", ".join(skipped))
    # the unobserved block: zero columns, the damping alone on the diagonal
    p = ref.cases()["b_unobserved_block"]
    n = 6 * p.n_free
    R = ref.reference(p.name, 1e-4)
    assert not R.H[n + 8:n + 16].any() and np.all(R.D[n + 8:n + 16] == 1)
    S = R.S.copy()
    assert np.all(np.diag(S)[n + 8:n + 16] == LD(1e-6) * LD(1e-4))
    S[np.arange(n + 8, n + 16), np.arange(n + 8, n + 16)] = 0
    assert not S[n + 8:].any() and not S[:, n + 8:].any()
    assert {ref.reference_step(k).accepted for k in ref.cases()} == {True, False}    # both verdicts are in the table


def _oracle_system(orc, p):
    """The oracle's per-observation blocks, Huber-corrected, assembled and reduced in float64; and its raw G."""
    O = len(p.obs_cam)
    r, F, E, G = np.zeros((O, 2)), np.zeros((O, 2, 6)), np.zeros((O, 2, 3)), np.zeros((O, 2, 8))
    for i in range(O):
        c, l = p.obs_cam[i], p.obs_lm[i]
        k = p.cam_intr[c]
        r[i], F[i], E[i] = orc.ba_residual_jacobian(p.cam_model[k], p.poses[c], p.points[l], p.intr[k], p.obs_uv[i])
        G[i] = orc.ba_residual_jacobian_intr(p.cam_model[k], p.poses[c], p.points[l], p.intr[k], p.obs_uv[i])
    raw_G = G.copy()
    if p.use_huber:
        s = np.sum(r * r, axis=1)
        k = np.where(s > p.huber ** 2, np.sqrt(p.huber / np.sqrt(np.where(s > 0, s, 1.0))), 1.0)
        r, F, E, G = k[:, None] * r, k[:, None, None] * F, k[:, None, None] * E, k[:, None, None] * G
    H, b, _ = ref.assemble(p, r, F, E, G)
    nt = 6 * p.n_free + 16
    S, g = H[:nt, :nt].copy(), b[:nt].copy()
    for l in range(len(p.points)):
        s = slice(nt + 3 * l, nt + 3 * l + 3)
        WP = H[:nt, s] @ np.linalg.inv(H[s, s])
        S -= WP @ H[:nt, s].T
        g -= WP @ b[s]
    return raw_G, S, g


def test_oracle_agrees_with_the_reference(orc):
    worst = {"K": (0.0, ""), "jac": (0.0, ""), "fd": (0.0, "")}

    def note(key, value, where):
        if value > worst[key][0]:
            worst[key] = (float(value), where)

    for name, p in ref.cases().items():
        R = ref.reference(name)
        note("fd", R.fd_disagreement, name)
        G, S, g = _oracle_system(orc, p)
        keep = np.ones(len(p.obs_cam), bool)
        if p.oracle == "not_special":
            keep[p.special[0]] = False          # the KB4 point on the axis: the dual numbers are not finite there
        assert np.isfinite(G[keep]).all(), name
        note("jac", ref.block_error(G[keep], R.G[keep]).max(), name)
        if p.oracle != "all":
            continue
        note("K", max(ref.ratio(S, R.S, R.A_S), ref.ratio(g, R.g, R.A_g)), name)
    print("oracle vs long-double reference (intrinsics):")
    print("  S, g  worst %.3g units of 2^-52 A at %s (recorded constant %.3g; the device gets %.3g)"
          % (worst["K"][0], worst["K"][1], ref.ORACLE_VS_REF_K_INTR, ref.K_INTR_GPU))
    print("  G     worst %.3g at %s (recorded constant %.3g)" % (worst["jac"][0], worst["jac"][1], ref.ORACLE_VS_REF_JAC_INTR))
    print("  finite-difference step halving: %.3g at %s (recorded %.3g)" % (worst["fd"][0], worst["fd"][1], ref.FD_RESOLUTION_INTR))
    assert worst["K"][0] <= ref.ORACLE_VS_REF_K_INTR
    assert worst["jac"][0] <= ref.ORACLE_VS_REF_JAC_INTR
    assert worst["fd"][0] <= ref.FD_RESOLUTION_INTR


def test_reference_against_itself():
    # the pose block of the bordered system is ba_ref's reduced camera system of the same problem
    for name in ("a_base_ds", "d_fixed_only_landmark", "a_models_0_3"):
        p = ref.cases()[name]
        A, B = ref.reference(name), ba_ref.linearize(p)
        n = 6 * p.n_free
        assert np.abs(A.S[:n, :n] - B.S).max() <= 1e-17 * np.abs(B.S).max(), name
        assert np.abs(A.g[:n] - B.g).max() <= 1e-17 * np.abs(B.g).max(), name
        assert abs(A.cost - B.cost) <= 1e-15 * B.cost
    # at 1 / radius = 0 the scaled system is D S D / D g of the plain one, and the step solves the FULL damped system
    A, B, s = ref.reference("a_kb4"), ref.reference("a_kb4", 0.0), ref.reference_step("a_kb4", 1e-4)
    nt = len(A.g)
    D = B.D[:nt]
    assert np.abs(B.S - D[:, None] * A.S * D[None, :]).max() <= 1e-16 * np.abs(B.S).max()
    assert np.abs(B.g - D * A.g).max() <= 1e-16 * np.abs(B.g).max()
    y = np.concatenate([s.d, s.dl.reshape(-1)])
    assert np.abs(s.lin.Hs @ y + s.lin.bs).max() < 1e-13 * np.abs(s.lin.bs).max()
    assert s.model_change > 0


def test_one_step_of_the_reference_lowers_the_cost():
    s = ref.reference_step("a_base_ds", 1e-4)
    assert s.cand_cost < 0.5 * s.cost and s.accepted and np.abs(s.step_i).max() > 1e-3
