"""CPU: pins tests/ba_ref.py (the long-double reference of the bundle-adjustment linearisation) and measures the oracle
(oracle/orc_ba.cpp) against it on every case the GPU tests of test_ba_edges_gpu.py use.  The largest figures are printed
(`pytest -s`) and must not exceed the constants recorded in ba_ref.py, which the GPU tolerances are 8 x of."""
import numpy as np

import ba_ref as ref

LD = np.longdouble


def _arr(orc, p):
    return orc.BaArrays(p.poses, p.cam_fixed, p.cam_intr, p.intr, p.points, p.obs_cam, p.obs_lm, p.obs_uv, p.cam_model)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_constants_are_within_the_limits():
    assert ref.ORACLE_VS_REF_K <= 8 and ref.K_GPU == min(8 * ref.ORACLE_VS_REF_K, 64)
    assert ref.RES_GPU == min(8 * ref.ORACLE_VS_REF_RES, 1e-11)


def test_projection_against_known_values():
    # pinhole by hand; every model maps the axis to (cx, cy); KB4 with k = 0 is f * theta along the point's direction
    ip = np.array(ref.INTR[1])
    assert np.abs(ref.project(1, ip, np.array([1.0, 2.0, 4.0])) - [350 / 4 + 365, 348 * 2 / 4 + 249]).max() < 1e-16 * 500
    for m in range(4):
        assert np.array_equal(ref.project(m, np.array(ref.INTR[m]), np.array([0.0, 0.0, 2.5])), np.array([365, 249], LD))
    ip = np.array([350.0, 348.0, 365.0, 249.0, 0, 0, 0, 0])
    uv = ref.project(3, ip, np.array([3.0, 4.0, 5.0]))
    th = np.arctan2(LD(5), LD(5))
    assert np.abs(uv - [350 * th * LD(3) / 5 + 365, 348 * th * LD(4) / 5 + 249]).max() < 1e-15
    # double sphere with xi = 0, alpha = 0 and EUCM with alpha = 0 are the pinhole
    p = np.array([0.3, -0.2, 2.0])
    pin = ref.project(1, ip, p)
    assert np.abs(ref.project(0, ip, p) - pin).max() < 1e-16 and np.abs(ref.project(2, ip, p) - pin).max() < 1e-16


def test_finite_differences_against_the_pinhole_closed_form():
    rng = np.random.default_rng(0)
    p = ref.scene_problem(3, 1, 5, 1, model=1)
    r, F, E, dis = p.blocks()
    pc = ref.camera_point(p.poses[p.obs_cam], p.points[p.obs_lm])
    fx, fy = LD(350), LD(348)
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    J = np.zeros((len(x), 2, 3), LD)
    J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 2] = fx / z, -fx * x / z ** 2, fy / z, -fy * y / z ** 2
    assert np.abs(F[:, :, :3] - J).max() < 1e-12 * np.abs(J).max()      # r = uv - projection, d p_c / d upsilon = -I
    assert dis.max() < 1e-13 and rng is not None


def test_tables_hold_their_premises():
    C = ref.cases()
    for m, mn in ref.MODEL_NAMES.items():
        for kind, lo, hi in (("axis", 0.0, 0.0), ("ratio1e-12", 0.99e-12, 1.01e-12), ("ratio1e-8", 0.99e-8, 1.01e-8),
                             ("ratio1e-4", 0.99e-4, 1.01e-4)):
            p = C["obs/%s/%s" % (mn, kind)]
            pc = ref.camera_point(p.poses[p.obs_cam[p.special]], p.points[p.obs_lm[p.special]])
            assert lo <= float(np.hypot(pc[0], pc[1]) / pc[2]) <= hi, p.name
        for kind, depth in (("depth0.1", 0.1), ("depth1e3", 1e3)):
            p = C["obs/%s/%s" % (mn, kind)]
            pc = ref.camera_point(p.poses[p.obs_cam[p.special]], p.points[p.obs_lm[p.special]])
            assert float(pc[2]) == np.float64(depth) or abs(float(pc[2]) / depth - 1) < 1e-12
        for kind, deg in (("angle60", 60), ("angle85", 85), ("negz", 100)):
            name = "obs/%s/%s" % (mn, kind)
            assert (name in C) == (m != 1 if deg < 100 else m == 0)
            if name in C:
                p = C[name]
                pc = ref.camera_point(p.poses[p.obs_cam[p.special]], p.points[p.obs_lm[p.special]])
                assert abs(float(np.degrees(np.arctan2(np.hypot(pc[0], pc[1]), pc[2]))) - deg) < 1e-6
                assert (float(pc[2]) < 0) == (deg > 90)
        p = C["obs/%s/rot_identity" % mn]
        assert 0 < np.abs(p.poses[1, :3]).max() < 1e-8
        assert abs(C["obs/%s/rot_qw0" % mn].poses[1, 3]) < 1e-8
        p = C["obs/%s/far1e3" % mn]
        assert np.linalg.norm(p.poses[1, 4:]) > 999 and np.linalg.norm(p.points, axis=1).min() > 990
        p = C["obs/%s/pair1mm" % mn]
        assert 0.9e-3 < np.linalg.norm(p.poses[0, 4:] - p.poses[1, 4:]) < 1.1e-3
        assert ref.reference(p.name).kappa.max() > 1e8
    for on in ("on", "off"):
        p = C["huber/" + on]
        R = ref.reference(p.name)
        s = np.sum(R.r * R.r, axis=1)
        rows = p.rows
        assert np.array_equal(R.r[rows["at"]], np.array([3, 4], LD)) and s[rows["at"]] == 25 and not R.outlier[rows["at"]]
        assert s[rows["above"]] > 25 and s[rows["above"]] - 25 < 1e-12 and R.outlier[rows["above"]] == (on == "on")
        assert s[rows["below"]] < 25 and 25 - s[rows["below"]] < 1e-12 and not R.outlier[rows["below"]]
        assert not R.r[rows["zero"]].any() and s[rows["huge"]] == LD(1e12)
        # the same in double arithmetic, as the kernels see it: s > a^2 strictly one ulp above, not at, not below
        for row, want in (("at", False), ("above", True), ("below", False)):
            r64 = p.obs_uv[rows[row]] - np.array([365.0, 249.0])
            assert (r64[0] * r64[0] + r64[1] * r64[1] > 25.0) == want
    S = {k: v for k, v in C.items() if k.startswith("structure/")}
    assert [S["structure/n%d" % k].n_free for k in (1, 8, 16, 21, 22)] == [1, 8, 16, 21, 22]
    assert len(S["structure/one_landmark"].points) == 1
    p = S["structure/ragged_chunk"]
    assert len(p.obs_cam) == 96 and len(p.points) == 32      # one workgroup; 31 landmarks fill a chunk at n = 12
    p = S["structure/fixed_only_and_unobserved"]
    assert not (p.obs_lm == 7).any() and p.cam_fixed[p.obs_cam[p.obs_lm == 3]].all() and (p.obs_lm == 3).sum() == 2
    p = S["structure/observed_twice"]
    assert ((p.obs_lm == 4) & (p.obs_cam == 2)).sum() == 2
    assert np.bincount(S["structure/cams64"].obs_lm).max() == 64 and len(S["structure/cams65"].poses) == 65
    for p in C.values():       # every landmark that is observed at all has at least two observations
        assert not (np.bincount(p.obs_lm, minlength=len(p.points)) == 1).any(), p.name


def test_oracle_agrees_with_the_reference(orc):
    worst = {"K": (0.0, ""), "res": (0.0, ""), "jac": (0.0, ""), "cost": (0.0, ""), "fd": (0.0, "")}

    def note(key, value, where):
        if value > worst[key][0]:
            worst[key] = (float(value), where)

    by_table = {}
    for name, p in ref.cases().items():
        R = ref.reference(name)
        note("fd", R.fd_disagreement, name)
        # per case: the finite differences agree with themselves to a tenth of the case's Jacobian tolerance, and no
        # case's tolerance is looser than the recorded resolution allows
        assert R.fd_disagreement <= ref.jac_tol(name) / 10, name
        assert 8 * ref.ORACLE_VS_REF_JAC <= ref.jac_tol(name) <= max(8 * ref.ORACLE_VS_REF_JAC, 10 * ref.FD_RESOLUTION), name
        arr = _arr(orc, p)
        for i in range(len(p.obs_cam)):
            c, l = p.obs_cam[i], p.obs_lm[i]
            r, Jp, Jl = orc.ba_residual_jacobian(p.cam_model[p.cam_intr[c]], p.poses[c], p.points[l], p.intr[p.cam_intr[c]], p.obs_uv[i])
            if p.oracle == "none":
                continue
            note("res", np.abs(r - R.r[i]).max(), name)
            if p.oracle != "not_special" or i != p.special:
                note("jac", max(ref.block_error(Jp, R.F[i]), ref.block_error(Jl, R.E[i])), name)
        if p.oracle != "all":
            continue
        S, g, cost = orc.ba_linearize(arr, use_huber=p.use_huber, huber=p.huber)
        k = max(ref.ratio(S, R.S, R.A_S), ref.ratio(g, R.g, R.A_g))
        note("K", k, name)
        note("cost", abs(cost - R.cost) / (R.cost if R.cost > 0 else 1.0), name)
        t = name.split("/")[0]
        by_table[t] = max(by_table.get(t, 0.0), k)
    print("oracle vs long-double reference:")
    for key, const in (("K", ref.ORACLE_VS_REF_K), ("res", ref.ORACLE_VS_REF_RES), ("jac", ref.ORACLE_VS_REF_JAC),
                       ("cost", ref.ORACLE_VS_REF_COST)):
        print("  %-4s worst %.3g at %s (recorded constant %.3g)" % (key, worst[key][0], worst[key][1], const))
    print("  S, g ratio by table: " + ", ".join("%s %.3g" % kv for kv in sorted(by_table.items())))
    print("  finite-difference step halving: %.3g at %s (recorded %.3g; 8 x the Jacobian constant is %.3g)"
          % (worst["fd"][0], worst["fd"][1], ref.FD_RESOLUTION, 8 * ref.ORACLE_VS_REF_JAC))
    assert worst["fd"][0] <= ref.FD_RESOLUTION
    assert worst["K"][0] <= ref.ORACLE_VS_REF_K <= 8
    assert worst["res"][0] <= ref.ORACLE_VS_REF_RES and worst["jac"][0] <= ref.ORACLE_VS_REF_JAC
    assert worst["cost"][0] <= ref.ORACLE_VS_REF_COST


def test_fused_form_of_the_reference():
    # at inv_radius = 0 the scaled system is D S D / D g of the plain one; damping only adds to the diagonal
    name = "structure/n8"
    A, B, Cc = ref.reference(name), ref.reference(name, 0.0), ref.reference(name, 1e-4)
    nc = 48
    D = B.D[:nc]
    assert np.abs(B.S - D[:, None] * A.S * D[None, :]).max() <= 1e-17 * np.abs(B.S).max()
    assert np.abs(B.g - D * A.g).max() <= 1e-17 * np.abs(B.g).max()
    assert np.all(np.diag(Cc.S) > np.diag(B.S)) and np.abs(Cc.S @ Cc.dc + Cc.g).max() < 1e-15 * np.abs(Cc.g).max()
    # the step solves the full damped system, not only the reduced one
    y = np.concatenate([Cc.dc, Cc.dl.reshape(-1)])
    assert np.abs(Cc.Hs @ y + Cc.bs).max() < 1e-14 * np.abs(Cc.bs).max()


def test_one_step_of_the_reference_lowers_the_cost():
    poses, points, step_c, step_l, c0, c1, _ = ref.lm_step(ref.cases()["structure/n8"])
    assert c1 < 0.5 * c0 and np.abs(step_c).max() > 1e-4
