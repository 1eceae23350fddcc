"""CPU: pins tests/spd_ref.py -- the long-double reference, the generators, the coupling table that separates the old
matrices of test_chol_gpu.py from the chain matrices, the 50x margin of the reference over fp64 LAPACK, and the
model / LAPACK ratios that set the tolerance of tests/test_chol_edges_gpu.py.  No GPU; prints what it measures (-s)."""
import ctypes

import numpy as np
import pytest

import spd_ref as ref

LD = np.longdouble
needs_ld = pytest.mark.skipif(not ref.LD_OK, reason=ref.LD_SKIP_REASON)


@pytest.fixture(scope="module")
def measured():
    """Per case: eta and forward error of LAPACK and of the path's model, cond(S), the model's diagnostics."""
    out = {}
    for case in ref.cases():
        S, b = ref.build_case(case)
        n, cyc = case["n"], case["cyclic"]
        bw = n - 1 if case["path"] == "dense_panels" else case["bw_pass"]
        info = {}
        xm = ref.model_solve(case["path"], S, b, bw, info)
        xl = ref.lapack_solve(S, b, bw, cyc)
        m = dict(case=case, info=info, eta_model=ref.backward_error(S, xm, b, bw, cyc),
                 eta_lapack=ref.backward_error(S, xl, b, bw, cyc))
        if case["forward"] and ref.LD_OK:
            ld = {}
            x_ld = ref.solve_ld(S, b, bw, cyc, ld)
            ev = np.linalg.eigvalsh(S)
            m.update(cond=float(ev[-1] / ev[0]), corrections=ld["corrections"],
                     plain=ref.forward_error(ld["plain"], x_ld), eta_ld=ref.backward_error(S, x_ld, b, bw, cyc),
                     fwd_model=ref.forward_error(xm, x_ld), fwd_lapack=ref.forward_error(xl, x_ld))
        out[case["name"]] = m
    return out


def test_case_list_is_well_formed():
    cs = ref.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    assert {c["path"] for c in cs} == set(ref.PATHS)
    for p in ref.PATHS:   # one scaled variant per path, every delta on the list
        assert sum(1 for c in cs if c["path"] == p and c["decades"]) == 1, p
    assert {c["delta"] for c in cs} == {1e-3, 1e-6, 1e-8}
    lin = [c for c in cs if c["path"] == "bcr"]
    assert {c["block"] for c in lin} >= {32, 64, 96, 224, 256}
    assert {c["n_blocks"] for c in lin if c["block"] == 32} >= {8, 9, 15, 16, 17, 33}
    assert {c["n"] % 32 for c in lin if c["block"] == 32} >= {0, 1, 31}          # ragged last blocks of 1 and B - 1
    ring = [c for c in cs if c["path"] == "bcr_cyclic"]
    assert {c["block"] for c in ring} >= {32, 64, 96, 224, 256}
    assert {c["n_blocks"] for c in ring} >= {8, 9, 15, 16, 17, 33}
    big = [c for c in cs if c["n"] == 5988]
    assert len(big) == 1 and (big[0]["block"], big[0]["n_blocks"], big[0]["levels"]) == (224, 27, 5) and not big[0]["forward"]
    seps = {ref.two_ended_split(c["n"], c["bw_pass"])[2] - c["bw_pass"] for c in cs if c["path"] == "band_two_ended"}
    assert seps >= {0, 31}


def test_ring_layout_matches_the_library(vsl):
    lib = vsl.load()
    B, nb = ctypes.c_int(), ctypes.c_int()
    for c in ref.cases():
        if c["cyclic"]:
            assert lib.vsl_bcr_cyclic_layout(c["n"], c["bw_pass"], ctypes.byref(B), ctypes.byref(nb)) == 1
            assert (B.value, nb.value) == (c["block"], c["n_blocks"]), c["name"]
    for n, bw in [(600, 100), (5988, 83), (1040, 128), (7, 1)]:
        ok = lib.vsl_bcr_cyclic_layout(n, bw, ctypes.byref(B), ctypes.byref(nb))
        lay = ref.cyclic_layout(n, bw)
        assert (lay is None) == (ok == 0) and (lay is None or lay == (B.value, nb.value))


@pytest.mark.parametrize("n,bw,cyclic", [(300, 20, False), (257, 1, False), (97, 96, False), (256, 0, False), (300, 20, True),
                                         (64, 31, True), (40, 25, True)])
def test_generators_have_the_exact_bandwidth_and_the_constant_eigenvector(n, bw, cyclic):
    S = ref.chain_spd(n, bw, 5, 1e-6, cyclic)
    assert np.array_equal(S, S.T) and ref.half_bandwidth(S, cyclic) == min(bw, n // 2 if cyclic else n - 1)
    if bw:
        d = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
        d = np.minimum(d, n - d) if cyclic else d
        assert np.all(S[d == min(bw, d.max())] != 0.0)            # the outermost diagonal is full
    assert np.abs(S @ np.ones(n) - 1e-6).max() < 64 * ref.U64 * np.abs(S).sum(1).max()
    assert np.array_equal(S, ref.chain_spd(n, bw, 5, 1e-6, cyclic))
    D = ref.scaled(S, 6, 9)
    assert ref.half_bandwidth(D, cyclic) == ref.half_bandwidth(S, cyclic) and np.array_equal(D, D.T)
    assert np.array_equal(ref.truncate(S, bw, cyclic), S)


@needs_ld
@pytest.mark.parametrize("n,bw,cyclic", [(300, 20, False), (257, 1, False), (200, 0, False), (120, 119, False), (300, 20, True),
                                         (257, 1, True), (40, 25, True), (256, 0, True)])
def test_solve_ld_against_lapack_on_well_conditioned_systems(n, bw, cyclic):
    # delta = 1: cond <= 5.  fp64 Cholesky: ||dx|| / ||x|| <= ~ cond gamma_{bw + 2} (Higham, Accuracy and Stability,
    # theorem 10.4 with the band's row length in place of n); the reference's own error is 2048 times smaller
    S = ref.chain_spd(n, bw, 17, 1.0, cyclic)
    b = np.random.default_rng(3).standard_normal(n)
    ev = np.linalg.eigvalsh(S)
    x_ld = ref.solve_ld(S, b, bw, cyclic)
    assert x_ld.dtype == LD
    fwd = ref.forward_error(ref.lapack_solve(S, b, bw, cyclic), x_ld)
    print("n %d bw %d cyclic %d: cond %.2f, LAPACK - reference %.2e" % (n, bw, cyclic, ev[-1] / ev[0], fwd))
    assert fwd <= (ev[-1] / ev[0]) * (bw + 2) * ref.U64
    # its own backward error at long-double rounding level: gamma_{bw + 2} for the factorisation, twice for the two
    # substitutions, once for the residual product
    eta = ref.backward_error(S, x_ld, b, bw, cyclic)
    print("   eta of the reference %.2e" % eta)
    assert eta <= 4 * (bw + 2) * ref.EPS_LD


@needs_ld
def test_reference_backward_error_on_every_forward_case(measured):
    for name, m in measured.items():
        if "eta_ld" in m:
            bw = min(m["case"]["bw_pass"] if m["case"]["bw_pass"] >= 0 else m["case"]["n"], m["case"]["n"])
            assert m["eta_ld"] <= 4 * (bw + 2) * ref.EPS_LD, (name, m["eta_ld"])


def test_coupling_table():
    """The table of DESIGN.md ("SPD solver tests"): n = 2048, bw = 100."""
    n, bw = 2048, 100
    old, new = {}, {}
    S_old = ref.band_spd_dominant(n, bw, 5 * n + bw)
    ref.model_odd_even(S_old, np.zeros(n), bw, info=old, solve=False)
    S_new = ref.chain_spd(n, bw, 1, 1e-9)
    ref.model_odd_even(S_new, np.ones(n), bw, info=new)
    for tag, S, info in (("dominant", S_old, old), ("chain 1e-9", S_new, new)):
        ev = np.linalg.eigvalsh(S)
        f = ref.PanelFactor(S, bw)
        print("%-10s cond(S) %.2e  coupling per level %s  max cond(L_kk) %.3g" %
              (tag, ev[-1] / ev[0], " ".join("%.2e" % c for c in info["coupling"]), f.cond_diag))
        info["cond"], info["cond_l"] = ev[-1] / ev[0], f.cond_diag
    assert old["cond"] < 10 and old["cond_l"] < 2
    assert old["coupling"][0] < 0.5 and old["coupling"][3] < 1e-10     # below the old tolerance from the fourth level on
    assert new["cond"] > 1e9 and new["cond_l"] > 1e3
    assert len(new["coupling"]) == 4 and min(new["coupling"]) > 0.99


def test_chain_coupling_does_not_decay_on_any_reduction_case(measured):
    for name, m in measured.items():
        c = m["case"]
        if c["path"] not in ("bcr", "bcr_cyclic"):
            continue
        coup = m["info"]["coupling"]
        print("%-30s levels %d coupling %s  weakest pair %s" % (name, c["levels"], " ".join("%.3f" % v for v in coup),
                                                                " ".join("%.3f" % v for v in m["info"]["coupling_min"])))
        assert len(coup) == c["levels"] == m["info"]["levels"]
        if c["bw"] == 0:
            assert max(coup) == 0.0     # delta I: the one case that is about indexing only
            continue
        # EVERY neighbouring pair of every level stays coupled at 0.01 or more (measured: 0.045 at the least, mostly above
        # 0.6): a term dropped or misplaced at any pair changes the solution by about that relative amount, twelve orders
        # above the bound of the GPU test -- where the old matrices had 1e-13 from the fourth level on
        assert min(m["info"]["coupling_min"]) >= 0.01, name
        if c["n"] % c["block"] == 1 and not c["cyclic"]:
            # the last level joins block 0 with a last block of ONE unknown, which a wide band ties in weakly (0.049 at
            # B = 96; 0.04 .. 0.13 over other seeds); the levels before it keep their strongest pair above 0.9
            assert min(coup[:-1]) > 0.9, name
        else:
            assert min(coup) > 0.9, name


def test_band_paths_see_ill_conditioned_diagonal_factors(measured):
    # the old matrices never had cond(L_kk) above 1.25; every path meets at least 100 here
    worst = {}
    for name, m in measured.items():
        worst[m["case"]["path"]] = max(worst.get(m["case"]["path"], 1.0), m["info"]["cond_diag"])
    print("largest cond(L_kk) per path:", {k: "%.3g" % v for k, v in worst.items()})
    for p in ref.PATHS:
        assert worst[p] > 100, (p, worst[p])


@needs_ld
def test_refinement_converges_and_the_plain_solve_is_within_its_estimate(measured):
    # the premise of REF_ERROR: cond eps_ld < 1, the corrections contract by about that factor and end below eps_ld; and
    # the plain long-double solve differs from the refined one by no more than its own estimate cond eps_ld
    for name, m in measured.items():
        if "cond" not in m:
            continue
        c = m["corrections"]
        print("%-30s cond eps_ld %.1e  corrections %s  plain - refined %.1e" %
              (name, m["cond"] * ref.EPS_LD, " ".join("%.1e" % v for v in c), m["plain"]))
        assert m["cond"] * ref.EPS_LD < 1e-3
        assert c[-1] <= ref.EPS_LD and len(c) <= 4, (name, c)
        assert m["plain"] <= m["cond"] * ref.EPS_LD, name


@needs_ld
def test_reference_is_50x_more_accurate_than_lapack(measured):
    dropped, checked = [], 0
    for name, m in measured.items():
        if "cond" not in m:
            continue
        checked += 1
        margin = m["fwd_lapack"] / ref.REF_ERROR
        print("%-30s cond %.2e  reference ~%.1e  LAPACK %.2e  margin %.0f" % (name, m["cond"], ref.REF_ERROR, m["fwd_lapack"], margin))
        if margin < 50:
            dropped.append(name)
    print("dropped from the forward check:", dropped)
    assert sorted(dropped) == sorted(ref.FORWARD_DROPPED)
    assert checked == sum(1 for c in ref.cases() if c["forward"])
    assert len(dropped) * 10 <= checked      # at most one case in ten


@needs_ld
def test_model_over_lapack_ratios_are_pinned(measured):
    eta, fwd, worst = {}, {}, {}
    for name, m in measured.items():
        p = m["case"]["path"]
        r = m["eta_model"] / m["eta_lapack"]
        eta[p] = max(eta.get(p, 0.0), r)
        line = "%-30s eta model %.2e LAPACK %.2e (%.2f)" % (name, m["eta_model"], m["eta_lapack"], r)
        if "fwd_model" in m and name not in ref.FORWARD_DROPPED:
            rf = m["fwd_model"] / m["fwd_lapack"]
            fwd[p] = max(fwd.get(p, 0.0), rf)
            line += "  fwd model %.2e LAPACK %.2e (%.2f)  cond(S) %.1e" % (m["fwd_model"], m["fwd_lapack"], rf, m["cond"])
            if rf >= worst.get(p, (0.0,))[0]:
                worst[p] = (rf, name)
        print(line + "  cond(L_kk) %.3g" % m["info"]["cond_diag"])
    print("eta ratios", {k: round(v, 2) for k, v in eta.items()})
    print("fwd ratios", {k: round(v, 2) for k, v in fwd.items()}, worst)
    for p in ref.PATHS:
        # the constant is the measurement, rounded up by at most a quarter and capped (above the cap: a finding about the
        # design, recorded in DESIGN.md, not a tolerance)
        for const, got in ((ref.MODEL_VS_LAPACK_ETA[p], eta[p]), (ref.MODEL_VS_LAPACK_FWD[p], fwd[p])):
            want = min(max(got, 1.0), ref.RATIO_CAP)
            assert want <= const <= min(1.25 * want, ref.RATIO_CAP), (p, const, got)


@pytest.mark.parametrize("n,bw,cyclic", [(512, 31, False), (467, 20, False), (97, 48, False), (512, 31, True)])
def test_globally_indefinite_fails_only_as_a_whole(n, bw, cyclic):
    S = ref.globally_indefinite(n, bw, 7, cyclic)
    assert ref.half_bandwidth(S, cyclic) == bw
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(S)
    assert np.linalg.eigvalsh(S)[0] < -1e-10
    for k in range(1, n // 2 + 1):
        np.linalg.cholesky(S[:k, :k])            # raises if a leading block is not positive definite
    np.linalg.cholesky(S[n - n // 2:, n - n // 2:])  # the bottom chunk of the two-ended form likewise


def test_backward_error_reads_the_band_only():
    S = ref.chain_spd(200, 7, 3, 1e-3)
    x = np.random.default_rng(1).standard_normal(200)
    b = S @ x
    e0 = ref.backward_error(S, x, b, 7)
    assert e0 < 4 * ref.U64
    S2 = S.copy()
    S2[150, 20] = S2[20, 150] = 5.0
    assert ref.backward_error(S2, x, b, 7) == e0
    assert ref.backward_error(S2, x, b, 199) > 1e-3
    C = ref.chain_spd(200, 7, 3, 1e-3, cyclic=True)
    assert ref.backward_error(C, x, C @ x, 7, cyclic=True) < 4 * ref.U64 < 1e-3 < ref.backward_error(C, x, C @ x, 7)
