"""The host half of the bundle adjustment's set-up (visual-slam_amd/csrc/ba_host_plan.h, chol_layout.h), compiled with
g++ as plain C++ without HIP headers and driven by tests/cpp/ba_host_plan_test.cpp.  Every expected value is written out
by hand from the rules or computed here with numpy, never taken from the code under test.

The layout rule, for n = 6 free cameras unknowns: band forms only for n > 128; bw = 6 half + 5; B_lin = ceil((bw + 1) / 32) 32;
cyclic iff a ring layout exists (>= 8 blocks of >= bw_cyc + 1 and <= B <= 256 unknowns, B a multiple of 32) and
4 B_cyc <= 3 B_lin; else linear iff 2 (bw + 32 + 1) < n; s_elems = n (ld + 1) + 64 in band form (ld = bw + 32), n n dense."""
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = ROOT / "visual-slam_amd" / "csrc"
LIMITS = (22, 24, 512, 256)  # SCH_CMAX, SCH_KMAX, BL_THREADS, BL_LMW


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ba_host_plan") / "ba_host_plan_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", "-I", str(CSRC),
                    str(ROOT / "tests" / "cpp" / "ba_host_plan_test.cpp"), "-o", str(exe)], check=True)

    def go(text, timeout=20):
        """-> {first word of a line: [its integers]}, "case" lines collected under "cases" """
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        out = {"cases": []}
        for ln in r.stdout.splitlines():
            w = ln.split()
            if w[0] == "layout":
                out["layout"] = {w[i]: int(w[i + 1]) for i in range(1, len(w), 2)}
            elif w[0] == "case":
                out["cases"].append({w[i]: int(w[i + 1]) for i in range(1, len(w), 2)})
            elif w[0] == "sum":
                out["sum " + w[1]] = int(w[2])
            elif w[0] == "uv_err":
                out["uv_err"] = float(w[1])
            else:
                out[w[0]] = [int(x) for x in w[1:]]
        return out

    return go


def problem_text(fixed, obs):
    return " ".join(map(str, fixed)) + "\n" + "".join("%d %d\n" % o for o in obs)


def plan(run, fixed, n_lms, obs, allow_band=0, limits=LIMITS):
    return run("plan %d %d %d %d %d %d %d %d\n" % ((allow_band, len(fixed), n_lms, len(obs)) + tuple(limits)) + problem_text(fixed, obs))


def band(run, fixed, n_lms, obs):
    return run("band %d %d %d\n" % (len(fixed), n_lms, len(obs)) + problem_text(fixed, obs))


def layout(run, n, half_lin, half_cyc, allow_band=1, force_dense=0, no_cyclic=0, schur_atomics=0, chol_no_bcr=0, chol_no_fused=0):
    return run("layout %d %d %d %d %d %d %d %d %d\n" % (n, half_lin, half_cyc, allow_band, force_dense, no_cyclic, schur_atomics,
                                                         chol_no_bcr, chol_no_fused))["layout"]


def dense(n):
    return dict(banded=0, cyclic=0, renumber=0, bw=n, ldS=n, offS=0, s_elems=n * n)


def banded(n, bw, cyclic):
    return dict(banded=1, cyclic=cyclic, renumber=1 - cyclic, bw=bw, ldS=bw + 32, offS=bw + 32, s_elems=n * (bw + 33) + 64)


def half_of(order, edges):
    """max |position difference| over the edges, order[position] = node"""
    pos = {v: k for k, v in enumerate(order)}
    return max(abs(pos[a] - pos[b]) for a, b in edges)


def test_limits_are_the_kernels(run):
    ba = (CSRC / "ba.hip").read_text()
    bl = (CSRC / "ba_large.h").read_text()
    got = tuple(int(re.search(r"#define %s (\d+)" % name, src).group(1))
                for name, src in (("SCH_CMAX", ba), ("SCH_KMAX", ba), ("BL_THREADS", bl), ("BL_LMW", bl)))
    assert got == LIMITS


# ------------------------------------------------------------------------------------------------ the arrays
TINY_FIXED = [1, 0, 0, 0]
TINY_OBS = [(2, 1), (0, 0), (1, 2), (1, 0), (3, 1), (0, 2), (3, 0)]  # (camera, landmark) in the caller's order


def test_tiny_unsorted_problem(run):
    # landmark 0 <- observations 1, 3, 6; landmark 1 <- 0, 4; landmark 2 <- 2, 5 (the caller's order inside a landmark)
    p = plan(run, TINY_FIXED, 3, TINY_OBS)
    assert p["cam_free"] == [-1, 0, 1, 2] and p["free_cams"] == [1, 2, 3] and p["nfree"] == [3]
    assert p["lm_start"] == [0, 3, 5, 7]
    assert p["perm"] == [1, 3, 6, 0, 4, 2, 5]
    assert p["own_pointers"] == [0]
    assert p["obs_cam"] == [0, 1, 3, 2, 3, 1, 0]
    assert p["obs_lm"] == [0, 0, 0, 1, 1, 2, 2]
    assert p["obs_u"] == [1, 3, 6, 0, 4, 2, 5]  # the pixels travel with their observations
    # camera 0 <- sorted positions 0, 6; camera 1 <- 1, 5; camera 2 <- 3; camera 3 <- 2, 4
    assert p["cam_start"] == [0, 2, 4, 5, 7]
    assert p["cam_obs"] == [0, 6, 1, 5, 3, 2, 4]
    assert p["cam_pos"] == [0, 2, 5, 4, 6, 3, 1]
    # free-camera observations per landmark: 2 (cameras 1, 3), 2 (cameras 2, 3), 1 (camera 1): 4 + 4 + 1 pairs
    assert p["kmax_free"] == [2] and p["n_pairs"] == [9] and p["small"] == [1]
    assert p["wg_lm"] == [] and p["n_wg"] == [0]
    assert p["layout"] == dict(banded=0, cyclic=0, renumber=0, bw=18, ldS=18, offS=0, s_elems=324)


def test_tiny_problem_presorted_keeps_the_callers_arrays(run):
    obs = [TINY_OBS[i] for i in [1, 3, 6, 0, 4, 2, 5]]
    p = plan(run, TINY_FIXED, 3, obs)
    assert p["perm"] == [] and p["own_pointers"] == [1]
    assert p["obs_cam"] == [0, 1, 3, 2, 3, 1, 0] and p["obs_u"] == list(range(7))
    assert p["lm_start"] == [0, 3, 5, 7] and p["cam_start"] == [0, 2, 4, 5, 7]
    assert p["cam_obs"] == [0, 6, 1, 5, 3, 2, 4] and p["cam_pos"] == [0, 2, 5, 4, 6, 3, 1]
    assert p["kmax_free"] == [2] and p["n_pairs"] == [9] and p["small"] == [1]


# ------------------------------------------------------------------------------------------------ band order
def chain_obs(sigma):
    """landmark j seen by the cameras sigma[j] and sigma[j + 1]"""
    return [(sigma[j + d], j) for j in range(len(sigma) - 1) for d in (0, 1)]


def test_chain_orders_into_half_bandwidth_one(run):
    b = band(run, [0] * 30, 29, chain_obs(list(range(30))))
    assert sorted(b["order"]) == list(range(30))
    assert b["half_lin"] == [1] and b["half_cyc"] == [1]
    assert half_of(b["order"], [(j, j + 1) for j in range(29)]) == 1


def test_scrambled_chain_is_restored_by_free_cams(run):
    sigma = [int(v) for v in np.random.default_rng(5).permutation(30)]
    edges = [(sigma[j], sigma[j + 1]) for j in range(29)]
    p = plan(run, [0] * 30, 29, chain_obs(sigma), allow_band=1)
    # n = 180, half 1: bw = 11, 2 (11 + 33) = 88 < 180: linear band (no ring of 8 blocks narrower than 3/4 of B_lin = 32)
    assert p["half_lin"] == [1]
    assert p["layout"] == banded(180, 11, cyclic=0)
    free_cams, cam_free = p["free_cams"], p["cam_free"]
    assert sorted(free_cams) == list(range(30))
    assert [cam_free[c] for c in free_cams] == list(range(30))  # cam_free is the inverse
    assert max(abs(cam_free[a] - cam_free[b]) for a, b in edges) == 1
    assert p["small"] == [0]


def test_half_is_the_largest_position_difference_on_a_random_graph(run):
    rng = np.random.default_rng(11)
    C, L = 41, 70
    fixed = [1 if c in (3, 17) else 0 for c in range(C)]
    obs = [(int(c), l) for l in range(L) for c in rng.choice(C, size=3, replace=False)]
    obs = [obs[i] for i in rng.permutation(len(obs))]
    free = [c for c in range(C) if not fixed[c]]
    idx = {c: k for k, c in enumerate(free)}
    edges = set()
    for l in range(L):
        cams = [idx[c] for c, ll in obs if ll == l and c in idx]
        edges |= {(a, b) for a in cams for b in cams if a != b}
    b = band(run, fixed, L, obs)
    assert sorted(b["order"]) == list(range(len(free)))
    assert b["half_lin"] == [half_of(b["order"], edges)]
    assert b["half_cyc"] == [max(min(abs(a - c), len(free) - abs(a - c)) for a, c in edges)]


def test_ring_of_four_consecutive_cameras_has_cyclic_half_three(run):
    C = 40
    obs = [((j + d) % C, j) for j in range(C) for d in range(4)]
    edges = {((j + d) % C, (j + e) % C) for j in range(C) for d in range(4) for e in range(4) if d != e}
    b = band(run, [0] * C, C, obs)
    assert b["half_cyc"] == [3]
    assert b["half_lin"] == [half_of(b["order"], edges)]


# ------------------------------------------------------------------------------------------------ layout rule
def test_cyclic_block_layout(run):
    # bw = 31: blocks of >= 32 unknowns; 8 blocks need n >= 256, and B = 32 holds 256 / 8
    assert run("cyclic 256 31\n")["1"] == [32, 8]
    assert run("cyclic 255 31\n")["0"] == [0, 0]  # at most 7 blocks of >= 32
    # bw = 256 needs B = 288 > BCR_MAXB = 256, however many unknowns
    assert run("cyclic 100000 256\n")["0"] == [0, 0]
    # 1000 cameras, 18 around the ring: bw = 113, at most 6000 // 114 = 52 blocks; B = 128 needs ceil(6000 / 128) = 47
    assert run("cyclic 6000 113\n")["1"] == [128, 47]
    # B = 96 would need 63 blocks of >= 96: only 62 fit, so B = 128
    assert run("cyclic 6000 95\n")["1"] == [128, 47]


def test_dense_up_to_128_unknowns(run):
    assert layout(run, 126, 1, 1) == dense(126)
    assert layout(run, 128, 1, 1) == dense(128)
    # 132 unknowns, half 1: bw = 11, 2 (11 + 33) = 88 < 132: band.  Ring: B_cyc = 32 (8 blocks <= 132 // 12), 4 * 32 > 3 * 32
    assert layout(run, 132, 1, 1) == banded(132, 11, cyclic=0)
    assert banded(132, 11, cyclic=0)["s_elems"] == 132 * 44 + 64 == 5872


def test_linear_band_only_when_it_holds_less_than_half(run):
    # half 8: bw = 53, 2 (53 + 33) = 172
    assert layout(run, 174, 8, 8, no_cyclic=1) == banded(174, 53, cyclic=0)
    assert banded(174, 53, cyclic=0) == dict(banded=1, cyclic=0, renumber=1, bw=53, ldS=85, offS=85, s_elems=174 * 86 + 64)
    assert layout(run, 168, 8, 8, no_cyclic=1) == dense(168)
    assert layout(run, 168, 8, 8) == dense(168)  # (and 168 unknowns hold no ring of 8 blocks of >= 54)


def test_cyclic_taken_and_refused_at_the_three_quarters(run):
    # 1000 cameras: 36 in the best line (bw = 221, B_lin = 224), 18 around the ring (bw = 113, B_cyc = 128): 512 <= 672
    want = dict(banded=1, cyclic=1, renumber=0, bw=113, ldS=145, offS=145, s_elems=6000 * 146 + 64)
    assert layout(run, 6000, 36, 18) == want == banded(6000, 113, cyclic=1)
    # ring half 14: bw = 89, B_cyc = 96 (63 blocks <= 6000 // 90); line half 20: bw = 125, B_lin = 128: 384 <= 384
    assert layout(run, 6000, 20, 14) == banded(6000, 89, cyclic=1)
    # line half 15: bw = 95, B_lin = 96: 384 > 288, so the linear band: 2 (95 + 33) < 6000
    assert layout(run, 6000, 15, 14) == banded(6000, 95, cyclic=0)
    assert banded(6000, 95, cyclic=0)["s_elems"] == 6000 * 128 + 64


@pytest.mark.parametrize("switch", ["no_cyclic", "schur_atomics", "chol_no_bcr", "chol_no_fused"])
def test_each_switch_refuses_the_cyclic_form(run, switch):
    assert layout(run, 6000, 36, 18, **{switch: 1}) == banded(6000, 221, cyclic=0)
    assert banded(6000, 221, cyclic=0)["s_elems"] == 6000 * 254 + 64


def test_dense_when_forced_or_not_allowed(run):
    assert layout(run, 6000, 36, 18, force_dense=1) == dense(6000)
    assert layout(run, 6000, 36, 18, allow_band=0) == dense(6000)


# ---------------------------------------------------------------------------------------------- landmark runs
def runs(run, counts):
    """23 free cameras (not small), landmark l with counts[l] observations"""
    obs = [((l + k) % 23, l) for l, n in enumerate(counts) for k in range(n)]
    p = plan(run, [0] * 23, len(counts), obs)
    assert p["small"] == [0]
    assert p["n_wg"] == [max(0, len(p["wg_lm"]) - 1)]
    return p["wg_lm"]


def test_a_run_closes_at_bl_threads_observations(run):
    assert runs(run, [300, 212, 1]) == [0, 2, 3]  # 512 fit, the 513th does not
    assert runs(run, [300, 213, 1]) == [0, 1, 3]
    assert runs(run, [512, 512]) == [0, 1, 2]


def test_a_run_closes_at_bl_lmw_landmarks(run):
    assert runs(run, [1] * 256) == [0, 256]
    assert runs(run, [1] * 257) == [0, 256, 257]


def test_a_landmark_larger_than_a_workgroup_empties_the_runs(run):
    assert runs(run, [3, 513, 3]) == []


# ------------------------------------------------------------------------------------------------ sub-problem
def test_sub_problem_of_a_landmark_range(run):
    obs = [(2, 4), (0, 1), (1, 3), (3, 2), (0, 3), (2, 0), (1, 2), (3, 4)]
    s = run("sub 4 5 8 2 2\n" + "".join("%d %d\n" % o for o in obs))  # landmarks 2, 3: observations 2, 3, 4, 6
    assert s["n_cams"] == [4] and s["n_lms"] == [2] and s["n_obs"] == [4] and s["points_offset"] == [6]
    assert s["obs_cam"] == [1, 3, 0, 1] and s["obs_lm"] == [1, 0, 1, 0] and s["obs_u"] == [2, 3, 4, 6]


def test_sub_problem_of_an_unobserved_range_is_empty(run):
    obs = [(0, 0), (1, 3), (0, 3), (1, 0)]
    s = run("sub 2 4 4 1 2\n" + "".join("%d %d\n" % o for o in obs))
    assert s["n_obs"] == [0] and s["obs_cam"] == [] and s["n_lms"] == [2]


# ---------------------------------------------------------------------------------------------------- threads
def checksum(a):
    a = np.asarray(a).astype(np.int64).astype(np.uint64)
    return int((np.arange(1, len(a) + 1, dtype=np.uint64) * a).sum(dtype=np.uint64))


def test_threads_and_failed_thread_starts_give_the_one_thread_plan(run):
    """Above both thresholds (2^19 observations, 2^15 landmarks).  The driver builds: landmark (48271 i) mod L, camera
    (lm C // L + (5 (i // L)) mod 9) mod C, cameras 0, 16, 32, 48 fixed; every team is forced to 1, 2, 3, 8 threads with
    the 1st, 2nd or last start failing.  The 1-thread plan is checked against numpy here, the others against it there."""
    C, L, O = 64, 1 << 15, 1 << 19
    out = run("threads %d %d %d\n" % (C, L, O), timeout=20)  # a team left waiting would end here, not stall the suite
    i = np.arange(O, dtype=np.int64)
    lm = i * 48271 % L
    cam = (lm * C // L + (5 * (i // L)) % 9) % C
    free_mask = (np.arange(C) % 16 != 0)
    lm_start = np.concatenate([[0], np.cumsum(np.bincount(lm, minlength=L))])
    perm = np.argsort(lm, kind="stable")
    s_cam = cam[perm]
    cam_start = np.concatenate([[0], np.cumsum(np.bincount(cam, minlength=C))])
    cam_obs = np.argsort(s_cam, kind="stable")
    cam_pos = np.empty(O, dtype=np.int64)
    cam_pos[cam_obs] = np.arange(O)
    k = np.bincount(lm[free_mask[cam]], minlength=L)
    assert out["sum lm_start"] == checksum(lm_start) and out["sum cam_start"] == checksum(cam_start)
    assert out["sum perm"] == checksum(perm) and out["sum obs_cam"] == checksum(s_cam) and out["sum obs_lm"] == checksum(lm[perm])
    assert out["sum cam_obs"] == checksum(cam_obs) and out["sum cam_pos"] == checksum(cam_pos)
    assert out["uv_err"] == 0.0
    assert out["kmax_free"] == [int(k.max())] and out["n_pairs"] == [int((k * k).sum())] and out["small"] == [0]
    # 16 observations per landmark: 32 landmarks fill a run of 512
    assert out["n_wg"] == [L // 32] and out["sum wg_lm"] == checksum(np.arange(0, L + 1, 32))
    # the covisibility graph of the free cameras, and the layout from the two half-bandwidths by the rule
    M = np.zeros((L, C), dtype=np.float32)
    M[lm, cam] = 1
    A = (M.T @ M)[np.ix_(free_mask, free_mask)] > 0
    nfree = int(free_mask.sum())
    edges = [(a, b) for a in range(nfree) for b in range(nfree) if a != b and A[a, b]]
    half_cyc = max(min(abs(a - b), nfree - abs(a - b)) for a, b in edges)
    assert out["half_cyc"] == [half_cyc]
    lay = out["layout"]
    assert lay["banded"] == 1 and lay["cyclic"] == 0  # 360 unknowns hold no ring of 8 blocks of >= 6 half_cyc + 6
    assert 8 * (6 * half_cyc + 6) > 6 * nfree
    free_cams, cam_free = out["free_cams"], out["cam_free"]
    assert sorted(free_cams) == [c for c in range(C) if free_mask[c]]
    assert [cam_free[c] for c in free_cams] == list(range(nfree)) and [cam_free[c] for c in range(0, C, 16)] == [-1] * 4
    natural = [c for c in range(C) if free_mask[c]]
    half = max(abs(cam_free[natural[a]] - cam_free[natural[b]]) for a, b in edges)
    assert out["half_lin"] == [half]
    assert lay == banded(6 * nfree, 6 * half + 5, cyclic=0) and 2 * (6 * half + 5 + 33) < 6 * nfree
    # every team size, every failed start: the same plan; `started` = threads that came to exist over the three regions
    # (covisibility pass, gather of the sorted copies, counting sort): all but the caller, or those before the failure
    want = [(1, 0, 0), (2, 0, 3), (2, 1, 0), (3, 0, 6), (3, 1, 0), (3, 2, 3), (8, 0, 21), (8, 1, 0), (8, 2, 3), (8, 7, 18)]
    assert [(c["threads"], c["fail_at"], c["started"]) for c in out["cases"]] == want
    assert all(c["equal"] == 1 for c in out["cases"])
