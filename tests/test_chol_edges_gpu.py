"""The six solve paths of visual-slam_amd/csrc/chol.hip on ill-conditioned band systems (tests/spd_ref.py: window Gram
matrices whose block coupling does not decay and whose 32 x 32 diagonal factors reach cond 1e4), judged by the normwise
backward error and the forward error against a long-double reference, each relative to what fp64 LAPACK reaches on
the same system (the rule and its measured constants: spd_ref.py, pinned by test_spd_ref_cpu.py).  Every case asserts
the path it took (Context.last_spd_path) with block size, block count and level count."""
import contextlib

import numpy as np
import pytest

import spd_ref as ref

pytestmark = pytest.mark.gpu

CASES = ref.cases()
BY_NAME = {c["name"]: c for c in CASES}
# the smallest accuracy case of every path: semantics that must hold on each of them
PER_PATH = [min((c for c in CASES if c["path"] == p and c["bw"] > 0 and not c["decades"]), key=lambda c: c["n"])["name"]
            for p in ref.PATHS]
_cache = {}


@contextlib.contextmanager
def _diagnostics(ctx, diag):
    try:
        for k, v in diag.items():
            ctx.set_diagnostic(k, v)
        yield
    finally:
        for k in diag:
            ctx.set_diagnostic(k, 0)


def _solve(ctx, case, S, b, bw_pass=None):
    bwp = case["bw_pass"] if bw_pass is None else bw_pass
    with _diagnostics(ctx, case["diag"]):
        return ctx.spd_solve_cyclic(S, b, bwp) if case["cyclic"] else ctx.spd_solve(S, b, bwp)


def _band(case):
    return case["n"] - 1 if case["path"] == "dense_panels" else case["bw_pass"]


def _system(name):
    """(S, b, x_lapack, x_ld or None) of a case, computed once and left unchanged."""
    if name not in _cache:
        case = BY_NAME[name]
        S, b = ref.build_case(case)
        xl = ref.lapack_solve(S, b, _band(case), case["cyclic"])
        fwd = case["forward"] and name not in ref.FORWARD_DROPPED and ref.LD_OK
        _cache[name] = (S, b, xl, ref.solve_ld(S, b, _band(case), case["cyclic"]) if fwd else None)
        for a in _cache[name]:
            if a is not None:
                a.setflags(write=False)
    return _cache[name]


def _assert_path(ctx, case):
    assert ctx.last_spd_path() == (case["path"], case["block"], case["n_blocks"], case["levels"]), case["name"]


def _assert_accurate(case, S, b, x, xl, x_ld, path=None, bw=None):
    path, bw = path or case["path"], _band(case) if bw is None else bw
    eta, eta_l = ref.backward_error(S, x, b, bw, case["cyclic"]), ref.backward_error(S, xl, b, bw, case["cyclic"])
    print("%s: eta %.2e (LAPACK %.2e, bound %.2e)" % (case["name"], eta, eta_l, ref.eta_bound(path, eta_l)))
    assert np.all(np.isfinite(x))
    assert eta <= ref.eta_bound(path, eta_l)
    if x_ld is not None:
        fwd, fwd_l = ref.forward_error(x, x_ld), ref.forward_error(xl, x_ld)
        print("%s: fwd %.2e (LAPACK %.2e, bound %.2e)" % (case["name"], fwd, fwd_l, ref.fwd_bound(path, fwd_l)))
        assert fwd <= ref.fwd_bound(path, fwd_l)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_path_and_accuracy(ctx, name):
    if BY_NAME[name]["forward"] and not ref.LD_OK:
        pytest.skip(ref.LD_SKIP_REASON)
    case = BY_NAME[name]
    S, b, xl, x_ld = _system(name)
    x = _solve(ctx, case, S, b)
    _assert_path(ctx, case)
    _assert_accurate(case, S, b, x, xl, x_ld)


@pytest.mark.parametrize("name", PER_PATH)
def test_zero_right_hand_side_and_identical_reruns(ctx, name):
    case = BY_NAME[name]
    S, b, _, _ = _system(name)
    x0 = _solve(ctx, case, S, np.zeros(case["n"]))
    _assert_path(ctx, case)
    assert not x0.any() and not np.signbit(x0).any()       # exactly +0
    x1, x2 = _solve(ctx, case, S, b), _solve(ctx, case, S, b)
    assert x1.tobytes() == x2.tobytes()                    # no atomics anywhere


@pytest.mark.parametrize("name", ["bcr-b32-15blk-ragged31-bw20", "ring-b32-15blk-bw20", "two-ended-sep-bw", "fused-8B-1",
                                  "panels-no-fused"])
def test_entries_outside_the_declared_band_are_ignored(ctx, name):
    # a matrix 5 diagonals wider than declared (delta = 2: what is left after the truncation is still positive
    # definite, the Gram part has norm <= ~4 spread over bw + 6 diagonals): the very bytes of the truncated solve
    case = BY_NAME[name]
    n, bw = case["n"], case["bw_pass"]
    S = ref.chain_spd(n, bw + 5, 91, 2.0, case["cyclic"])
    St = ref.truncate(S, bw, case["cyclic"])
    assert ref.half_bandwidth(S, case["cyclic"]) == bw + 5 and ref.half_bandwidth(St, case["cyclic"]) == bw
    np.linalg.cholesky(St)
    b = np.random.default_rng(92).standard_normal(n)
    x = _solve(ctx, case, S, b)
    _assert_path(ctx, case)
    xt = _solve(ctx, case, St, b)
    assert x.tobytes() == xt.tobytes()
    assert ref.backward_error(St, x, b, bw, case["cyclic"]) <= ref.eta_bound(
        case["path"], ref.backward_error(St, ref.lapack_solve(St, b, bw, case["cyclic"]), b, bw, case["cyclic"]))


@pytest.mark.parametrize("name,wider", [("bcr-b32-15blk-ragged31-bw20", 27), ("bcr-b32-15blk-ragged31-bw20", 40),
                                        ("ring-b32-15blk-bw20", 27), ("two-ended-sep-bw+31", 30), ("fused-8B-1", 45),
                                        ("panels-no-fused", 33), ("dense-bw-n-1", 100000)])
def test_a_wider_declared_band_gives_the_same_solution(ctx, name, wider):
    # explicit zeros inside the declared band (another block size or another path where the width says so): same x, to
    # the bound of the path taken
    case = BY_NAME[name]
    S, b, xl, x_ld = _system(name)
    path, B, nblk, levels = ref.expected_path(case["n"], wider, case["cyclic"], case["diag"].get("chol_no_fused", 0),
                                              case["diag"].get("chol_no_bcr", 0), case["diag"].get("chol_one_ended", 0))
    x = _solve(ctx, case, S, b, wider)
    assert ctx.last_spd_path() == (path, B, nblk, levels)
    _assert_accurate(case, S, b, x, xl, x_ld, path=path, bw=min(wider, case["n"] - 1))


def test_plan_cache_follows_size_bandwidth_and_form(vsl, ctx):
    # the context keeps ONE reduction plan with its job lists on the device, keyed by (n, bandwidth, form): a chain, a
    # ring, the chain of the ring's very (n, bw), the first chain again -- every solve with the bytes that a context
    # which has never held another plan gives
    first, ring, chain = BY_NAME["bcr-b32-8blk-bw0"], BY_NAME["ring-b32-15blk-bw20"], BY_NAME["bcr-b32-15blk-ragged31-bw20"]
    assert (first["n"], first["path"]) == (256, "bcr")
    assert (ring["n"], ring["bw_pass"], ring["path"]) == (479, 20, "bcr_cyclic")
    assert (chain["n"], chain["bw_pass"], chain["path"]) == (479, 20, "bcr")
    for case in (first, ring, chain, first):
        S, b = _system(case["name"])[:2]
        x = _solve(ctx, case, S, b)
        _assert_path(ctx, case)
        fresh = vsl.Context(0)
        try:
            x_fresh = _solve(fresh, case, S, b)
            _assert_path(fresh, case)
        finally:
            fresh.close()
        assert x.tobytes() == x_fresh.tobytes(), case["name"]
        assert np.all(np.isfinite(x))


NEGATIVE = [("dense_panels", 97, 48, False, -1, {}), ("band_panels", 467, 20, False, 20, {"chol_no_fused": 1}),
            ("band_fused", 467, 20, False, 20, {"chol_no_bcr": 1, "chol_one_ended": 1}),
            ("band_two_ended", 467, 20, False, 20, {"chol_no_bcr": 1}), ("bcr", 512, 31, False, 31, {}),
            ("bcr_cyclic", 512, 31, True, 31, {})]


@pytest.mark.parametrize("path,n,bw,cyclic,bw_pass,diag", NEGATIVE, ids=[t[0] for t in NEGATIVE])
def test_indefinite_only_through_global_coupling(ctx, vsl, path, n, bw, cyclic, bw_pass, diag):
    # every leading block up to n / 2 (and the trailing and middle ones) is positive definite: the pivot can only fail at
    # the separator, the last panel or the last level.  Error -7, and the context solves the next system correctly.
    S = ref.globally_indefinite(n, bw, 7, cyclic)
    case = dict(name="indefinite-" + path, n=n, cyclic=cyclic, bw_pass=bw_pass, diag=diag, path=path)
    with pytest.raises(vsl.VslError) as e:
        _solve(ctx, case, S, np.ones(n))
    assert e.value.code == -7
    assert ctx.last_spd_path()[0] == path
    Sg = ref.chain_spd(n, bw, 8, 1e-6, cyclic)
    bg = np.random.default_rng(9).standard_normal(n)
    x = _solve(ctx, case, Sg, bg)
    assert ctx.last_spd_path()[0] == path
    band = n - 1 if bw_pass < 0 else bw_pass
    _assert_accurate(case, Sg, bg, x, ref.lapack_solve(Sg, bg, band, cyclic), None, bw=band)


@pytest.mark.parametrize("name", ["bcr-b32-15blk-ragged31-bw20", "ring-b32-15blk-bw20", "bcr-b32-9blk-ragged1-bw1"])
@pytest.mark.parametrize("where", ["last_block", "deepest_level", "first_block"])
def test_negative_diagonal_in_the_last_block_and_at_the_deepest_level(ctx, vsl, name, where):
    # -1 inside the ragged last block, inside the block eliminated at the deepest level (block 2^(levels - 1): the last
    # level's ring or chain of two is blocks 0 and 2^(levels - 1)), and inside block 0, which is factored last of all
    case = BY_NAME[name]
    S, b, _, _ = _system(name)
    _, nblk, off = ref.bcr_layout(case["n"], case["bw_pass"], case["cyclic"])
    blk = {"last_block": nblk - 1, "deepest_level": 2 ** (case["levels"] - 1), "first_block": 0}[where]
    i = (off[blk] + off[blk + 1]) // 2
    S = S.copy()
    S[i, i] = -1.0
    with pytest.raises(vsl.VslError) as e:
        _solve(ctx, case, S, b)
    assert e.value.code == -7
    _assert_path(ctx, case)
