"""GPU: iterative Schur -- the matrix-free PCG on the reduced camera system (visual-slam_amd/csrc/ba_pcg.h).

Bars, per quantity (n = unknowns of the reduced system, S_oracle / g_oracle from the oracle's linearisation):
  (1) product      |y - S_oracle x|_inf <= n * 1e-9 * max|S_oracle| for |x|_inf <= 1: the project accepts 1e-9 max|S| per
                   entry of S (tests/test_ba_gpu.py) and an entry of y sums n of them;
  (2) solve        tol 1e-12: reported rel_residual <= tol, iterations <= 4 n, the residual recomputed from S_oracle agrees
                   with the reported one within bar (1) (scaled by |x|_inf: the bar is per unit of x), error in x at most
                   cond(S_oracle) * 1e-12 * |x|;
  (3) LM, tight    "ba_pcg_tol_exp" = 12 against the switch off and against the oracle: the bars of
                   test_bundle_adjust_matches_oracle (same iterations / termination / successful steps, final cost rel
                   1e-7, poses and points atol 1e-6), fixed cameras bit-unchanged;
  (4) LM, default  forcing term 0.1: a convergence code, cost decreased, relative gap of the final cost to the direct
                   route's at most LM_FUNCTION_TOLERANCE (1e-6, lm_policy.h) times the iterations run.
                   Measured on the MI355X: 1.96e-7 after 7 iterations (small), 3.01e-6 after 5 (big).
Shapes: tests/ba_wide_ref.py -- 16 keyframes (30 free cameras, 180 unknowns: beyond the fused window and beyond the
one-workgroup dense solve) and 40 keyframes (78 free cameras: three segments per camera in the camera pass, > 200
workgroups in the landmark pass).  tests/test_ba_pcg_cpu.py checks on the CPU that block-Jacobi PCG on S_oracle reaches
1e-12 within 4 n on these seeds."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ba_wide_ref as W

pytestmark = pytest.mark.gpu

SHAPES = {"small": (1, 16, 600), "big": (2, 40, 1500)}
_cache = {}


def _problem(synth, name):
    if name not in _cache:
        _cache[name] = W.wide(synth, *SHAPES[name])
    return _cache[name]


def _oracle_lin(orc, synth, name, huber=True, model=0):
    key = ("lin", name, huber, model)
    if key not in _cache:
        d = dict(_problem(synth, name))
        d["cam_model"] = (model, model)
        if model == 1:  # the extended-unified parameters of tests/test_ba_gpu.py's table
            d["intr"] = np.array([[350.0, 348.0, 365.0, 249.0, 0, 0, 0, 0]] * 2)
        S, g, c = orc.ba_linearize(W.arrays(orc, d), use_huber=huber)
        S.setflags(write=False)
        g.setflags(write=False)
        _cache[key] = (d, S, g)
    return _cache[key]


def _solve(ctx, orc, d, iterative, max_iters=20, tol_exp=0, poll=0, huber=True):
    a = W.arrays(orc, d)
    ctx.set_diagnostic("ba_iterative_schur", int(iterative))
    ctx.set_diagnostic("ba_pcg_tol_exp", tol_exp)
    ctx.set_diagnostic("ba_pcg_poll", poll)
    try:
        s = ctx.bundle_adjust(a, use_huber=huber, max_iters=max_iters)
        layout, pcg = ctx.last_ba_layout(), ctx.last_ba_pcg()
    finally:
        ctx.set_diagnostic("ba_iterative_schur", 0)
        ctx.set_diagnostic("ba_pcg_tol_exp", 0)
        ctx.set_diagnostic("ba_pcg_poll", 0)
    return SimpleNamespace(s=s, a=a, layout=layout, pcg=pcg)


def _direct(ctx, orc, synth, name):
    key = ("direct", name)
    if key not in _cache:
        _cache[key] = _solve(ctx, orc, _problem(synth, name), False)
    return _cache[key]


def _same_trajectory(x, y):
    assert (x.s.iterations, x.s.termination, x.s.successful_steps) == (y.s.iterations, y.s.termination, y.s.successful_steps)
    assert x.s.final_cost == pytest.approx(y.s.final_cost, rel=1e-7)
    assert np.allclose(x.a.poses, y.a.poses, rtol=0, atol=1e-6)
    assert np.allclose(x.a.points, y.a.points, rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", ["small", "big"])
def test_wide_maps_are_dense_with_the_switch_off(ctx, orc, synth, name):
    d = _problem(synth, name)
    assert W.covisible_fraction(d) > 0.95
    W.assert_dense_when_off(ctx, orc, d)
    assert ctx.last_ba_pcg() == (0, 0, 0, 0.0)


# ---------------------------------------------------------------------------------------------- (1) product
@pytest.mark.parametrize("name,huber,model", [("small", True, 0), ("small", False, 0), ("small", True, 1), ("big", True, 0)])
def test_product_matches_the_oracle_matrix(ctx, orc, synth, name, huber, model):
    d, S, g = _oracle_lin(orc, synth, name, huber, model)
    arr = W.arrays(orc, d)
    n = len(g)
    assert n > 128
    rng = np.random.default_rng(5)
    xs = [np.eye(n)[0], np.eye(n)[n - 6], np.eye(n)[n - 1]] + [rng.uniform(-1, 1, n) for _ in range(3)]
    bar = n * 1e-9 * np.abs(S).max()
    for x in xs:
        y = ctx.ba_schur_apply(arr, x, use_huber=huber)
        err = np.abs(y - S @ x).max()
        print("product %s huber=%s model=%d: err %.3e bar %.3e" % (name, huber, model, err, bar))
        assert err <= bar
        assert np.array_equal(ctx.ba_schur_apply(arr, -x, use_huber=huber), -y)  # linear in bits under x -> -x
        assert np.array_equal(ctx.ba_schur_apply(arr, x, use_huber=huber), y)    # repeatable bit for bit


# ---------------------------------------------------------------------------------------------- (2) solve
@pytest.mark.parametrize("name", ["small", "big"])
def test_pcg_solves_the_oracle_system(ctx, orc, synth, name):
    d, S, g = _oracle_lin(orc, synth, name)
    arr = W.arrays(orc, d)
    n, tol = len(g), 1e-12
    x_ref = np.linalg.solve(S, g)
    x, it, rel = ctx.ba_schur_pcg(arr, tol=tol)
    res_host = np.linalg.norm(g - S @ x)
    cond = np.linalg.cond(S)
    bar1 = n * 1e-9 * np.abs(S).max() * max(1.0, np.abs(x).max())
    print("pcg %s: it %d rel %.3e host residual %.3e |g| %.3e cond %.3e err %.3e" %
          (name, it, rel, res_host, np.linalg.norm(g), cond, np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)))
    assert rel <= tol and 0 < it <= 4 * n
    assert abs(res_host - rel * np.linalg.norm(g)) <= bar1
    assert np.linalg.norm(x - x_ref) <= cond * 1e-12 * np.linalg.norm(x_ref)
    assert ctx.last_ba_pcg()[:3] == (1, it, it)
    # another right-hand side, and the explicit g: the same call
    x2, it2, rel2 = ctx.ba_schur_pcg(arr, b=np.asarray(g), tol=tol)
    assert np.abs(x2 - x_ref).max() <= cond * 1e-12 * np.linalg.norm(x_ref) and rel2 <= tol
    e0 = np.zeros(n)
    e0[3] = 1.0
    x3, _, rel3 = ctx.ba_schur_pcg(arr, b=e0, tol=tol)
    x3_ref = np.linalg.solve(S, e0)
    assert rel3 <= tol and np.linalg.norm(x3 - x3_ref) <= cond * 1e-12 * np.linalg.norm(x3_ref)


# ---------------------------------------------------------------------------------------------- (3) LM, tight tolerance
@pytest.mark.parametrize("name", ["small", "big", "loop"])
def test_lm_with_tight_pcg_follows_the_direct_route_and_the_oracle(ctx, orc, synth, name):
    if name == "loop":
        d = synth.ba_problem(52, n_kf=60, n_lms=5000, loop_radius=10.0)
        off = _solve(ctx, orc, d, False)
        assert off.layout[1] in (1, 2)  # a band route when the switch is off
    else:
        d = _problem(synth, name)
        off = _direct(ctx, orc, synth, name)
        assert off.layout[1] == 0
    on = _solve(ctx, orc, d, True, tol_exp=12)
    assert on.layout[:2] == (0, 3)
    print("LM tight %s: direct (%d, %d, %d) cost %.9e; pcg cost %.9e, %d solves, %d PCG iterations" %
          (name, off.s.iterations, off.s.termination, off.s.successful_steps, off.s.final_cost, on.s.final_cost, on.pcg[0], on.pcg[1]))
    _same_trajectory(on, off)
    a_cpu = W.arrays(orc, d)
    cpu = SimpleNamespace(s=orc.bundle_adjust(a_cpu, max_iters=20), a=a_cpu)
    _same_trajectory(on, cpu)
    fixed = d["cam_fixed"].astype(bool)
    assert np.array_equal(on.a.poses[fixed], d["poses"][fixed])
    assert on.s.final_cost < on.s.initial_cost


# ---------------------------------------------------------------------------------------------- (4) LM, forcing term
@pytest.mark.parametrize("name", ["small", "big"])
def test_lm_with_the_default_forcing_term_converges(ctx, orc, synth, name):
    d = _problem(synth, name)
    off = _direct(ctx, orc, synth, name)
    on = _solve(ctx, orc, d, True, max_iters=50)
    gap = abs(on.s.final_cost - off.s.final_cost) / off.s.final_cost
    print("LM forcing %s: pcg (%d, %d, %d) cost %.9e, direct (%d, %d) cost %.9e, gap %.3e, %d PCG iterations in %d solves" %
          (name, on.s.iterations, on.s.termination, on.s.successful_steps, on.s.final_cost, off.s.iterations, off.s.termination,
           off.s.final_cost, gap, on.pcg[1], on.pcg[0]))
    assert on.s.termination in (1, 2, 3)
    assert on.s.final_cost < on.s.initial_cost
    assert gap <= 1e-6 * on.s.iterations  # LM_FUNCTION_TOLERANCE of lm_policy.h: each iteration may stop that far short


# ---------------------------------------------------------------------------------------------- (5) bookkeeping
def test_bookkeeping(ctx, orc, synth):
    d = _problem(synth, "small")
    n = 6 * int((d["cam_fixed"] == 0).sum())
    on = _solve(ctx, orc, d, True)
    assert on.layout[:2] == (0, 3)
    solves, total, last, rel = on.pcg
    assert solves == on.s.iterations and total >= solves and 0 < last <= 4 * n and 0.0 <= rel <= 0.1
    off = _solve(ctx, orc, d, False)
    assert off.layout[:2] == (n * n, 0) and off.pcg == (0, 0, 0, 0.0)


# ---------------------------------------------------------------------------------------------- (6) reproducibility, cadence
def test_two_solves_and_every_poll_cadence_return_the_same_bits(ctx, orc, synth):
    d = _problem(synth, "small")
    runs = [_solve(ctx, orc, d, True, poll=p) for p in (0, 0, 1, 8, 64)]
    for r in runs[1:]:
        assert np.array_equal(r.a.poses, runs[0].a.poses) and np.array_equal(r.a.points, runs[0].a.points)
        assert (r.s.iterations, r.s.final_cost, r.pcg) == (runs[0].s.iterations, runs[0].s.final_cost, runs[0].pcg)
    arr = W.arrays(orc, d)
    x1, it1, rel1 = ctx.ba_schur_pcg(arr, tol=1e-10)
    ctx.set_diagnostic("ba_pcg_poll", 3)
    try:
        x2, it2, rel2 = ctx.ba_schur_pcg(arr, tol=1e-10)
    finally:
        ctx.set_diagnostic("ba_pcg_poll", 0)
    assert np.array_equal(x1, x2) and (it1, rel1) == (it2, rel2)


# ---------------------------------------------------------------------------------------------- (7) edges
def test_landmark_seen_only_by_fixed_cameras(ctx, orc, synth):
    d = dict(_problem(synth, "small"))
    # one more landmark, observed by the two fixed cameras alone: it has no Z block
    src = 0
    m = (d["obs_lm"] == src) & (d["obs_cam"] < 2)
    assert m.sum() == 2
    L = len(d["points"])
    d["points"] = np.concatenate([d["points"], d["points"][src:src + 1] + 0.01])
    d["obs_cam"] = np.concatenate([d["obs_cam"], d["obs_cam"][m]])
    d["obs_lm"] = np.concatenate([d["obs_lm"], np.full(2, L, np.int32)])
    d["obs_uv"] = np.concatenate([d["obs_uv"], d["obs_uv"][m] + 1.0])
    off = _solve(ctx, orc, d, False)
    on = _solve(ctx, orc, d, True, tol_exp=12)
    _same_trajectory(on, off)


def test_free_camera_with_a_single_observation_and_the_context_afterwards(ctx, orc, synth):
    d = dict(_problem(synth, "small"))
    cam = len(d["poses"]) - 1
    keep = d["obs_cam"] != cam
    keep[np.flatnonzero(~keep)[0]] = True  # one observation left: two equations for six unknowns
    for k in ("obs_cam", "obs_lm", "obs_uv"):
        d[k] = d[k][keep]
    assert (d["obs_cam"] == cam).sum() == 1
    off = _solve(ctx, orc, d, False, max_iters=10)
    on = _solve(ctx, orc, d, True, tol_exp=12, max_iters=10)
    print("rank-deficient: direct termination %d (%d iterations), pcg termination %d (%d iterations)" %
          (off.s.termination, off.s.iterations, on.s.termination, on.s.iterations))
    assert on.s.termination == off.s.termination
    assert np.isfinite(on.a.poses).all() and np.isfinite(on.a.points).all()
    # the context stays usable: a well-posed solve passes afterwards
    good = _problem(synth, "small")
    again = _solve(ctx, orc, good, True, tol_exp=12)
    _same_trajectory(again, _direct(ctx, orc, synth, "small"))


def test_zero_iterations_returns_zero_and_unit_residual(ctx, orc, synth):
    arr = W.arrays(orc, _problem(synth, "small"))
    x, it, rel = ctx.ba_schur_pcg(arr, tol=1e-12, max_iterations=0)
    assert it == 0 and rel == 1.0 and not x.any()


def test_two_ranks_with_the_switch_on_are_refused(ctx, vsl, orc, synth):
    d = _problem(synth, "small")
    arr = W.arrays(orc, d)
    st, o, out = ctx._ba_struct(arr), ctx._ba_opts(True, 1.0, 5, 0), vsl.BaSummary()
    called = []
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)
    cb = FN(lambda *a: called.append(1) or 1)
    ctx.set_diagnostic("ba_iterative_schur", 1)
    try:
        rc = ctx.L.vsl_global_bundle_adjust(ctx.h, C.byref(st), C.byref(o), cb, None, 0, 2, C.byref(out))
    finally:
        ctx.set_diagnostic("ba_iterative_schur", 0)
    assert rc == -1 and not called  # VSL_ERR_INVALID before any collective
    assert np.array_equal(arr.poses, d["poses"])


def test_local_window_ignores_the_switch(ctx, orc, synth):
    d = synth.ba_problem(51, n_kf=6, n_lms=2500)
    assert 6 * int((d["cam_fixed"] == 0).sum()) <= 126
    off = _solve(ctx, orc, d, False)
    on = _solve(ctx, orc, d, True)
    assert np.array_equal(on.a.poses, off.a.poses) and np.array_equal(on.a.points, off.a.points)
    assert (on.s.iterations, on.s.final_cost) == (off.s.iterations, off.s.final_cost)
