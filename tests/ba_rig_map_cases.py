"""TEST INFRASTRUCTURE: the case table of the rig MAP route (vsl_global_bundle_adjust_rig), shared by
tests/test_ba_rig_map_plan_cpu.py and tests/test_ba_rig_map_gpu.py.  Every scene comes from ba_rig_ref.rig_scene; the
long-double reference of a case is computed once per process and shared (read-only).

  case                scene                                                       expected storage (confirmed on the CPU)
  open                rig_scene(25, 1, 22, window=3): 24 free bodies, no wrap     linear band, half-bandwidth 2
  open_dense          three landmarks per window start (rig_scene(25, 1, 72, window=3)    linear band, half-bandwidth 2
                      with the wrapped views dropped): the open graph with end bodies
                      that see three landmarks -- `open` leaves its end bodies one
                      landmark each, the undamped system is singular and the LM runs
                      into the iteration limit; this one stops on the function tolerance
  open_edges          open, plus: free body 13 shares no landmark with another    linear band (the graph falls apart into
                      free body (diagonal-only pair), landmark 5 seen by the      components; the order keeps them apart)
                      fixed body only, body 11 carries a right camera only
  open_long_body      open, plus 520 landmarks seen by the fixed body and body 10 only:   linear band, half-bandwidth 2; the
                      523 groups in one body list, so the pairs of that body have two     renumbered slots carry the long list
                      segments IN BAND STORAGE (2256 observations)
  open_huber_models   open with camera models (0, 3) and two gross outliers       linear band, half-bandwidth 2
  ring_narrow         rig_scene(25, 1, 24, window=2): landmark windows wrap       linear band in RCM order (cyclic refused
                      (window=3 orders into half-bandwidth 5, linear blocks       by the 3/4 block rule: ring blocks of 32
                      of 64, and the rule then TAKES the ring: shape adjusted)    against linear blocks of 32)
  ring_cyclic         rig_scene(41, 1, 40, window=5): 240 unknowns                cyclic band, ring blocks of 32 x 8
  wide_clique         ring_cyclic plus landmark 0 seen by 14 free bodies          whatever ba_reduced_layout says
  small               ba_rig_ref's a_base (12 unknowns)                           dense, pair gather
  multi_segment       rig_scene(3, 1, 600): 600 groups per body, 2 segments       dense, pair gather (3600 observations)
"""
import numpy as np

import ba_rig_ref as ref

EXPECT_FORM = {"open": 1, "open_dense": 1, "open_long_body": 1, "open_edges": 1, "open_huber_models": 1, "ring_narrow": 1, "ring_cyclic": 2, "small": 0,
               "multi_segment": 0,
               # 14 free bodies on one landmark: half-bandwidth 17 in RCM order, 13 around the ring.  The ring needs
               # 8 blocks of >= 6 * 13 + 6 unknowns (240 have room for 2), the band 2 * (107 + 32 + 1) < 240: dense
               "wide_clique": 0}
# the solve tests: cases (and iteration limits) at which the dense route stops on the function tolerance.  wide_clique's
# extra views pull at one landmark and nine bodies: the free problem of the same cameras needs 39 iterations on the CPU
SOLVE_CASES = ("open_dense", "ring_cyclic", "wide_clique")
SOLVE_MAX_ITERS = {"open_dense": 20, "ring_cyclic": 20, "wide_clique": 60}

# The figure the device bound derives from (the rule of ba_rig_ref.py): the CPU oracle's ba_linearize of the expanded
# problem, folded with A in float64 numpy, against the long-double reference, entrywise in units of 2^-52 A.  Measured by
# tests/test_ba_rig_map_plan_cpu.py on the cases of this table (x86-64, 80-bit long double): S 13.10 on `open`, 5.01 on
# ring_cyclic / wide_clique, 4.15 ring_narrow, 1.66 open_dense, 3.26 open_huber_models, 2.52 open_edges, 0.30 multi_segment; g at most
# 1.68.  That is past ba_rig_ref.ORACLE_FOLD_VS_REF_K = 3.0 (whose cases have 3 bodies, or 23 with one wide landmark), so
# the new cases get their own constant, recorded rounded up, and the device 8 x it, capped at 64.  `small` IS a case of
# ba_rig_ref and keeps K_RIG_GPU.
MAP_ORACLE_FOLD_VS_REF_K = 13.5
K_MAP_GPU = min(8.0 * MAP_ORACLE_FOLD_VS_REF_K, 64.0)


def k_gpu(name):
    return ref.K_RIG_GPU if name == "small" else K_MAP_GPU


def _open(seed=600, **kw):
    return ref.rig_scene(25, 1, 22, seed, window=3, **kw)


def _add_clique(rp, seed):
    """Landmark 0 also from every camera of bodies up to 14 that does not see it yet (14 free bodies in all), as case
    h_23_free of ba_rig_ref builds it."""
    have = set(rp.obs_camera[rp.obs_lm == 0].tolist())
    extra_c = np.array([c for c in range(len(rp.cam_body)) if 1 <= rp.cam_body[c] <= 14 and c not in have])
    rp.obs_camera = np.concatenate([rp.obs_camera, extra_c]).astype(np.int32)
    rp.obs_lm = np.concatenate([rp.obs_lm, np.zeros(len(extra_c), np.int32)]).astype(np.int32)
    rp.obs_uv = np.concatenate([rp.obs_uv, np.zeros((len(extra_c), 2))])
    true_uv = rp.obs_uv - rp.blocks(jac=False).astype(np.float64)
    rng = np.random.default_rng(seed)
    rp.obs_uv[-len(extra_c):] = true_uv[-len(extra_c):] + 0.5 * rng.normal(size=(len(extra_c), 2))
    return rp


def _open_dense(seed=700):
    rp = ref.rig_scene(25, 1, 72, seed, window=3)
    free = rp.cam_body[rp.obs_camera] - 1                  # free index of the observing body, -1 the fixed one
    return ref._drop(rp, ~((free >= 0) & (free < rp.obs_lm % 24)))     # a view from before the window's start has wrapped


def _open_long_body(seed=605, extra=520):
    rp = ref.rig_scene(25, 1, 22 + extra, seed)            # everything sees everything, then cut down
    body, lm = rp.cam_body[rp.obs_camera], rp.obs_lm
    keep = np.where(lm < 22, (body == 0) | (((body - 1) - lm) % 24 < 3), (body == 0) | (body == 10))
    return ref._drop(rp, keep)


def _build():
    T = {}
    T["open"] = _open()
    T["open_long_body"] = _open_long_body()
    T["open_dense"] = _open_dense()
    rp = _open(603, cams_of_body=[(0, 1)] * 11 + [(1,)] + [(0, 1)] * 13)
    body = rp.cam_body[rp.obs_camera]
    drop = ((body == 13) & (rp.obs_lm != 12)) | ((rp.obs_lm == 12) & ((body == 14) | (body == 15))) | ((rp.obs_lm == 5) & (body != 0))
    T["open_edges"] = ref._drop(rp, ~drop)
    rp = _open(604, models=(0, 3), use_huber=True, huber=1.0)
    i0 = int(np.flatnonzero((rp.obs_camera == 8) & (rp.obs_lm == 3))[0])
    i1 = int(np.flatnonzero((rp.obs_camera == 31) & (rp.obs_lm == 14))[0])
    rp.obs_uv[i0] += [35.0, -22.0]
    rp.obs_uv[i1] += [-28.0, 41.0]
    rp.outliers = (i0, i1)
    T["open_huber_models"] = rp
    T["ring_narrow"] = ref.rig_scene(25, 1, 24, 601, window=2)
    T["ring_cyclic"] = ref.rig_scene(41, 1, 40, 602, window=5)
    T["wide_clique"] = _add_clique(ref.rig_scene(41, 1, 40, 602, window=5), 6021)
    T["small"] = ref.cases()["a_base"]
    T["multi_segment"] = ref.rig_scene(3, 1, 600, 509)
    for name, rp in T.items():
        if name != "small":
            rp.name = "map/" + name
    return T


_CASES = None
_LIN = {}


def cases():
    """name -> RigProblem, built once (read-only: copy what a solve changes)."""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def reference(name, inv_radius=None):
    key = (name, inv_radius)
    if key not in _LIN:
        _LIN[key] = ref.linearize(cases()[name], inv_radius)
    return _LIN[key]


def problem_text(rp):
    """The stdin of tests/cpp/ba_rig_map_plan_test.cpp."""
    j = lambda v: " ".join(str(int(x)) for x in v)  # noqa: E731
    return "%d\n%s\n%d\n%s\n%s\n%d %d\n%s\n%s\n" % (len(rp.cam_fixed), j(rp.cam_fixed), len(rp.cam_body), j(rp.cam_body), j(rp.cam_intr),
                                                 len(rp.points), len(rp.obs_lm), j(rp.obs_camera), j(rp.obs_lm))
