"""TEST INFRASTRUCTURE: the problems of the band-route covariance tests (tests/test_global_ba_covariance_gpu.py), built
from synth.ba_problem(..., loop_radius=R), and their references, computed once per problem and shared.

open_chain   the first 30 keyframes of a 120-keyframe loop: 60 cameras in a chain, 388 landmarks, 2352 observations, at
             most 10 observations per landmark, covisibility half bandwidth 9 cameras.  With cameras 0 and 1 fixed:
             n = 348 unknowns (ten panels of 32 and a ragged one), bw = 59, 2 (59 + 33) = 184 < 348: linear band.
ring         a closed 64-keyframe loop, uncut: 128 cameras (126 free), 1420 landmarks, 5029 observations, n = 756.
             Half bandwidth 5 cameras around the ring, about 10 in reverse Cuthill-McKee order: band position != id.
The band condition is 2 (6 half + 38) < 6 n_free with n > 128 (ba_reduced_layout); every test asserts the route.
"""
import numpy as np

import ba_cov_ref as R

_cache = {}


def open_chain(synth, fixed=(0, 1), n_cams=60):
    """The dict of arrays; `fixed`: the camera ids that are fixed."""
    key = ("chain", n_cams)
    if key not in _cache:
        d = synth.ba_problem(3, n_kf=120, n_lms=1500, loop_radius=60.0)
        sel = d["obs_cam"] < n_cams
        cnt = np.bincount(d["obs_lm"][sel], minlength=len(d["points"]))
        keep = cnt >= 2
        remap = -np.ones(len(keep), np.int64)
        remap[keep] = np.arange(keep.sum())
        sel &= keep[d["obs_lm"]]
        e = dict(d)
        e["poses"], e["cam_intr"] = d["poses"][:n_cams].copy(), d["cam_intr"][:n_cams].copy()
        e["points"] = d["points"][keep].copy()
        e["obs_cam"], e["obs_uv"] = d["obs_cam"][sel].copy(), d["obs_uv"][sel].copy()
        e["obs_lm"] = remap[d["obs_lm"][sel]].astype(np.int32)
        _cache[key] = e
    e = dict(_cache[key])
    e["cam_fixed"] = np.zeros(n_cams, np.uint8)
    e["cam_fixed"][list(fixed)] = 1
    return e


def ring(synth):
    if "ring" not in _cache:
        _cache["ring"] = synth.ba_problem(3, n_kf=64, n_lms=1500, loop_radius=60.0)
    return dict(_cache["ring"])


def chain_ref(orc, synth, fixed=(0, 1), huber=True):
    """ba_cov_ref.Ref (numpy.linalg.inv of the full dense H from the oracle's Jacobians) of the open chain."""
    key = ("chain_ref", tuple(fixed), huber)
    if key not in _cache:
        _cache[key] = R.Ref(orc, R.arrays(orc, open_chain(synth, fixed)), use_huber=huber)
    return _cache[key]


def max_block_error(blocks, ref_block, ids):
    return max(float(np.abs(blocks[k] - ref_block(i)).max()) for k, i in enumerate(ids))
