"""describe_tile_kernel computes the two orientation moments with int8 matrix instructions on pixels biased by -128.
The moments must be the integers the byte sums give -- so positions, moments, angle bit patterns, descriptor bytes and
near-tie records of the tile path are compared with the generic describe_kernel of the same build (diagnostic knobs),
with a numpy sum over the clamped disc, and with the CPU oracle where the oracle is defined (windows inside the image).

Corners are placed through Frames.describe_at (vsl_diag_frames_describe_at), so the number of keypoints per tile is
exact; describe_tile_min_images = 1 sends launches of 2 to 8 small images through the tile kernel.  The near-tie
radius is widened to 5e-5 px (below the 1e-4 px band the fast kernels re-examine) so that the records are not empty."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the 256 test pairs {xa, ya, xb, yb} the library is built from
_PAT_TEXT = (Path(__file__).resolve().parents[1] / "visual-slam_amd" / "csrc" / "rbrief_pattern.inc").read_text()
PATTERN = [tuple(int(v) for v in m) for m in re.findall(r"\{\s*(-?\d+),\s*(-?\d+),\s*(-?\d+),\s*(-?\d+)\}", _PAT_TEXT)]
assert len(PATTERN) == 256

W, H = 160, 144          # tiles are 128 x 128: a tile boundary at x = 128 and at y = 128, four tiles
TIE_EPS = 5e-5
_DY, _DX = np.mgrid[-15:16, -15:16]
_DISC = (_DX * _DX + _DY * _DY) <= 225
HALF_PLANE_MAX = 255 * int((-_DX[_DISC & (_DX < 0)]).sum())   # all of the disc's left half at 255, the rest 0


def ref_moments(img, pts):
    """(m01, m10) over the radius-15 disc with coordinates clamped to the image, as every describe kernel reads it."""
    h, w = img.shape
    out = np.zeros((len(pts), 2), np.int64)
    for k, (x, y) in enumerate(pts):
        v = img[np.clip(y + _DY, 0, h - 1), np.clip(x + _DX, 0, w - 1)].astype(np.int64) * _DISC
        out[k] = ((_DY * v).sum(), (_DX * v).sum())
    return out


def textured(seed, w=W, h=H):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8)).astype(np.float32)
    img = np.kron(base, np.ones((8, 8), np.float32))[:h, :w]
    return np.clip(img + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def describe(ctx, vsl, imgs, corners, path):
    """One launch over all images on `path` ('tile' or 'generic'): per-slot moments, positions, angles, descriptors and
    the sorted near-tie records."""
    imgs = np.stack(imgs)
    n, h, w = imgs.shape
    fr = vsl.Frames(ctx, n, w, h, max(1, max(len(c) for c in corners)), max_pairs=1)
    knob, on, off = ("describe_tile_min_images", 1, 96) if path == "tile" else ("force_generic_describe", 1, 0)
    ctx.set_diagnostic(knob, on)
    ctx.set_tie_eps(TIE_EPS)
    try:
        fr.upload(0, imgs)
        mom, word, rec = fr.describe_at(0, corners, True)
        assert word & (1 << 30) == 0, "exact-list overflow: the launch would be redone by the generic kernel"
        assert (word & ((1 << 30) - 1)) == len(rec)
        fr.resolve_ties()
        kps = [fr.keypoints(i) for i in range(n)]
    finally:
        ctx.set_tie_eps(1e-12)
        ctx.set_diagnostic(knob, off)
        fr.close()
    assert (rec[:, 3] == 0).all()
    ties = sorted(map(tuple, rec[:, :3].tolist()))
    return {"mom": mom, "xy": [k[0] for k in kps], "ang": [k[1] for k in kps], "desc": [k[2] for k in kps], "ties": ties}


def check(ctx, vsl, orc, imgs, corners):
    corners = [np.asarray(c, np.int32).reshape(-1, 2) for c in corners]
    t = describe(ctx, vsl, imgs, corners, "tile")
    g = describe(ctx, vsl, imgs, corners, "generic")
    # The generic kernel flags |frac - 0.5| < eps.  The fast path's integer test scales the distance to EITHER rounding
    # boundary of round(v) = k by 2k + 1 (exact_round_ratio), which is exact for the upper boundary and loose by
    # (2k + 1) / (2k - 1) <= 3 for the lower one: it flags every sample the generic kernel flags, and whatever else it
    # flags lies within 3 eps of a boundary (a flag only sends the bit to the host's libm check).
    assert set(g["ties"]) <= set(t["ties"])
    for slot, kp, bit in sorted(set(t["ties"]) - set(g["ties"])):
        m01, m10 = (float(v) for v in t["mom"][slot][kp])
        nrm = math.hypot(m01, m10)
        xa, ya, xb, yb = PATTERN[bit]
        v = [(m10 * xa - m01 * ya) / nrm, (m01 * xa + m10 * ya) / nrm, (m10 * xb - m01 * yb) / nrm, (m01 * xb + m10 * yb) / nrm]
        assert min(abs(abs(c) % 1.0 - 0.5) for c in v) < 3.0 * TIE_EPS * (1 + 1e-6), (slot, kp, bit)
    for i, (img, c) in enumerate(zip(imgs, corners)):
        h, w = img.shape
        assert np.array_equal(t["xy"][i], c.astype(np.float64)) and np.array_equal(g["xy"][i], t["xy"][i])
        assert np.array_equal(t["mom"][i], g["mom"][i]), i
        want = ref_moments(img, c)
        assert np.array_equal(t["mom"][i], want), i
        assert np.array_equal(t["ang"][i].view(np.uint64), g["ang"][i].view(np.uint64))
        assert np.array_equal(t["ang"][i].view(np.uint64),
                              np.array([math.atan2(a, b) for a, b in want], np.float64).view(np.uint64))
        assert np.array_equal(t["desc"][i], g["desc"][i]), i
        inner = (c[:, 0] >= 19) & (c[:, 0] < w - 20) & (c[:, 1] >= 19) & (c[:, 1] < h - 19)   # the oracle does not clamp
        if inner.any():
            kp = c[inner].astype(np.float64)
            o01, o10 = orc.patch_moments(img, kp)
            assert np.array_equal(t["mom"][i][inner], np.stack([o01, o10], 1))
            oang = orc.compute_angles(img, kp, True)
            assert np.array_equal(t["ang"][i][inner].view(np.uint64), oang.view(np.uint64))
            assert np.array_equal(t["desc"][i][inner], orc.compute_descriptors(img, kp, oang))
    return t


def grid(step=9):
    return [(x, y) for y in range(0, H, step) for x in range(0, W, step)]


def test_constant_images_have_zero_moments(ctx, vsl, orc):
    # the -128 bias must cancel exactly: moments 0, angle 0 (the n2 == 0 branch), also where the window is clamped
    imgs = [np.full((H, W), v, np.uint8) for v in (255, 0, 128)]
    t = check(ctx, vsl, orc, imgs, [grid()] * 3)
    for i in range(3):
        assert not t["mom"][i].any() and not t["ang"][i].any()


def test_half_planes_reach_the_largest_moments(ctx, vsl, orc):
    left = np.zeros((H, W), np.uint8)
    left[:, :80] = 255
    top = np.zeros((H, W), np.uint8)
    top[:72, :] = 255
    pts = grid(7) + [(x, y) for x in range(60, 100) for y in (40, 72, 100)] + [(x, y) for y in range(52, 92) for x in (30, 80, 140)]
    t = check(ctx, vsl, orc, [left, top, 255 - left, 255 - top], [pts] * 4)
    # (80, y): pixels with dx < 0 are 255, the others 0 -- the extreme of m10; the same for m01 on the transpose
    assert t["mom"][0][:, 1].min() == -HALF_PLANE_MAX and t["mom"][2][:, 1].max() == HALF_PLANE_MAX
    assert t["mom"][1][:, 0].min() == -HALF_PLANE_MAX and t["mom"][3][:, 0].max() == HALF_PLANE_MAX


def test_borders_corners_and_tile_boundaries(ctx, vsl, orc):
    pts = []
    for d in list(range(0, 20)):       # within 15 and within 19 pixels of each border
        pts += [(d, 70), (W - 1 - d, 71), (75, d), (76, H - 1 - d), (d, d), (W - 1 - d, d), (d, H - 1 - d), (W - 1 - d, H - 1 - d)]
    for a in range(120, 137):          # both sides of the tile boundaries at x = 128 and y = 128, and their crossing
        pts += [(a, 60), (60, a), (a, a), (a, 255 - a)]
    pts += [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (127, 127), (128, 128), (127, 128), (128, 127)]
    imgs = [textured(s) for s in (11, 12)]
    check(ctx, vsl, orc, imgs, [pts, pts[::-1]])


@pytest.mark.parametrize("counts", [(0, 1, 15, 16, 17, 33, 70, 137), (600, 129)])
def test_keypoints_per_tile(ctx, vsl, orc, counts):
    # tile 0 (x, y < 128) holds exactly `count` keypoints: empty tile, partial and several groups of 16 per wavefront
    # (8 wavefronts take every 8th entry: 137 gives one of them 18), parked lanes, and with 600 a second batch of 64 per
    # wavefront; the three small tiles hold 0 to 2 each
    rng = np.random.default_rng(sum(counts))
    imgs, corners = [], []
    for i, c in enumerate(counts):
        imgs.append(textured(100 + i))
        pts = np.stack([rng.integers(0, 128, c), rng.integers(0, 128, c)], 1)
        extra = [(130 + i, 5 + i), (140, 130 + i), (7 * i, 135)][:i % 4]
        corners.append(np.concatenate([pts, np.array(extra, np.int64).reshape(-1, 2)]))
    check(ctx, vsl, orc, imgs, corners)


def test_headline_stereo_pair(ctx, vsl, orc, synth):
    # the benchmark's shape: a seeded 752 x 480 stereo pair, 1500 features, detected and described on the tile path
    left, right = synth.stereo_pair(21)
    imgs = np.stack([left, right])
    fr = vsl.Frames(ctx, 2, imgs.shape[2], imgs.shape[1], 1500, max_pairs=1)
    ctx.set_diagnostic("describe_tile_min_images", 1)
    try:
        fr.upload(0, imgs)
        fr.detect_describe(0, 2, 1500, True)
        fr.resolve_ties()
        got = [fr.keypoints(i) for i in range(2)]
    finally:
        ctx.set_diagnostic("describe_tile_min_images", 96)
        fr.close()
    for img, (xy, ang, desc) in zip(imgs, got):
        oxy, oang, odesc = orc.detect_describe(img, 1500, True)
        assert len(xy) > 1000 and np.array_equal(xy, oxy)
        assert np.array_equal(ang.view(np.uint64), oang.view(np.uint64)) and np.array_equal(desc, odesc)
    # the same corners placed by hand: moments and tie records of the tile path against the generic kernel and the oracle
    check(ctx, vsl, orc, list(imgs), [g[0].astype(np.int32) for g in got])
