"""Helpers of tests/test_orb_{ref_cpu,gpu}.py: a vectorised numpy restatement of the ORB front end's stages, written from
the conventions listed at the top of oracle/orc_orb.cpp (whole images at a time, no per-pixel loops, other groupings of
the same integer sums; numpy evaluates every fp32 operation correctly rounded and never contracts), and the
adversarial images both test files run on.  tests/test_orb_ref_cpu.py pins this file to the oracle bit for bit."""
import math

import numpy as np

LEVELS, EDGE, FAST_THR, HALF_PATCH = 8, 19, 20, 15
F32 = np.float32

# the 16 pixels of the radius-3 Bresenham circle in the order that makes "contiguous arc" mean consecutive indices
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
          (-3, 1), (-2, 2), (-1, 3)]


# ---------------------------------------------------------------------------------------------- level sizes and quotas
def level_scales():
    return np.array([math.pow(float(F32(1.2)), l) for l in range(LEVELS)]).astype(F32)


def level_sizes(w, h):
    """(widths, heights, scales): cvRound of the fp32 quotient w / s_l, s_l = (float)pow((double)1.2f, l)."""
    s = level_scales()
    return np.rint(F32(w) / s).astype(np.int32), np.rint(F32(h) / s).astype(np.int32), s


def level_quota(nfeatures):
    """orb.cpp: a geometric series in fp32, each term rounded half to even, the remainder to the last level."""
    factor = F32(1.0 / float(F32(1.2)))
    nd = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(math.pow(float(factor), LEVELS)))
    q = np.zeros(LEVELS, np.int32)
    for l in range(LEVELS - 1):
        q[l] = int(np.rint(nd))
        nd = F32(nd * factor)
    q[-1] = max(nfeatures - int(q[:-1].sum()), 0)
    return q


# ------------------------------------------------------------------------------------------------------------- resize
def _linear_taps(dst, src, clamp_high):
    """Source index and the two 11-bit weights of every destination index (sample position (d + 0.5) * src / dst - 0.5)."""
    f = ((np.arange(dst) + 0.5) * (src / dst) - 0.5).astype(F32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(F32)
    if clamp_high:   # columns: positions outside the row take the border pixel with weight 1
        lo, hi = i < 0, i >= src - 1
        f = np.where(lo | hi, F32(0), f)
        i = np.where(lo, 0, np.where(hi, src - 1, i))
    w0 = np.rint((F32(1) - f) * F32(2048)).astype(np.int16).astype(np.int64)
    w1 = np.rint(f * F32(2048)).astype(np.int16).astype(np.int64)
    return i, w0, w1


def resize(src, dw, dh):
    """OpenCV's 8-bit INTER_LINEAR: horizontal pass in 11-bit weights, vertical pass on the sums >> 4, (.. + 2) >> 2."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    ix, a0, a1 = _linear_taps(dw, sw, True)
    iy, b0, b1 = _linear_taps(dh, sh, False)
    s = src.astype(np.int64)
    rows = s[:, ix] * a0 + s[:, np.minimum(ix + 1, sw - 1)] * a1                       # [sh, dw]
    top, bot = rows[np.clip(iy, 0, sh - 1)], rows[np.clip(iy + 1, 0, sh - 1)]          # [dh, dw]
    v = (((b0[:, None] * (top >> 4)) >> 16) + ((b1[:, None] * (bot >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def pyramid(img):
    img = np.ascontiguousarray(img, np.uint8)
    lw, lh, _ = level_sizes(img.shape[1], img.shape[0])
    out = [img]
    for l in range(1, LEVELS):
        out.append(resize(out[-1], int(lw[l]), int(lh[l])))
    return out


# --------------------------------------------------------------------------------------------------------------- FAST
def fast_score(img, thr=FAST_THR):
    """FAST-9/16 score image: the largest t at which 9 contiguous circle pixels are all > v + t or all < v - t, for the
    pixels of [3, W - 3) x [3, H - 3) that are corners at thr; 0 elsewhere."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    if W < 7 or H < 7:
        return out
    c = img[3:H - 3, 3:W - 3].astype(np.int16)
    d = np.stack([img[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx].astype(np.int16) - c for dx, dy in CIRCLE])
    d = np.concatenate([d, d[:8]])                      # arcs that wrap index 15 -> 0
    brighter = np.full(c.shape, -1000, np.int16)        # the weakest pixel of the best brighter arc
    darker = np.full(c.shape, -1000, np.int16)
    for s in range(16):
        arc = d[s:s + 9]
        brighter = np.maximum(brighter, arc.min(axis=0))
        darker = np.maximum(darker, (-arc).min(axis=0))
    best = np.maximum(brighter, darker)                 # a corner at t  <=>  best > t
    out[3:H - 3, 3:W - 3] = np.where(best > thr, best - 1, 0).astype(np.uint8)
    return out


def nms_flags(score):
    """Strict 3x3 maxima of a score image inside the 19-pixel border."""
    H, W = score.shape
    f = np.zeros((H, W), np.uint8)
    if W < 2 * EDGE + 1 or H < 2 * EDGE + 1:
        return f
    s = score.astype(np.int16)
    c = s[EDGE:H - EDGE, EDGE:W - EDGE]
    ok = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= c > s[EDGE + dy:H - EDGE + dy, EDGE + dx:W - EDGE + dx]
    f[EDGE:H - EDGE, EDGE:W - EDGE] = ok
    return f


def retain_best(scores, quota):
    """retainBest: the cut score; everything at or above the quota-th best score is kept (all ties with it included)."""
    if quota == 0:
        return 256
    if len(scores) <= quota:
        return 0
    return int(np.sort(scores)[::-1][quota - 1])


# --------------------------------------------------------------------------------------------------------------- blur
def gauss7_kernel():
    k = [math.exp(-(i - 3) * (i - 3) / 8.0) for i in range(7)]
    total = 0.0
    for v in k:
        total += v
    return np.array([v / total for v in k]).astype(F32)


def gauss7(img):
    """7-tap sigma-2 separable blur, BORDER_REFLECT_101, fp32 sums in tap order, rows first, round half to even."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    k = gauss7_kernel()
    p = np.pad(img, ((0, 0), (3, 3)), mode="reflect").astype(F32)
    t = np.zeros((H, W), F32)
    for i in range(7):
        t = t + k[i] * p[:, i:i + W]
    p = np.pad(t, ((3, 3), (0, 0)), mode="reflect")
    s = np.zeros((H, W), F32)
    for i in range(7):
        s = s + k[i] * p[i:i + H, :]
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


# -------------------------------------------------------------------------------------------------------- orientation
def umax_table():
    """Half-widths of the rows of the radius-15 disc: rounded circle for the flat rows, the transposed shape for the rest
    (the disc is symmetric under swapping u and v)."""
    u = [int(np.rint(math.sqrt(HALF_PATCH * HALF_PATCH - v * v))) for v in range(HALF_PATCH + 1)]
    vmin = math.ceil(HALF_PATCH * math.sqrt(2.0) / 2)
    for v in range(vmin, HALF_PATCH + 1):
        u[v] = max(x for x in range(vmin) if u[x] >= v)
    return u


def disc_mask():
    um = umax_table()
    v, u = np.mgrid[-HALF_PATCH:HALF_PATCH + 1, -HALF_PATCH:HALF_PATCH + 1]
    return np.abs(u) <= np.array(um)[np.abs(v)], u, v


def moments(img, xs, ys):
    """(m01, m10) of the radius-15 disc around each (x, y): exact integers."""
    img = np.asarray(img, np.uint8).astype(np.int64)
    mask, u, v = disc_mask()
    m01, m10 = np.zeros(len(xs), np.int64), np.zeros(len(xs), np.int64)
    for i, (x, y) in enumerate(zip(xs, ys)):
        p = img[y - HALF_PATCH:y + HALF_PATCH + 1, x - HALF_PATCH:x + HALF_PATCH + 1] * mask
        m01[i], m10[i] = (p * v).sum(), (p * u).sum()
    return m01, m10


def fast_atan2(y, x):
    """OpenCV's fastAtan2 in degrees: 7th-order odd polynomial of min / (max + DBL_EPSILON) in fp32, folded by octant."""
    y, x = np.asarray(y).astype(F32), np.asarray(x).astype(F32)
    scale = F32(180 / math.pi)
    p1, p3, p5, p7 = (F32(c) * scale for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
                                               -0.04432655554792128))
    ax, ay = np.abs(x), np.abs(y)
    eps = F32(2.220446049250313e-16)
    with np.errstate(all="ignore"):
        c = np.where(ax >= ay, ay / (ax + eps), ax / (ay + eps)).astype(F32)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(ax >= ay, a, F32(90) - a)
    a = np.where(x < 0, F32(180) - a, a)
    a = np.where(y < 0, F32(360) - a, a)
    return a.astype(F32)


# ------------------------------------------------------------------------------------------------ whole front end
def stages(img):
    """Per level: (pyramid level, FAST score image, NMS + border flags, blurred level)."""
    return [(p, s, nms_flags(s), gauss7(p)) for p in pyramid(img) for s in [fast_score(p)]]


def keypoints(img, nfeatures, st=None):
    """int64 [n, 4] (x, y, score, level) at level resolution in the output order (level, row, column), and fp32 angles."""
    st = stages(img) if st is None else st
    quota = level_quota(nfeatures)
    rows, angles = [], []
    for l, (p, s, f, _) in enumerate(st):
        ys, xs = np.nonzero(f)                        # raster order
        sc = s[ys, xs].astype(np.int64)
        keep = sc >= retain_best(sc, int(quota[l]))
        xs, ys, sc = xs[keep], ys[keep], sc[keep]
        rows.append(np.stack([xs, ys, sc, np.full(len(xs), l)], axis=1).astype(np.int64))
        m01, m10 = moments(p, xs, ys)
        angles.append(fast_atan2(m01, m10))
    return np.concatenate(rows), np.concatenate(angles).astype(F32)


def kp5(kp, angles):
    """The (x, y in level-0 pixels, angle, response, octave) fp32 rows the front end returns for keypoints()."""
    s = level_scales()[kp[:, 3]]
    return np.stack([kp[:, 0].astype(F32) * s, kp[:, 1].astype(F32) * s, angles, kp[:, 2].astype(F32), kp[:, 3].astype(F32)],
                    axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------- adversarial images
def blocky_noise(w, h, seed, block=6, sigma=5.0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.float32)
    return np.clip(np.kron(base, np.ones((block, block), np.float32))[:h, :w] + rng.normal(0, sigma, (h, w)), 0, 255).astype(np.uint8)


def dot_grid(w, h, step):
    """Black with one saturated pixel every `step`: every dot scores 254, so a whole level ties."""
    img = np.zeros((h, w), np.uint8)
    img[step // 2::step, step // 2::step] = 255
    return img


# (w, h, step, nfeatures): level 0 holds 560 / 176 / 225 tied keypoints against segments of 108 / 72 / 68
DOT_GRIDS = [(256, 192, 8, 100), (160, 120, 8, 20), (128, 128, 6, 8)]


def graded_dots(q, w=128, h=96):
    """q isolated dots of distinct brightness on a 16-pixel grid: level 0 has exactly q strict maxima of distinct scores."""
    img = np.zeros((h, w), np.uint8)
    cells = [(x, y) for y in range(24, h - EDGE, 16) for x in range(24, w - EDGE, 16)]
    assert q <= len(cells)
    for i, (x, y) in enumerate(cells[:q]):
        img[y, x] = 60 + 9 * i
    return img


def put_ring(img, cx, cy, center, values):
    """A flat disc of `center` (radius < 3) with the 16 circle pixels set to `values` (after test_oracle_orb._ring)."""
    H, W = img.shape
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dx * dx + dy * dy <= 5 and 0 <= cx + dx < W and 0 <= cy + dy < H:
                img[cy + dy, cx + dx] = center
    for (dx, dy), v in zip(CIRCLE, values):
        if 0 <= cx + dx < W and 0 <= cy + dy < H:
            img[cy + dy, cx + dx] = v


# name -> (center, ring values, expected score at the centre)
RINGS = {
    "arc9": (100, [160] * 9 + [100] * 7, 59),
    "arc8": (100, [160] * 8 + [100] * 8, 0),
    "contrast20": (100, [120] * 9 + [100] * 7, 0),
    "contrast21": (100, [121] * 9 + [100] * 7, 20),
    "darker9": (100, [100] * 3 + [30] * 9 + [100] * 4, 69),
    "wrap": (100, [40] * 4 + [100] * 7 + [40] * 4 + [55], 44),
    "center0": (0, [0] * 5 + [90] * 9 + [0] * 2, 89),
    "center255": (255, [255] * 7 + [180] * 9, 74),
}
FAST_W, FAST_H = 128, 96


def fast_edges():
    """(image, [(x, y, expected FAST score at (x, y))]): the ring cases in the interior, strong corners on both sides of
    the 3-pixel apron and the x < W - 3 rule, of the 19-pixel border, and of the 16 x 16 tile seams."""
    W, H = FAST_W, FAST_H
    img = np.full((H, W), 100, np.uint8)
    placed = []

    def put(x, y, name):
        c, vals, exp = RINGS[name]
        put_ring(img, x, y, c, vals)
        inside = 3 <= x < W - 3 and 3 <= y < H - 3
        placed.append((x, y, exp if inside else 0))

    for i, name in enumerate(RINGS):                       # the ring cases, interior, 16-pixel grid
        put(24 + 16 * (i % 4), 24 + 16 * (i // 4), name)
    # the apron of the score image: x = 2 / 3 / 4 and W - 5 / W - 4 / W - 3 (and the same in y); rings cut by the image edge
    for x, y in [(3, 30), (4, 46), (W - 4, 30), (W - 3, 46), (2, 62), (W - 5, 62), (90, 3), (106, 4), (90, H - 4), (106, H - 3)]:
        put(x, y, "arc9")
    # the border filter of the flag image: 18 | 19 and W - 20 | W - 19, in x and in y
    for x, y in [(18, 72), (19, 60), (W - 20, 60), (W - 19, 72), (32, 18), (48, 19), (64, H - 20), (90, H - 19)]:
        put(x, y, "arc9")
    # both sides of tile seams (x or y = 31 | 32, 47 | 48, 63 | 64), away from the other rings
    for x, y in [(31, 60), (32, 70), (47, 60), (48, 70), (63, 58), (64, 68), (100, 31), (88, 32), (100, 47), (88, 48),
                 (79, 63), (80, 73)]:
        put(x, y, "arc9")
    for i, a in enumerate(placed):     # no ring touches another one
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 7 for b in placed[:i]), a
    return img, placed


def nms_ties():
    """(image, groups): pixels of equal maximal score next to each other -- a pair, a 2 x 2 block, a diagonal pair -- and one
    isolated dot as the control that survives.  groups: name -> list of (x, y)."""
    img = np.zeros((96, 128), np.uint8)
    groups = {"pair": [(30, 30), (31, 30)], "block": [(60, 30), (61, 30), (60, 31), (61, 31)],
              "diagonal": [(90, 30), (91, 31)], "control": [(40, 60)]}
    for pts in groups.values():
        for x, y in pts:
            img[y, x] = 255
    return img, groups


def extreme_images(w, h):
    """name -> image: what the resize and the blur see at their extremes."""
    yy, xx = np.mgrid[0:h, 0:w]
    lines = np.zeros((h, w), np.uint8)
    lines[[0, 1, h - 2, h - 1], :] = 255
    lines[:, [0, 1, w - 2, w - 1]] = 255
    return {"checker": (((xx + yy) & 1) * 255).astype(np.uint8), "lines": lines, "all255": np.full((h, w), 255, np.uint8),
            "ramp": ((xx * 255) // (w - 1)).astype(np.uint8)}


def angle_dots():
    """Isolated dots (moments 0) and dots with one dimmer neighbour 6 pixels away on each axis and each diagonal."""
    img = np.zeros((200, 320), np.uint8)
    centres = {}
    img[40, 40] = 255
    centres["isolated"] = (40, 40)
    for i, (dx, dy) in enumerate([(6, 0), (0, 6), (-6, 0), (0, -6), (6, 6), (-6, 6), (-6, -6), (6, -6)]):
        x, y = 40 + 64 * (i % 4), 100 + 56 * (i // 4)
        img[y, x] = 255
        img[y + dy, x + dx] = 128
        centres[(dx, dy)] = (x, y)
    return img, centres


def one_sided_patch():
    """A bright rectangle on black: its corners are keypoints on several levels, each with the bright side on one side."""
    img = np.zeros((240, 320), np.uint8)
    img[70:170, 90:230] = 200
    return img


def nf_for_level0_quota(q):
    """The smallest nfeatures whose level-0 quota is q."""
    return next(nf for nf in range(1, 100 * (q + 1)) if level_quota(nf)[0] == q)


GRADED_Q = 12
# Level widths where the fp32 quotient rounds to another integer than exact arithmetic (w / 1.2^l = k + 0.5 exactly, the
# fp32 scale puts it just below): 129 -> 107 and 141 -> 117 at level 1 (exact: 108, 118), 324 -> 187 at level 3 (188),
# 237 -> 197 at level 1 (198).  Found by sweeping w over 64..700.  The same sweep finds NO width at which
# (int)floor((dx + .5) * scale - .5) reaches sw - 1 in the last column: the ratio of consecutive levels stays above 1, so
# the last sample position is sw - 0.5 * scale - 0.5 < sw - 1.  That clamp is only reachable when enlarging, which the
# CPU test does on the resize alone.
EXTREME_SIZES = [(129, 141), (324, 237)]
BIG_W, BIG_H = 1024, 1100   # rows >= 1024 lie in chunks >= 1024 of level 0: the scan kernel's second trip, and 19 < 1100 - 1024


def small_cases():
    """(name, image, nfeatures) of every adversarial image up to 752 x 480."""
    for w, h, step, nf in DOT_GRIDS:
        yield "dots%dx%d" % (w, h), dot_grid(w, h, step), nf
    for dq in (0, -1, 5):
        yield "graded_q%+d" % dq, graded_dots(GRADED_Q), nf_for_level0_quota(GRADED_Q + dq)
    for nf in (1, 2, 4, 5, 8):   # quotas with zeros; 200 x 160 keeps level 7 (56 x 45) wider than the border
        yield "noise200x160_nf%d" % nf, blocky_noise(200, 160, 360), nf
    yield "noise100x81_nf50000", blocky_noise(100, 81, 181), 50000
    yield "fast_edges", fast_edges()[0], 500
    yield "nms_ties", nms_ties()[0], 500
    for w, h in EXTREME_SIZES:
        for name, img in extreme_images(w, h).items():
            yield "%s%dx%d" % (name, w, h), img, 500
    yield "angle_dots", angle_dots()[0], 500
    yield "one_sided_patch", one_sided_patch(), 500
    yield "noise333x251", blocky_noise(333, 251, 584), 1000
    yield "noise64x64", blocky_noise(64, 64, 128), 8
    yield "noise640x480", blocky_noise(640, 480, 1120), 1000
    yield "noise752x480", blocky_noise(752, 480, 1232), 1500


def large_cases():
    yield "noise1280x720", blocky_noise(1280, 720, 2000), 4000
    yield "noise%dx%d" % (BIG_W, BIG_H), blocky_noise(BIG_W, BIG_H, 2124), 20000
