"""CPU: tests/orb_ref.py, the numpy restatement of the ORB front end's stages that tests/test_orb_gpu.py compares the
kernels' stage images with, is pinned bit for bit to oracle/orc_orb.cpp on the adversarial images of that file.  Two
independent statements of the conventions agreeing on these inputs is also the check of the oracle itself."""
import numpy as np
import pytest

import orb_ref as R

SMALL = list(R.small_cases())
LARGE = list(R.large_cases())
IDS = [c[0] for c in SMALL + LARGE]


def test_level_sizes_and_quotas(orc):
    for w, h in [(64, 64), (100, 81), (752, 480), (1280, 720), (R.BIG_W, R.BIG_H)] + R.EXTREME_SIZES:
        lw, lh, sc = orc.orb_level_sizes(w, h)
        rw, rh, rs = R.level_sizes(w, h)
        assert np.array_equal(lw, rw) and np.array_equal(lh, rh) and np.array_equal(sc.view(np.uint32), rs.view(np.uint32))
    for nf in (1, 2, 4, 5, 8, 20, 100, 500, 1000, 1500, 4000, 20000, 50000):
        assert np.array_equal(orc.orb_level_quota(nf), R.level_quota(nf))


@pytest.mark.parametrize("name,img,nf", SMALL + LARGE, ids=IDS)
def test_resize_and_blur_equal_the_oracle(orc, name, img, nf):
    pyr = R.pyramid(img)
    for l in range(1, R.LEVELS):
        h, w = pyr[l].shape
        assert np.array_equal(pyr[l], orc.orb_resize(pyr[l - 1], w, h)), (name, l)
    for l in (0, 1, 4, 7):
        assert np.array_equal(R.gauss7(pyr[l]), orc.orb_gauss7(pyr[l])), (name, l)


def test_resize_clamps_when_enlarging(orc):
    # the pyramid never reaches the sx >= sw - 1 clamp (orb_ref.EXTREME_SIZES); enlarging and extreme ratios do
    img = R.blocky_noise(37, 29, 66, block=2)
    for dw, dh in [(53, 41), (37, 29), (74, 58), (36, 28), (5, 3), (111, 30)]:
        assert np.array_equal(R.resize(img, dw, dh), orc.orb_resize(img, dw, dh)), (dw, dh)


@pytest.mark.parametrize("name,img,nf", SMALL, ids=IDS[:len(SMALL)])
def test_fast_score_equals_the_oracle_at_every_pixel(orc, name, img, nf):
    if img.shape[0] * img.shape[1] > 130 * 150:
        img = img[:96, :128]          # every pixel through the oracle's per-pixel entry: keep the images small
    for lvl in R.pyramid(img)[::3]:
        h, w = lvl.shape
        exp = np.array([[orc.orb_fast_score(lvl, x, y) for x in range(w)] for y in range(h)], np.uint8)
        assert np.array_equal(R.fast_score(lvl), exp), name


@pytest.mark.parametrize("name,img,nf", SMALL + LARGE, ids=IDS)
def test_keypoints_equal_the_oracle(orc, name, img, nf):
    kp, ang = R.keypoints(img, nf)
    okp, _ = orc.orb_detect_describe(img, nf)
    # (x, y, score, level) as the set the issue asks for, then order, coordinates and angles bit for bit
    sc = R.level_scales()
    oset = {(int(np.rint(k[0] / sc[int(k[4])])), int(np.rint(k[1] / sc[int(k[4])])), int(k[3]), int(k[4])) for k in okp}
    assert {tuple(r) for r in kp.tolist()} == oset
    assert len(kp) == len(okp)
    assert np.array_equal(R.kp5(kp, ang).view(np.uint32), okp.view(np.uint32))


def test_umax_table_is_the_published_one():
    assert R.umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_oracle_wrapper_returns_every_tie(orc):
    # 619 keypoints against num_features = 100: the wrapper's first buffer (264) must not cut them
    w, h, step, nf = R.DOT_GRIDS[0]
    okp, odesc = orc.orb_detect_describe(R.dot_grid(w, h, step), nf)
    assert len(okp) == 619 == len(odesc) and int((okp[:, 4] == 0).sum()) == 560 and np.all(okp[okp[:, 4] == 0, 3] == 254)
