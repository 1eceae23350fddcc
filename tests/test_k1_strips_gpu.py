"""GPU parity of the response kernel's strip walk (detect.hip min_eig_response_kernel) against the oracle, where the
tall strips, the mid-strip list flush and the border-only maximum are most likely to break.

The batch kernel walks strips of ROWS rows x 60 columns, four per workgroup; a wave drains its 384-slot LDS candidate
list into the image's global list whenever fewer than 96 slots are left at a check (once per six rows), and takes the
image maximum over the emitted candidates plus the pixels of row 0, row h - 1, column 0 and column w - 1 only.  So:
heights around the strip seams, widths around the 60-column strips, launches on the plain grid (1 and 7 images) and on
the XCD-dealt grid with and without a padded tail (8 and 9), and images that fill the list (noise), have no corner at
all (constant), hold their maximum on a plateau (checkerboards; the 3-px one is one plateau over the whole image and
outruns the flush checks, so it takes the direct global append), or hold it on row 0, on column w - 1 and on the rows
next to a strip seam.  Every input property is checked on the CPU (oracle + numpy) before the GPU is asked.

Compared exactly: the keypoints, the image maximum the selection stage used (bit pattern, whenever it is positive;
<= 0 on both sides otherwise) and the response image through the parity hook.  The device's candidate count depends on
where the early quality cuts fall, so it is checked against the two oracle counts that bracket it: every candidate
above the quality threshold must be listed, and nothing but provisional candidates (positive 3 x 3 maxima) can be."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 120            # K1_ROWS of detect.hip
K1_WLIST = 384        # LDS candidate slots per wave
HEIGHTS = [ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 3, 480]
WIDTHS = [61, 64, 121, 752]
LAUNCHES = [1, 7, 8, 9]
NF = 1500
ROW0_SEED, COLW_SEED, SEAM_SEED = 23, 2, 5   # patches whose largest response lies where the case wants it (asserted)


def patch(seed):
    return (np.random.default_rng(seed).integers(0, 2, (6, 6)) * 215 + 40).astype(np.uint8)


def patch_image(w, h, seed, y0, x0):
    """One high-contrast 6 x 6 patch with its top-left pixel at (y0, x0) on a constant image."""
    img = np.full((h, w), 40, np.uint8)
    img[y0:y0 + 6, x0:x0 + 6] = patch(seed)
    return img


def argmax2(r):
    return tuple(int(v) for v in np.unravel_index(np.argmax(r), r.shape))


def patch_image_with_maximum_at(orc, w, h, seed, ty, tx):
    """The response of a patch far from the border moves with the patch: find its maximum once, then shift."""
    dy, dx = argmax2(orc.min_eig_response(patch_image(40, 40, seed, 17, 17)))
    return patch_image(w, h, seed, ty - (dy - 17), tx - (dx - 17))


def block_image(seed, w, h):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8)).astype(np.float32)
    img = np.kron(base, np.ones((8, 8), np.float32))[:h, :w]
    return np.clip(img + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def checker(w, h, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // b) + (xx // b)) % 2 * 200 + 20).astype(np.uint8)


def seam_rows(h):
    """(row just above the first seam, row just below the last seam) of an image with a seam far enough from its
    border; two neighbouring rows in the middle of a one-strip image."""
    if h >= ROWS + 8:
        return ROWS - 1, (h - 8) // ROWS * ROWS
    return h // 2 - 1, h // 2


def provisional(r):
    """Positive 3 x 3 maxima off the outermost pixels: what the response kernel may list."""
    p = np.pad(r, 1, constant_values=-np.inf)
    dil = np.max([p[dy:dy + r.shape[0], dx:dx + r.shape[1]] for dy in range(3) for dx in range(3)], axis=0)
    keep = (r == dil) & (r > 0)
    keep[0, :] = keep[-1, :] = keep[:, 0] = keep[:, -1] = False
    return keep


def case_images(orc, synth, w, h):
    above, below = seam_rows(h)
    imgs = {
        "noise": np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8),
        "flat": np.full((h, w), 90, np.uint8),
        "checker16": checker(w, h, 16),
        "row0": patch_image(w, h, ROW0_SEED, 0, 28),
        "colw": patch_image(w, h, COLW_SEED, 48, w - 6),
        "above_seam": patch_image_with_maximum_at(orc, w, h, SEAM_SEED, above, 30),
        "below_seam": patch_image_with_maximum_at(orc, w, h, SEAM_SEED, below, 30),
    }
    if (w, h) == (752, 480):   # one stereo frame of the generator bench.py times
        pair = synth.stereo_pair_variants(7000, 1, margin=24)[0]
        imgs["stereo_left"], imgs["stereo_right"] = pair[0], pair[1]
    else:
        imgs["blocks"] = block_image(w + h, w, h)
        # the 3-px checkerboard's response is one plateau: every pixel is listed, 60 per row step
        imgs["checker3" if w * h <= 32768 else "blocks2"] = checker(w, h, 3) if w * h <= 32768 else block_image(w * h, w, h)
    return imgs


def oracle_facts(orc, img):
    r = orc.min_eig_response(img)
    prov = provisional(r)
    thr = np.float32(np.float64(r.max()) * 0.01)
    return dict(r=r, max=r.max(), prov=prov, n_prov=int(prov.sum()), n_above=int((prov & (r > thr)).sum()),
                xy=orc.detect_describe(img, NF, True)[0])


def check_input_properties(name, img, f, w, h):
    r, m = f["r"], f["r"] == f["max"]
    if name == "noise":       # more candidates in the first strip than its list holds: the mid-strip flush fires
        assert f["prov"][:ROWS, :61].sum() > K1_WLIST and f["n_above"] > K1_WLIST
    elif name == "flat":
        assert f["max"] <= 0 and f["n_prov"] == 0
    elif name == "checker16":   # the maximum sits on plateaus: neighbouring pixels hold it
        assert f["max"] > 0 and ((m[:, 1:] & m[:, :-1]).any() or (m[1:, :] & m[:-1, :]).any())
    elif name == "checker3":    # one plateau: more candidates in six rows of a strip than the flush check leaves room for
        assert m.sum() > 0.9 * w * h and f["prov"][1:7, :61].sum() > K1_WLIST // 2
    elif name == "row0":
        assert m.sum() == 1 and argmax2(r)[0] == 0
    elif name == "colw":
        assert m.sum() == 1 and argmax2(r)[1] == w - 1
    elif name in ("above_seam", "below_seam"):
        above, below = seam_rows(h)
        assert m.sum() == 1 and argmax2(r) == (above if name == "above_seam" else below, 30)


def check_slot(fr, slot, n, name, f, counts, maxima):
    xy = fr.keypoints(slot)[0]
    assert np.array_equal(xy, f["xy"]), (name, n, slot)
    assert f["n_above"] <= counts[slot] <= f["n_prov"], (name, n, slot, f["n_above"], int(counts[slot]), f["n_prov"])
    if f["max"] > 0:
        assert maxima[slot:slot + 1].view(np.uint32)[0] == np.array([f["max"]], np.float32).view(np.uint32)[0], (name, n, slot)
    else:
        assert maxima[slot] <= 0, (name, n, slot)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_strip_seams_launch_sizes_and_image_kinds(ctx, orc, vsl, synth, w, h):
    imgs = case_images(orc, synth, w, h)
    names = list(imgs)
    facts = {k: oracle_facts(orc, v) for k, v in imgs.items()}
    for k in names:
        check_input_properties(k, imgs[k], facts[k], w, h)
    assert len(names) == max(LAUNCHES)
    fr = vsl.Frames(ctx, len(names), w, h, NF)
    try:
        for shift, n in enumerate(LAUNCHES):   # another image in every slot each time: a stale result cannot pass
            order = names[shift:] + names[:shift]
            fr.upload(0, np.stack([imgs[k] for k in order]))
            fr.detect_describe(0, n, NF, True)
            fr.resolve_ties()
            counts, maxima = fr.candidate_counts(n), fr.response_max(n)
            for slot in range(n):
                check_slot(fr, slot, n, order[slot], facts[order[slot]], counts, maxima)
            if "noise" in order[:n]:
                assert counts[order.index("noise")] > K1_WLIST
    finally:
        fr.close()
    # the response image itself, through the parity hook (same strips, one image)
    for k in names:
        assert np.array_equal(ctx.min_eig_response(imgs[k]).view(np.uint32), facts[k]["r"].view(np.uint32)), k


@pytest.mark.parametrize("cap", [0, 16])
def test_short_lists_flush_and_overflow_in_a_batch(ctx, orc, vsl, synth, cap):
    """A list of `cap` slots (k1_list_cap): with 16 every group of six rows that found a candidate ends in a flush, and
    the noise image lists more than 16 in such a group, so the direct append runs in between; with 0 every candidate
    takes the direct append and every flush is empty."""
    w, h = 121, 2 * ROWS + 3
    imgs = case_images(orc, synth, w, h)
    names = list(imgs)[:8]
    facts = {k: oracle_facts(orc, imgs[k]) for k in names}
    assert facts["noise"]["prov"][6:12, :61].sum() > 16   # candidate rows of the strip's second group of six steps
    fr = vsl.Frames(ctx, 8, w, h, NF)
    ctx.set_diagnostic("k1_list_cap", cap)
    try:
        fr.upload(0, np.stack([imgs[k] for k in names]))
        fr.detect_describe(0, 8, NF, True)
        fr.resolve_ties()
        counts, maxima = fr.candidate_counts(8), fr.response_max(8)
        for slot, k in enumerate(names):
            check_slot(fr, slot, 8, k, facts[k], counts, maxima)
    finally:
        ctx.set_diagnostic("k1_list_cap", -1)
        fr.close()
