"""GPU parity of the corner-selection kernel's shortened chain (detect.hip select_kernel) against the oracle.

The kernel reads a candidate list of at most SEL_CHUNK keys once and keeps it in registers through the counting sort,
ranks the pixel positions straight to their final place (behind the keys up to SEL_CHUNK / 2 candidates, over them
beyond), counts accepted corners and accepted corners inside the output border in one packed scan per greedy batch,
and decides the cut at num_features from that scan.  Each case below puts one of those paths under the smallest image
that reaches it; that an image really lies in its regime (candidate count, fullest response bin, where the cap
falls, which corners lie in the border) is asserted on the CPU, from the oracle and numpy alone, so a case cannot
pass by missing its path.  The expected keypoints are always the oracle's, in order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEL_CHUNK = 8192      # keys sorted at once (and held in registers, eight per thread)
SEL_THREADS = 1024    # ranks per greedy batch
SEL_BINS = 1024       # response bins of the counting sort
SEL_MAX_CELLS = 6144  # 8 x 8 cells (with the empty ring) of the LDS variant
BUCKET_CAP = 128      # fullest bin the counting sort accepts (the default of the "select_bucket_cap" knob)
BORDER = 19
W, H = 96, 64


def lattice_image(seed, w=W, h=H, sigma=6.0, amp=40.0):
    """Dense random texture: a period-4 wave in x and in y (its squared gradients have period 2, so the response has
    a local maximum on almost every second pixel in both directions) under Gaussian noise that makes every response
    distinct.  sigma = 0: the bare wave, whose responses repeat exactly."""
    rng = np.random.default_rng(seed)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    img = 128 + amp * (np.sin(np.pi * x / 2) + np.sin(np.pi * y / 2))
    if sigma:
        img = img + rng.normal(0, sigma, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def block_image(seed, w, h, block=8, sigma=6.0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.float32)
    img = np.kron(base, np.ones((block, block), np.float32))[:h, :w]
    return np.clip(img + rng.normal(0, sigma, (h, w)), 0, 255).astype(np.uint8)


def ranked_candidates(orc, img):
    """Local 3 x 3 maxima of the response above the quality threshold, best first (ties: the later pixel first, as
    the reference sorts): the selection kernel's input after its threshold."""
    r = orc.min_eig_response(img)
    h, w = r.shape
    thr = np.float32(np.float64(r.max()) * 0.01)
    p = np.pad(r, 1, constant_values=-np.inf)
    dil = np.max([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    keep = (r == dil) & (r > thr)
    keep[0, :] = keep[-1, :] = keep[:, 0] = keep[:, -1] = False
    ys, xs = np.nonzero(keep)
    order = np.lexsort((-(ys * w + xs), -r[ys, xs].astype(np.float64)))
    return xs[order], ys[order], r[ys, xs][order]


def fullest_bin(r):
    """Occupancy of the fullest bin of the kernel's counting sort: SEL_BINS bins on the top bits of the (positive)
    response's bit pattern between the threshold and the maximum, the shift chosen as the kernel chooses it."""
    bits = r.view(np.uint32).astype(np.int64)
    hi_max = int(bits.max())
    hi_floor = int(np.float32(np.float64(r.max()) * 0.01).view(np.uint32))
    shift = 16
    while shift < 31 and (hi_max >> shift) - (hi_floor >> shift) >= SEL_BINS:
        shift += 1
    return int(np.bincount((hi_max >> shift) - np.minimum(bits >> shift, hi_max >> shift)).max())


def regime(orc, img):
    """Candidate count, fullest bin, and the ranks (positions in the sorted candidate list) of the corners the
    reference's greedy loop accepts when nothing caps it, with whether each lies inside the output border."""
    xs, ys, r = ranked_candidates(orc, img)
    rank = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(xs, ys))}
    acc = orc.good_features(img, 0)
    h, w = img.shape
    inside = (acc[:, 0] >= BORDER) & (acc[:, 0] < w - BORDER) & (acc[:, 1] >= BORDER) & (acc[:, 1] < h - BORDER)
    return dict(n=len(xs), fullest=fullest_bin(r) if len(xs) else 0,
                acc_rank=np.array([rank[(int(x), int(y))] for x, y in acc], np.int64), inside=inside)


def cells_of(w, h):
    return (((w + 7) // 8 + 2) * ((h + 7) // 8 + 2) + 1) & ~1


def ring_image():
    """Texture along the edges only: every corner lies within BORDER of an edge."""
    img = lattice_image(3, sigma=12.0)
    img[16:48, 16:80] = 128
    return img


def centre_image():
    """Texture in the middle only: no corner lies within BORDER of an edge."""
    img = np.full((H, W), 128, np.uint8)
    img[22:42, 22:74] = lattice_image(3, sigma=12.0)[22:42, 22:74]
    return img


def plateau_image():
    """The bare wave (its responses repeat exactly: hundreds of equal keys in one bin) with one noisy corner."""
    img = lattice_image(0, sigma=0.0)
    img[:16, :16] = lattice_image(5, sigma=10.0)[:16, :16]
    return img


DENSE_SEED = 1


@pytest.fixture(scope="module")
def dense(orc):
    img = lattice_image(DENSE_SEED)
    return img, regime(orc, img)


def check(ctx, orc, img, nf):
    want = orc.detect_keypoints(img, nf)
    got = ctx.detect_keypoints(img, nf)
    assert np.array_equal(got, want), (len(got), len(want))
    return want


def test_dense_small_image_two_batches(ctx, orc, dense):
    """More than one key per thread in registers (ranked behind the keys), and two greedy batches, both accepting."""
    img, p = dense
    print(p["n"], p["fullest"], len(p["acc_rank"]))
    assert SEL_THREADS < p["n"] <= 2 * SEL_THREADS and p["fullest"] <= BUCKET_CAP
    assert (p["acc_rank"] < SEL_THREADS).any() and (p["acc_rank"] >= SEL_THREADS).sum() >= 2
    assert p["inside"].any() and not p["inside"].all()
    want = check(ctx, orc, img, 1500)             # no cut: fewer corners exist than are asked for
    assert len(want) == int(p["inside"].sum()) > 0


@pytest.mark.parametrize("where", ["inside_second_batch", "on_batch_boundary", "inside_first_batch"])
def test_cap_position(ctx, orc, dense, where):
    """The cut at num_features from the packed scan: strictly inside the second batch (corners of that batch are
    accepted on both sides of the cut), exactly at the end of the first batch (the batch's accepted total equals what
    is left: nothing is cut, and the second batch must not run), and inside the first batch."""
    img, p = dense
    a1, a = int((p["acc_rank"] < SEL_THREADS).sum()), len(p["acc_rank"])
    nf = {"inside_second_batch": a1 + (a - a1) // 2, "on_batch_boundary": a1, "inside_first_batch": a1 // 2}[where]
    if where == "inside_second_batch":
        assert a1 < nf < a
    kept_inside = p["inside"][:nf]
    assert kept_inside.any() and not kept_inside.all() and not p["inside"][nf:].all()   # the cut shows in the output
    want = check(ctx, orc, img, nf)
    assert len(want) == int(kept_inside.sum())


@pytest.mark.parametrize("name", ["ring", "centre"])
def test_border_all_or_nothing(ctx, orc, name):
    """Every accepted corner outside the output border (the second half of the packed count stays zero: no
    keypoint), and every accepted corner inside it (both halves equal)."""
    img = ring_image() if name == "ring" else centre_image()
    p = regime(orc, img)
    assert len(p["acc_rank"]) >= 10 and p["fullest"] <= BUCKET_CAP
    assert not p["inside"].any() if name == "ring" else p["inside"].all()
    want = check(ctx, orc, img, 1500)
    assert len(want) == (0 if name == "ring" else len(p["acc_rank"]))
    check(ctx, orc, img, 5)                        # and with a cut


def test_plateau_takes_the_bitonic_path(ctx, orc):
    img = plateau_image()
    p = regime(orc, img)
    print(p["n"], p["fullest"])
    assert SEL_THREADS < p["n"] <= 2 * SEL_THREADS and p["fullest"] > BUCKET_CAP
    assert (p["acc_rank"] >= SEL_THREADS).any()
    check(ctx, orc, img, 1500)
    check(ctx, orc, img, int((p["acc_rank"] < SEL_THREADS).sum()) + 1)


def test_more_than_half_a_chunk_of_candidates(ctx, orc):
    """Between SEL_CHUNK / 2 and SEL_CHUNK candidates on the counting-sort path: the ranked positions overwrite the
    keys, so each thread carries them in registers across a barrier (up to six keys per thread here)."""
    img = lattice_image(2, 192, 128, sigma=20.0)
    p = regime(orc, img)
    print(p["n"], p["fullest"])
    assert SEL_CHUNK // 2 < p["n"] <= SEL_CHUNK and p["fullest"] <= BUCKET_CAP
    a = len(p["acc_rank"])
    assert (p["acc_rank"] >= 4 * SEL_THREADS).any()
    check(ctx, orc, img, 1500)
    check(ctx, orc, img, a - 3)


@pytest.mark.parametrize("case", ["one_chunk", "chunks"])
def test_global_grid_variant(ctx, orc, case):
    """An image with more than SEL_MAX_CELLS cells keeps the grid in global memory: once with a candidate list that
    stays in registers (the grid is initialised before the sort there), once with more than SEL_CHUNK candidates."""
    w, h = 1024, 768
    assert cells_of(w, h) > SEL_MAX_CELLS
    img = block_image(7, w, h, 16, 2.0) if case == "one_chunk" else block_image(7, w, h, 8, 6.0)
    xs, _, r = ranked_candidates(orc, img)
    print(len(xs), fullest_bin(r))
    if case == "one_chunk":
        assert SEL_THREADS < len(xs) <= SEL_CHUNK and fullest_bin(r) <= BUCKET_CAP
    else:
        assert len(xs) > SEL_CHUNK
    want = check(ctx, orc, img, 60)
    assert 0 < len(want) < 60                      # sixty accepted, some of them in the border


def test_provisional_list_longer_than_a_chunk(ctx, orc, vsl):
    """Low-contrast noise with one high-contrast patch: the response kernel's per-workgroup early cut lets more than
    SEL_CHUNK provisional candidates through, the image-wide threshold leaves a few hundred.  That list does not fit
    the registers, so the counting sort reads it from memory twice, as it always did."""
    rng = np.random.default_rng(9)
    img = (128 + rng.integers(-12, 13, (480, 752))).astype(np.uint8)
    img[200:232, 300:332] = rng.integers(0, 256, (32, 32))
    xs, _, r = ranked_candidates(orc, img)
    assert 0 < len(xs) <= SEL_CHUNK and fullest_bin(r) <= BUCKET_CAP
    fr = vsl.Frames(ctx, 1, 752, 480, 1500, max_pairs=1)
    try:
        fr.upload(0, img)
        fr.detect_describe(0, 1, 1500, True)
        fr.resolve_ties()
        got = fr.keypoints(0)[0]
        assert fr.candidate_counts(1)[0] > SEL_CHUNK   # the device's own count of provisional candidates
    finally:
        fr.close()
    assert np.array_equal(got, orc.detect_keypoints(img, 1500))


def test_nine_images_in_one_launch(ctx, orc, vsl):
    """Nine small images of every regime above in one launch, in nine launches of one, and from the oracle."""
    imgs = [lattice_image(s) for s in (0, 1, 2, 3)] + [plateau_image(), ring_image(), centre_image()] + \
           [lattice_image(s) for s in (4, 5)]
    nf = 64                                        # cuts the dense images (in their first or second batch), not the others
    want = [orc.detect_keypoints(im, nf) for im in imgs]
    assert any(len(x) == 0 for x in want) and sum(len(x) > 0 for x in want) >= 7
    one, nine = vsl.Frames(ctx, 1, W, H, 128, max_pairs=1), vsl.Frames(ctx, 9, W, H, 128, max_pairs=1)
    try:
        nine.upload(0, np.stack(imgs))
        nine.detect_describe(0, 9, nf, True)
        nine.resolve_ties()
        together = [nine.keypoints(s)[0] for s in range(9)]
        alone = []
        for im in imgs:
            one.upload(0, im)
            one.detect_describe(0, 1, nf, True)
            one.resolve_ties()
            alone.append(one.keypoints(0)[0])
    finally:
        one.close()
        nine.close()
    for s in range(9):
        assert np.array_equal(together[s], want[s]), s
        assert np.array_equal(alone[s], want[s]), s
