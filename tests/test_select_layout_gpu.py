"""GPU parity of the corner-selection kernel's packed LDS layout (detect.hip select_kernel) against the oracle.

The kernel keeps an accepted corner as the low three bits of x and y in a byte of its 8 x 8-px cell (two slots = one
u16 per cell) and a cell's batch list head as a u16 rank, two cells per 32-bit word.  These cases single out what
that layout could break: corners on the last column / row and cells with both slots taken, the largest image the LDS
variant takes and the first one of the global-grid variant, the last rank of a batch taking part in the blocker
lists, and grid state that crosses a chunk boundary.  Every input property is checked on the CPU (oracle + numpy)
before the GPU is asked; the expected value is always the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 752, 480
SEL_CHUNK = 8192      # keys sorted at once
SEL_THREADS = 1024    # ranks per greedy batch
SEL_MAX_CELLS = 6144  # 8 x 8 cells (with the empty ring) of the LDS variant


def noise_image(seed, w=W, h=H):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def block_image(seed, w=W, h=H, sigma=6):
    """Random 8 x 8 blocks plus noise (the images of test_odd_image_sizes): a few thousand candidates."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8)).astype(np.float32)
    img = np.kron(base, np.ones((8, 8), np.float32))[:h, :w]
    return np.clip(img + rng.normal(0, sigma, (h, w)), 0, 255).astype(np.uint8)


def edged_block_image(seed):
    """block_image with 16-px strips of noise along the right and bottom edges: corners on the last column and row
    that can hold one, with no more than SEL_CHUNK candidates in all."""
    img, n = block_image(seed), noise_image(seed + 100)
    img[:, -16:] = n[:, -16:]
    img[-16:, :] = n[-16:, :]
    return img


def ranked_candidates(orc, img):
    """Local 3 x 3 maxima of the response above the quality threshold, best first: the selection kernel's input."""
    r = orc.min_eig_response(img)
    thr = np.float32(np.float64(r.max()) * 0.01)
    p = np.pad(r, 1, constant_values=-np.inf)
    dil = np.max([p[dy:dy + r.shape[0], dx:dx + r.shape[1]] for dy in range(3) for dx in range(3)], axis=0)
    keep = (r == dil) & (r > thr)
    keep[0, :] = keep[-1, :] = keep[:, 0] = keep[:, -1] = False   # goodFeaturesToTrack does not look at the outermost pixels
    ys, xs = np.nonzero(keep)
    order = np.argsort(-r[ys, xs].astype(np.float64), kind="stable")
    return xs[order], ys[order], r[ys, xs][order]


def cells_of(w, h):
    return (((w + 7) // 8 + 2) * ((h + 7) // 8 + 2) + 1) & ~1


def full_cells(xy):
    """Number of 8 x 8 cells that hold two accepted corners."""
    _, counts = np.unique((xy[:, 1] >> 3) * 4096 + (xy[:, 0] >> 3), return_counts=True)
    return int((counts >= 2).sum())


def same_as_oracle(ctx, orc, img, nf):
    xy, ang, desc = ctx.detect_describe(img, nf, True)
    oxy, oang, odesc = orc.detect_describe(img, nf, True)
    assert len(oxy) > 0
    return np.array_equal(xy, oxy) and np.array_equal(ang.view(np.uint64), oang.view(np.uint64)) and np.array_equal(desc, odesc)


# (image, number of features): one image on the counting-sort path, one beyond SEL_CHUNK candidates
EDGE_CASES = {"blocks": (lambda: edged_block_image(0), 1500), "noise": (lambda: noise_image(0), 1500)}


def edge_case_properties(orc, name):
    make, nf = EDGE_CASES[name]
    img = make()
    acc = orc.good_features(img, nf)   # the first nf accepted corners, border ring included: what fills the grid
    n_cand = len(ranked_candidates(orc, img)[0])
    return img, nf, dict(n_cand=n_cand, accepted=len(acc), last_col=int((acc[:, 0] == W - 2).sum()),
                         last_row=int((acc[:, 1] == H - 2).sum()), full_cells=full_cells(acc))


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_last_column_last_row_and_full_cells(ctx, orc, name):
    """Corners accepted at x = 750 and y = 478, the last column and row that can hold one (goodFeaturesToTrack, and
    so the oracle and the response kernel, never takes the outermost pixels 751 / 479: no input produces a corner
    there).  They lie outside the 19-px output border, but they count towards num_features and fill the last
    real cells next to the empty ring.  Also cells with both slots taken."""
    img, nf, p = edge_case_properties(orc, name)
    print(name, p)
    assert p["accepted"] == nf          # the cut at num_features is live: one wrong decision anywhere shifts the output
    assert p["last_col"] > 0 and p["last_row"] > 0 and p["full_cells"] > 0
    assert (p["n_cand"] <= SEL_CHUNK) == (name == "blocks")
    assert same_as_oracle(ctx, orc, img, nf)


@pytest.mark.parametrize("w,h,in_lds", [(752, 496, True), (752, 497, False)])
def test_largest_lds_grid_and_first_global_grid(ctx, orc, w, h, in_lds):
    assert cells_of(w, h) == SEL_MAX_CELLS if in_lds else cells_of(w, h) > SEL_MAX_CELLS
    assert cells_of(w, h - 1) <= SEL_MAX_CELLS
    img = block_image(7, w, h)
    acc = orc.good_features(img, 0)
    assert (acc[:, 1] >= h - 8).any() and (acc[:, 0] >= w - 8).any()   # the last row and column of cells are used
    assert same_as_oracle(ctx, orc, img, 1500)
    assert same_as_oracle(ctx, orc, noise_image(11, w, h), 3000)        # and with more than one chunk


LAST_RANK_IMAGE = lambda: block_image(3)  # noqa: E731


def last_rank_properties(orc):
    img = LAST_RANK_IMAGE()
    xs, ys, r = ranked_candidates(orc, img)
    k = SEL_THREADS - 1
    d2 = (xs[:k].astype(np.int64) - xs[k]) ** 2 + (ys[:k].astype(np.int64) - ys[k]) ** 2
    return img, dict(n_cand=len(xs), neighbours_above=int((d2 < 64).sum()), tie=bool(r[k - 1] == r[k] or r[k] == r[k + 1]))


def test_last_rank_of_a_batch_in_the_blocker_lists(ctx, orc):
    """Rank 1023 of the first batch (no corner accepted yet, so every rank survives the grid test) has higher-ranked
    candidates of its batch within the minimum distance: its rank (all ten bits set) is a list head / list
    member while its blockers are collected, and it waits for them.  (Blockers are HIGHER-ranked members of a batch,
    so 1023 itself is never stored as one; 1022 is the largest blocker id, 1023 the largest list entry.)"""
    img, p = last_rank_properties(orc)
    print(p)
    assert SEL_THREADS < p["n_cand"] <= SEL_CHUNK and p["neighbours_above"] > 0 and not p["tie"]
    assert same_as_oracle(ctx, orc, img, 1500)


def chunk_crossing_properties(orc, img, nf):
    xs, ys, _ = ranked_candidates(orc, img)
    acc = orc.good_features(img, nf)
    rank = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(xs, ys))}
    acc_rank = np.array([rank.get((int(x), int(y)), -1) for x, y in acc])
    first = acc[(acc_rank >= 0) & (acc_rank < SEL_CHUNK)].astype(np.int64)
    # candidates of a later chunk that lie within the minimum distance of a corner accepted in the first chunk
    lx, ly = xs[SEL_CHUNK:].astype(np.int64), ys[SEL_CHUNK:].astype(np.int64)
    blocked = 0
    for i in range(0, len(lx), 512):
        d2 = (lx[i:i + 512, None] - first[None, :, 0]) ** 2 + (ly[i:i + 512, None] - first[None, :, 1]) ** 2
        blocked += int((d2 < 64).any(axis=1).sum())
    return dict(n_cand=len(xs), accepted=len(acc), unranked=int((acc_rank < 0).sum()),
                accepted_after_first_chunk=int((acc_rank >= SEL_CHUNK).sum()), blocked_across=blocked)


def test_grid_state_crosses_a_chunk_boundary(ctx, orc):
    """A dense field: more than SEL_CHUNK candidates and more features asked for than exist, so every chunk is
    consumed -- corners accepted in the first chunk reject candidates of the later ones, and later chunks accept."""
    img, nf = noise_image(3), 5000
    p = chunk_crossing_properties(orc, img, nf)
    print(p)
    assert p["n_cand"] > SEL_CHUNK and p["accepted"] < nf and p["unranked"] == 0
    assert p["accepted_after_first_chunk"] > 0 and p["blocked_across"] > 0
    assert same_as_oracle(ctx, orc, img, nf)
