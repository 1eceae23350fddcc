"""GPU parity of vsl_frames_bow_vectors (batched ORB + vocabulary transform + device database append on the frame
store) with the single-image path it batches: vsl_compute_bow_vector (+ vsl_bowdb_append) and the oracle's ORB +
transform.  Every comparison is exact: integer arrays as they are, doubles through view(np.uint64).

Shapes are the smallest at which the batched kernels can go wrong: 96 x 80 and 161 x 123 images (odd sizes: no pyramid
level is a multiple of a tile), 60 and 300 features, ranges of 1, 3 and 5 slots."""
import ctypes as C

import numpy as np
import pytest

import orb_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (161, 123)]
NFS = [60, 300]
LEVELSUP = 4
u32p, i32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double)
ERR_INVALID, ERR_CAPACITY = -1, -4


def _images(w, h, base_seed=0):
    return np.stack([R.blocky_noise(w, h, 1000 * base_seed + 17 * w + h + i) for i in range(5)])


def _bits(vec):
    """(ids, vals, fv_node, fv_feat) with the doubles as their bit patterns."""
    ids, vals, fn, ff = vec
    return (np.asarray(ids, np.uint32), np.asarray(vals, np.float64).view(np.uint64), np.asarray(fn, np.uint32),
            np.asarray(ff, np.uint32))


def _assert_same(got, exp, what=""):
    for name, g, e in zip(("ids", "vals", "fv_node", "fv_feat"), _bits(got), _bits(exp)):
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        assert np.array_equal(g, e), (what, name)


@pytest.fixture(scope="module")
def voc_pair(ctx, orc, vsl, synth, tmp_path_factory):
    path = tmp_path_factory.mktemp("frames_bow") / "voc.txt"
    path.write_text(synth.vocabulary_text(5, 10, 3))
    voc, ovoc = vsl.Vocabulary(ctx, str(path)), orc.Vocabulary(str(path))
    yield voc, ovoc
    voc.close()


@pytest.fixture(scope="module")
def ref(ctx, orc, voc_pair):
    """Single-image results, computed once: ref[(w, h, nf)] = (images[5], [compute_bow_vector per image], [feature counts])."""
    voc, ovoc = voc_pair
    out = {}
    for w, h in SIZES:
        imgs = _images(w, h)
        for nf in NFS:
            single = [voc.compute_bow_vector(img, nf, LEVELSUP) for img in imgs]
            counts = []
            for img, s in zip(imgs, single):
                _, odesc = orc.orb_detect_describe(img, nf)
                _assert_same(s, ovoc.transform(odesc, LEVELSUP), "single-image path vs oracle")
                counts.append(len(odesc))
            assert min(counts) > 0
            out[(w, h, nf)] = (imgs, single, counts)
    return out


def _store(vsl, ctx, imgs):
    f = vsl.Frames(ctx, len(imgs), imgs.shape[2], imgs.shape[1], max_features=64, max_pairs=1)
    f.upload(0, imgs)
    return f


def _abi(ctx, frames, first, n, voc, nf, db=None, cap=0, levelsup=LEVELSUP):
    """The raw call: (rc, ids, vals, nnz, fv_node, fv_feat, fv_n, n_features, db_index), buffers pre-filled with marks."""
    m = max(n * cap, 1)
    ids, vals = np.full(m, 0xABABABAB, np.uint32), np.full(m, -7.0, np.float64)
    fn, ff = np.full(m, 0xABABABAB, np.uint32), np.full(m, 0xABABABAB, np.uint32)
    nnz, fvn = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    nfeat, index = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    rc = ctx.L.vsl_frames_bow_vectors(ctx.h, frames.h, first, n, voc.h if voc is not None else None, nf, levelsup,
                                      db.h if db is not None else None, index.ctypes.data_as(i32p), cap,
                                      ids.ctypes.data_as(u32p), vals.ctypes.data_as(f64p), nnz.ctypes.data_as(i32p),
                                      fn.ctypes.data_as(u32p), ff.ctypes.data_as(u32p), fvn.ctypes.data_as(i32p),
                                      nfeat.ctypes.data_as(i32p))
    return rc, ids, vals, nnz, fn, ff, fvn, nfeat, index


def _raw_bytes(res):
    return b"".join(a.tobytes() for a in res[1:])


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("w,h", SIZES)
def test_batched_equals_single_image_path_and_oracle(ctx, vsl, voc_pair, ref, w, h, nf, n):
    voc, _ = voc_pair
    imgs, single, counts = ref[(w, h, nf)]
    f = _store(vsl, ctx, imgs)
    try:
        first = 5 - n
        got = f.bow_vectors(first, n, voc, nf, LEVELSUP)
        assert len(got) == n
        for i in range(n):
            _assert_same(got[i], single[first + i], "image %d" % (first + i))   # = the oracle's ORB + transform (ref fixture)
        rc, *_, nfeat, _ = _abi(ctx, f, first, n, voc, nf)    # cap_per_image = 0: only the feature counts
        assert rc == 0 and nfeat[:n].tolist() == counts[first:]
    finally:
        f.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,nf", [(96, 80, 300), (161, 123, 60)])
def test_image_result_is_independent_of_its_neighbours(ctx, vsl, voc_pair, ref, w, h, nf):
    voc, _ = voc_pair
    imgs, single, _ = ref[(w, h, nf)]
    f = _store(vsl, ctx, imgs)
    try:
        alone = f.bow_vectors(2, 1, voc, nf, LEVELSUP)[0]
        among = f.bow_vectors(0, 5, voc, nf, LEVELSUP)[2]
        others = _images(w, h, base_seed=3)
        others[2] = imgs[2]
        assert not np.array_equal(others[1], imgs[1])
        f.upload(0, others)
        replaced = f.bow_vectors(0, 5, voc, nf, LEVELSUP)[2]
        for got in (alone, among, replaced):
            _assert_same(got, single[2])
    finally:
        f.close()


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,nf", [(96, 80, 60), (161, 123, 300)])
def test_result_is_independent_of_the_pass_size(ctx, vsl, voc_pair, ref, w, h, nf):
    voc, _ = voc_pair
    imgs, single, counts = ref[(w, h, nf)]
    f = _store(vsl, ctx, imgs)
    cap = max(counts)
    try:
        results = []
        for chunk in (1, 2, 5, 0):   # 0 = unset: as many images as the scratch budget holds
            ctx.set_diagnostic("frames_bow_chunk", chunk)
            res = _abi(ctx, f, 0, 5, voc, nf, cap=cap)
            assert res[0] == 0
            results.append(_raw_bytes(res))
        assert results[0] == results[1] == results[2] == results[3]
        for i in range(5):   # ... and they are the right bytes
            _assert_same(f.bow_vectors(0, 5, voc, nf, LEVELSUP)[i], single[i])
    finally:
        ctx.set_diagnostic("frames_bow_chunk", 0)
        f.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1])
def test_mixed_batch_flat_tie_overflow_and_ordinary(ctx, orc, vsl, voc_pair, chunk):
    voc, ovoc = voc_pair
    w, h, nf = 161, 123, 60
    flat = np.full((h, w), 90, np.uint8)
    dots = R.dot_grid(w, h, 8)
    okp, odesc = orc.orb_detect_describe(dots, nf)
    assert int((okp[:, 4] == 0).sum()) > 2 * orc.orb_level_quota(nf)[0] + 64   # level 0 overflows its first segment
    ordinary = R.blocky_noise(w, h, 4242)
    imgs = np.stack([flat, dots, ordinary, dots, flat])
    f = _store(vsl, ctx, imgs)
    try:
        ctx.set_diagnostic("frames_bow_chunk", chunk)
        got = f.bow_vectors(0, 5, voc, nf, LEVELSUP)
        rc, *_, nfeat, _ = _abi(ctx, f, 0, 5, voc, nf)
        assert rc == 0
        for i, img in enumerate(imgs):
            _assert_same(got[i], voc.compute_bow_vector(img, nf, LEVELSUP), "image %d" % i)
            _, od = orc.orb_detect_describe(img, nf)
            _assert_same(got[i], ovoc.transform(od, LEVELSUP), "image %d vs oracle" % i)
            assert nfeat[i] == len(od)
        assert nfeat[0] == 0 and all(len(a) == 0 for a in got[0])
        assert nfeat[1] == len(odesc) > 0 and nfeat[2] > 0
    finally:
        ctx.set_diagnostic("frames_bow_chunk", 0)
        f.close()


@pytest.mark.parametrize("keys64", [0, 1])
def test_one_pass_with_images_on_both_sides_of_the_2048_feature_kernel(ctx, orc, vsl, voc_pair, keys64):
    """The assembly kernel has a form for <= 2048 features and one for more, each with 32- or 64-bit sort keys; the
    single-image call picks per image, a pass picks for its largest image.  320 x 240 is the smallest dot grid
    (step 4) with more than 2048 tied keypoints; the images beside it have a few hundred features."""
    voc, ovoc = voc_pair
    w, h, nf = 320, 240, 100
    dots = R.dot_grid(w, h, 4)
    imgs = np.stack([R.blocky_noise(w, h, 77), dots, R.blocky_noise(w, h, 78)])
    exp = []
    for img in imgs:
        _, od = orc.orb_detect_describe(img, nf)
        exp.append((len(od), ovoc.transform(od, LEVELSUP)))
    assert 2048 < exp[1][0] <= 8192 and 0 < exp[0][0] < 2048 and 0 < exp[2][0] < 2048
    single = [voc.compute_bow_vector(img, nf, LEVELSUP) for img in imgs]   # default keys, the form of each image's own size
    f = _store(vsl, ctx, imgs)
    try:
        ctx.set_diagnostic("bow_keys64", keys64)
        got = f.bow_vectors(0, 3, voc, nf, LEVELSUP)                      # one pass: the 8192 form for all three
        alone = f.bow_vectors(0, 1, voc, nf, LEVELSUP)[0]                 # ... and the 2048 form for the first alone
        for i in range(3):
            _assert_same(got[i], exp[i][1], "image %d vs oracle" % i)
            _assert_same(got[i], single[i], "image %d vs single-image call" % i)
        _assert_same(alone, single[0])
    finally:
        ctx.set_diagnostic("bow_keys64", 0)
        f.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def _db_answers(db, queries, n_words):
    out = [db.info()]
    for ids, vals in queries:
        out.append(db.score(ids, vals).view(np.uint64).tolist())
        idx, cnt, sc, ns, mx = db.query(ids, vals, n_words)
        out.append((idx.tolist(), cnt.tolist(), sc.view(np.uint64).tolist(), ns, mx))
    return out


@pytest.mark.parametrize("w,h,nf", [(96, 80, 300), (161, 123, 60)])
def test_device_append_equals_sequential_appends(ctx, vsl, voc_pair, ref, w, h, nf):
    voc, _ = voc_pair
    imgs, single, _ = ref[(w, h, nf)]
    n_words = voc.info()[3]
    seq, bat = vsl.BowDatabase(ctx, 1 << 16, 64), vsl.BowDatabase(ctx, 1 << 16, 64)
    f = _store(vsl, ctx, imgs)
    try:
        for k, s in enumerate(single):
            assert seq.append(s[0], s[1]) == k
        vecs, index = f.bow_vectors(0, 5, voc, nf, LEVELSUP, db=bat)
        assert index.tolist() == [0, 1, 2, 3, 4]
        queries = [(s[0], s[1]) for s in single]
        assert _db_answers(bat, queries, n_words) == _db_answers(seq, queries, n_words)
        # a second batch (device only, with an empty vector in it) continues the numbering
        more = imgs[[3, 1, 0]].copy()
        more[1] = 90
        f.upload(0, more)
        for img in more:
            v = voc.compute_bow_vector(img, nf, LEVELSUP)
            seq.append(v[0], v[1])
        none, index = f.bow_vectors(0, 3, voc, nf, LEVELSUP, db=bat, host_outputs=False)
        assert none is None and index.tolist() == [5, 6, 7]
        assert bat.info()[0] == 8
        assert _db_answers(bat, queries, n_words) == _db_answers(seq, queries, n_words)
    finally:
        f.close()
        seq.close()
        bat.close()


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_capacity_contract(ctx, vsl, voc_pair, ref):
    voc, _ = voc_pair
    w, h, nf = 161, 123, 300
    imgs, single, counts = ref[(w, h, nf)]
    n_words = voc.info()[3]
    queries = [(s[0], s[1]) for s in single[:2]]
    f = _store(vsl, ctx, imgs)
    db = vsl.BowDatabase(ctx, 1 << 16, 64)
    try:
        db.append(single[0][0], single[0][1])
        before = _db_answers(db, queries, n_words)
        for chunk in (0, 2):   # the counts are filled whichever pass meets the error
            ctx.set_diagnostic("frames_bow_chunk", chunk)
            rc, *_, nfeat, _ = _abi(ctx, f, 0, 5, voc, nf, db=db, cap=max(counts) - 1)
            assert rc == ERR_CAPACITY and nfeat.tolist() == counts
            assert str(max(counts)) in ctx.L.vsl_last_error(ctx.h).decode()
            assert _db_answers(db, queries, n_words) == before
        ctx.set_diagnostic("frames_bow_chunk", 0)
        # room for 4 of 5 vectors
        tiny_ids, tiny_vals = np.array([1, 5], np.uint32), np.array([0.25, 0.75])
        while db.info()[0] < 60:
            db.append(tiny_ids, tiny_vals)
        before = _db_answers(db, queries, n_words)
        rc, *_, nfeat, _ = _abi(ctx, f, 0, 5, voc, nf, db=db)
        assert rc == ERR_CAPACITY and nfeat.tolist() == counts
        assert _db_answers(db, queries, n_words) == before
        rc, *_, index = _abi(ctx, f, 0, 4, voc, nf, db=db)   # four do fit
        assert rc == 0 and index[:4].tolist() == [60, 61, 62, 63] and db.info()[0] == 64
        db.reserve(1 << 16, 128)                              # ... and after a reserve the fifth
        rc, *_, index = _abi(ctx, f, 4, 1, voc, nf, db=db)
        assert rc == 0 and index[0] == 64
        sc = db.score(single[4][0], single[4][1], cand_index=[64])
        seq = vsl.BowDatabase(ctx, 1 << 16, 64)
        try:
            seq.append(single[4][0], single[4][1])
            assert sc.view(np.uint64).tolist() == seq.score(single[4][0], single[4][1]).view(np.uint64).tolist()
        finally:
            seq.close()
        # bad ranges, a NULL vocabulary
        for first, n in ((-1, 1), (0, 6), (5, 1), (3, 3), (0, -1)):
            assert _abi(ctx, f, first, n, voc, nf)[0] == ERR_INVALID, (first, n)
            assert b"range" in ctx.L.vsl_last_error(ctx.h)
        assert _abi(ctx, f, 0, 5, None, nf)[0] == ERR_INVALID and b"voc" in ctx.L.vsl_last_error(ctx.h)
    finally:
        ctx.set_diagnostic("frames_bow_chunk", 0)
        f.close()
        db.close()
    small = vsl.Frames(ctx, 2, 48, 48, max_features=64, max_pairs=1)
    try:
        small.upload(0, np.zeros((2, 48, 48), np.uint8))
        assert _abi(ctx, small, 0, 2, voc, nf)[0] == ERR_INVALID and b"64" in ctx.L.vsl_last_error(ctx.h)
    finally:
        small.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_determinism_same_context_and_fresh_context(ctx, vsl, synth, ref, tmp_path):
    w, h, nf = 161, 123, 300
    imgs, single, counts = ref[(w, h, nf)]
    path = tmp_path / "voc.txt"
    path.write_text(synth.vocabulary_text(5, 10, 3))
    runs = []
    for c in (ctx, ctx, vsl.Context(0)):
        voc = vsl.Vocabulary(c, str(path))
        f = _store(vsl, c, imgs)
        try:
            res = _abi(c, f, 0, 5, voc, nf, cap=max(counts))
            assert res[0] == 0
            runs.append(_raw_bytes(res))
        finally:
            f.close()
            voc.close()
            if c is not ctx:
                c.close()
    assert runs[0] == runs[1] == runs[2]


# 8 ---------------------------------------------------------------------------------------------------------------------
def test_single_image_call_between_two_batched_calls_shares_the_scratch(ctx, orc, vsl, voc_pair, ref):
    """Both entry points carve the context's one scratch and one pinned buffer, each in its own way: a single-image
    call of another size between two batched calls leaves nothing behind that the second one sees."""
    voc, _ = voc_pair
    w, h, nf = 161, 123, 300
    imgs, single, counts = ref[(w, h, nf)]
    small = R.blocky_noise(96, 80, 9680)
    f = _store(vsl, ctx, imgs)
    try:
        first = _abi(ctx, f, 0, 5, voc, nf, cap=max(counts))
        kp, desc = ctx.orb_detect_describe(small, nf)
        second = _abi(ctx, f, 0, 5, voc, nf, cap=max(counts))
        assert first[0] == 0 and second[0] == 0 and _raw_bytes(first) == _raw_bytes(second)
        okp, odesc = orc.orb_detect_describe(small, nf)
        assert len(okp) > 0 and np.array_equal(kp.view(np.uint32), okp.view(np.uint32)) and np.array_equal(desc, odesc)
        for i, v in enumerate(f.bow_vectors(0, 5, voc, nf, LEVELSUP)):   # ... and they are the right bytes
            _assert_same(v, single[i])
    finally:
        f.close()
