"""CPU: the ONE place the oracle is pinned by the reference's own code.

`oracle/_ref/libdbow2_ref.so` is the reference's thirdparty/DBoW2_ORBSLAM/DBoW2/BowVector.cpp (addWeight :34-46,
addIfNotExist :50-58, normalize :62-84) and FeatureVector.cpp (addFeature :30-44), compiled unmodified where they
lie (`make -C oracle ref`).  The restatement in oracle/orc_bow.cpp must produce identical maps -- same keys, same
order, same f64 bit patterns -- on the same operation streams:
  * live, against the reference objects, wherever the library exists;
  * against tests/golden/dbow2_ref_streams.npz and dbow2_ref_live_digests.json, outputs of the reference objects
    (digests of them for the randomised streams) written by tools/make_ref_bow_golden.py, everywhere.
"""
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

from conftest import GOLDEN, ROOT


def _gen():
    spec = importlib.util.spec_from_file_location("make_ref_bow_golden", ROOT / "tools" / "make_ref_bow_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _same_f64(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_restatement_matches_reference_golden(orc):
    g = np.load(GOLDEN / "dbow2_ref_streams.npz")
    gen = _gen()
    for name, ids, vals, ops, norm in gen.streams():
        # the committed inputs are the generator's streams (the fixture is self-describing)
        assert np.array_equal(g[name + "_ids"], ids) and _same_f64(g[name + "_vals"], vals)
        oi, ov = orc.bowvec_stream(g[name + "_ids"], g[name + "_vals"], g[name + "_ops"], int(g[name + "_norm"]))
        assert np.array_equal(oi, g[name + "_out_ids"]), name
        assert _same_f64(ov, g[name + "_out_vals"]), name
    for name, nodes, feats in gen.fv_streams():
        on, of = orc.featvec_stream(g[name + "_nodes"], g[name + "_feats"])
        assert np.array_equal(on, g[name + "_out_nodes"]) and np.array_equal(of, g[name + "_out_feats"]), name


def test_restatement_matches_reference_objects_live(orc):
    gen = _gen()
    live = orc.ref_lib() is not None
    want = json.loads((GOLDEN / "dbow2_ref_live_digests.json").read_text())
    for trial, (ids, vals, ops, norm, nodes, feats) in enumerate(gen.live_trials()):
        oi, ov = orc.bowvec_stream(ids, vals, ops, norm)
        on, of = orc.featvec_stream(nodes, feats)
        if live:
            ri, rv = orc.ref_bowvec_stream(ids, vals, ops, norm)
            assert np.array_equal(oi, ri), trial
            assert _same_f64(ov, rv), trial
            rn, rf = orc.ref_featvec_stream(nodes, feats)
            assert np.array_equal(on, rn) and np.array_equal(of, rf), trial
        # everywhere: the reference objects' outputs on the same streams, as recorded by tools/make_ref_bow_golden.py
        assert gen.digest(oi, ov) == want["bowvec"][trial], trial
        assert gen.digest(on, of) == want["featvec"][trial], trial
    assert trial + 1 == len(want["bowvec"]) == len(want["featvec"])


def test_transform_tail_is_the_pinned_container_code(orc, synth, tmp_path):
    """orc_bow_transform's container half (everything after the tree descent) equals the reference classes driven
    with the per-descriptor (word, weight, node) triples: recover the triples by transforming one descriptor at a
    time (un-normalised weight = the leaf weight), replay them on the reference objects, compare with the batch.
    Where the reference library is absent, the replay's outputs recorded by tools/make_ref_bow_golden.py stand in."""
    gen = _gen()
    (ids, vals, fn, ff), (words, w, nodes, feats) = gen.transform_tail_case(orc, synth, tmp_path / "voc.txt")
    assert len(words) > 0
    if orc.ref_lib() is not None:
        ri, rv = orc.ref_bowvec_stream(words, w, np.zeros(len(words), np.uint8), 1)
        rn, rf = orc.ref_featvec_stream(nodes, feats)
        assert np.array_equal(ids, ri) and _same_f64(vals, rv)
        assert np.array_equal(fn, rn) and np.array_equal(ff, rf)
    want = json.loads((GOLDEN / "dbow2_ref_live_digests.json").read_text())["transform_tail"]
    assert gen.digest(ids, vals) == want["bowvec"]
    assert gen.digest(fn, ff) == want["featvec"]


def _pattern_from_inc(path):
    import re
    s = Path(path).read_text()
    s = s[s.index("*/") + 2:]
    return np.array([int(x) for x in re.findall(r"-?\d+", s)], np.int8).reshape(-1, 4)


# sha256 of the 256 x 4 int8 table {xa, ya, xb, yb} parsed from the reference's include/visnav/keypoints.h:55-131
REF_PATTERN_SHA256 = "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"


def test_rbrief_pattern_tables_equal_the_reference_table():
    """The 256 rBRIEF test pairs of the oracle and of the HIP kernels are the reference's numbers (keypoints.h:55-131):
    against the checksum recorded from the reference's text, and against the table parsed from that text
    (tests/golden/rbrief_pattern_ref.npy, written by tools/gen_pattern.py)."""
    import hashlib
    root = Path(__file__).resolve().parents[1]
    tabs = [_pattern_from_inc(root / "oracle" / "rbrief_pattern.inc"),
            _pattern_from_inc(root / "visual-slam_amd" / "csrc" / "rbrief_pattern.inc")]
    for t in tabs:
        assert t.shape == (256, 4)
        assert hashlib.sha256(t.tobytes()).hexdigest() == REF_PATTERN_SHA256
    ref = np.load(GOLDEN / "rbrief_pattern_ref.npy")
    assert ref.dtype == np.int8 and ref.shape == (256, 4)
    assert hashlib.sha256(ref.tobytes()).hexdigest() == REF_PATTERN_SHA256
    assert (tabs[0] == ref).all() and (tabs[1] == ref).all()
