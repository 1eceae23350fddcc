#!/usr/bin/env python3
"""Writes tests/golden/dbow2_ref_streams.npz: operation streams for DBoW2::BowVector / FeatureVector and the
outputs of the REFERENCE's own classes on them, and tests/golden/dbow2_ref_live_digests.json: sha256 digests of the
reference's outputs on the randomised streams of tests/test_oracle_ref_pin.py (live_trials, transform_tail_case) (oracle/_ref/libdbow2_ref.so = the reference's BowVector.cpp and
FeatureVector.cpp compiled unmodified by `make -C oracle ref`).  Run in the build container, where /root/reference
exists; the fixture is data (inputs + expected outputs), so the pin also holds where the reference is absent.
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as entry  # noqa: E402


def streams():
    """Deterministic operation streams: (name, ids, vals, ops, norm)."""
    out = []
    rng = np.random.default_rng(20261004)
    for case, (n, n_ids, norm) in enumerate([(0, 1, 1), (1, 1, 1), (1500, 400, 1), (1500, 1000000, 1), (4000, 37, 1),
                                              (1500, 400, 2), (1500, 400, 0), (257, 5, 1)]):
        ids = rng.integers(0, n_ids, n, dtype=np.uint32)
        # TF-IDF-like weights over many magnitudes, exact zeros and negative values included (fabs in normalize)
        vals = np.exp(rng.uniform(-12, 6, n)) * rng.choice([1.0, 1.0, 1.0, -1.0], n)
        vals[rng.random(n) < 0.02] = 0.0
        ops = (rng.random(n) < (0.5 if case % 2 else 0.0)).astype(np.uint8)
        out.append(("case%d" % case, ids, vals, ops, norm))
    return out


def fv_streams():
    rng = np.random.default_rng(7)
    out = []
    for case, (n, n_nodes) in enumerate([(0, 1), (1, 1), (1500, 90), (1500, 100000), (3000, 3)]):
        nodes = rng.integers(0, n_nodes, n, dtype=np.uint32)
        feats = rng.permutation(n).astype(np.uint32)
        out.append(("fv%d" % case, nodes, feats))
    return out


def live_trials():
    """The 60 randomised streams of the live comparison: (ids, vals, ops, norm, nodes, feats)."""
    rng = np.random.default_rng(99)
    for _ in range(60):
        n = int(rng.integers(0, 3000))
        n_ids = int(rng.choice([1, 7, 300, 5000, 2 ** 31]))
        ids = rng.integers(0, n_ids, n, dtype=np.uint32)
        vals = np.exp(rng.uniform(-20, 10, n)) * rng.choice([1.0, -1.0], n, p=[0.8, 0.2])
        vals[rng.random(n) < 0.05] = 0.0
        ops = (rng.random(n) < rng.choice([0.0, 0.3, 1.0])).astype(np.uint8)
        norm = int(rng.integers(0, 3))
        nodes = rng.integers(0, max(1, n_ids // 3), n, dtype=np.uint32)
        feats = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
        yield ids, vals, ops, norm, nodes, feats


def transform_tail_case(orc, synth, voc_path):
    """orc_bow_transform of 600 random descriptors on a k = 10, L = 3 vocabulary written to `voc_path`, and the
    per-descriptor (word, weight, node, feature) stream that replays its container half: the triples come from
    transforming one descriptor at a time (un-normalised weight = the leaf weight).
    Returns ((ids, vals, fnodes, ffeats) of the batch, (words, weights, nodes, feats) of the replay)."""
    voc_path = Path(voc_path)
    voc_path.write_text(synth.vocabulary_text(3, k=10, L=3))
    voc = orc.Vocabulary(voc_path)
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (600, 32), dtype=np.uint8)
    batch = voc.transform(f, levelsup=1)
    words, nodes, feats = [], [], []
    # leaf weights from the vocabulary text: line i+1 describes node i+1; word ids number the leaves in file order
    lines = voc_path.read_text().splitlines()[1:]
    leaf_w = [float(ln.split()[-1]) for ln in lines if ln.split()[1] == "1"]
    for i in range(len(f)):
        wi, wv, ni, _ = voc.transform(f[i:i + 1], levelsup=1)
        if len(wi):
            words.append(int(wi[0]))
            nodes.append(int(ni[0]))
            feats.append(i)
    w = np.array([leaf_w[k] for k in words])
    return tuple(batch), (np.array(words, np.uint32), w, np.array(nodes, np.uint32), np.array(feats, np.uint32))


def digest(*arrays):
    """sha256 of arrays by value: integers as int64, floats by their f64 bit patterns, shapes included."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        a = a.astype(np.float64).view(np.uint64) if a.dtype.kind == "f" else a.astype(np.int64)
        h.update(repr(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def write_live_digests(orc, tmp_dir):
    import importlib
    synth = importlib.import_module("visual_slam_amd.synth")
    doc = {"bowvec": [], "featvec": []}
    for ids, vals, ops, norm, nodes, feats in live_trials():
        doc["bowvec"].append(digest(*orc.ref_bowvec_stream(ids, vals, ops, norm)))
        doc["featvec"].append(digest(*orc.ref_featvec_stream(nodes, feats)))
    _, (words, w, nodes, feats) = transform_tail_case(orc, synth, Path(tmp_dir) / "voc.txt")
    doc["transform_tail"] = {"bowvec": digest(*orc.ref_bowvec_stream(words, w, np.zeros(len(words), np.uint8), 1)),
                             "featvec": digest(*orc.ref_featvec_stream(nodes, feats))}
    (ROOT / "tests" / "golden" / "dbow2_ref_live_digests.json").write_text(json.dumps(doc, indent=1) + "\n")


def main():
    import tempfile
    orc = entry.load_oracle()
    entry.load_package()
    assert orc.ref_lib() is not None, "oracle/_ref/libdbow2_ref.so missing and /root/reference absent"
    with tempfile.TemporaryDirectory() as d:
        write_live_digests(orc, d)
    doc = {}
    for name, ids, vals, ops, norm in streams():
        oi, ov = orc.ref_bowvec_stream(ids, vals, ops, norm)
        doc.update({name + "_ids": ids, name + "_vals": vals, name + "_ops": ops, name + "_norm": np.int32(norm),
                    name + "_out_ids": oi, name + "_out_vals": ov})
    for name, nodes, feats in fv_streams():
        on, of = orc.ref_featvec_stream(nodes, feats)
        doc.update({name + "_nodes": nodes, name + "_feats": feats, name + "_out_nodes": on, name + "_out_feats": of})
    np.savez_compressed(ROOT / "tests" / "golden" / "dbow2_ref_streams.npz", **doc)
    print("wrote", len(doc), "arrays")


if __name__ == "__main__":
    main()
