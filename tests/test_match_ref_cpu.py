"""CPU: the plain matcher reference (tests/match_ref.py) against the oracle, and the reach of the generators that
tests/test_match_batched_gpu.py feeds to the kernels -- checked here, from the reference alone, so that no GPU test has to
skip or can pass on inputs that exercise nothing."""
import numpy as np
import pytest

import match_ref as mr
from conftest import GOLDEN
from test_match_gpu import _planted


@pytest.fixture(scope="module")
def cases(synth):
    return mr.all_cases(synth)


def test_reference_is_the_oracle_on_planted_sets(orc, synth):
    for n1, n2 in ((1, 1), (1, 2), (63, 65), (64, 64), (300, 7), (7, 300), (513, 700)):
        d1, d2 = _planted(synth, 100 + n1 + n2, n1, n2)
        for thr, ratio in ((70, 1.2), (1, 1.2), (70, 1.0), (70, 0.5), (130, 1.2), (256, 1.2), (257, 1.0), (300, 2.0)):
            assert np.array_equal(mr.match(d1, d2, thr, ratio), orc.match_descriptors(d1, d2, thr, ratio)), (n1, n2, thr, ratio)


@pytest.mark.parametrize("k", [0, 9])
def test_reference_on_golden_euroc_pairs(orc, k):
    g = np.load(GOLDEN / ("euroc_pair%d.npz" % k))
    m = mr.match(g["desc0"], g["desc1"], 70, 1.2)
    assert np.array_equal(m, g["matches"])
    assert np.array_equal(m, orc.match_descriptors(g["desc0"], g["desc1"], 70, 1.2))


def test_reference_degenerate_sets(orc):
    z = np.zeros((0, 4), np.uint64)
    one = np.zeros((1, 4), np.uint64)
    for a, b in ((z, one), (one, z), (z, z)):
        for thr, ratio in ((70, 1.2), (257, 1.0)):
            assert mr.match(a, b, thr, ratio).shape == (0, 2)     # what every entry of the kernels returns for an empty set
    same = np.tile(np.array([[1, 2, 3, 4]], np.uint64), (130, 1))
    assert np.array_equal(mr.match(same, same), orc.match_descriptors(same, same))
    ones = np.full((70, 4), np.uint64(0xFFFFFFFFFFFFFFFF))
    zeros = np.zeros((70, 4), np.uint64)
    for thr in (256, 257):
        assert np.array_equal(mr.match(ones, zeros, thr, 1.0), orc.match_descriptors(ones, zeros, thr, 1.0))
    assert np.array_equal(mr.match(ones, zeros, 257, 1.0), [[0, 0]])


def test_reference_is_the_oracle_on_every_gpu_case(orc, cases):
    n = 0
    for c in cases:
        for pairs, thr, ratio in c.launches:
            for (a, b), m in zip(pairs, c.expected(pairs, thr, ratio)):
                if len(c.slots[a]) == 0 or len(c.slots[b]) == 0:
                    assert len(m) == 0        # (the oracle's loop is not defined on an empty set; the ABI returns no match)
                    continue
                assert np.array_equal(m, orc.match_descriptors(c.slots[a], c.slots[b], thr, ratio)), (c.name, a, b)
                n += 1
    assert n > 150


def test_every_gpu_case_reaches_every_rule(cases):
    """Per launch: at least one match, one row dropped by each rule, and (where ties are planted) one row whose best
    distance is shared by two or more columns -- except what mr.EXEMPT lists, which must then indeed not occur."""
    assert set(mr.EXEMPT) <= {c.name for c in cases}
    for c in cases:
        assert all(len(s) <= c.F for s in c.slots)
        exempt = mr.EXEMPT.get(c.name, set())
        for pairs, thr, ratio in c.launches:
            res = c.expected(pairs, thr, ratio, details=True)
            reasons = np.concatenate([info["reason"] for _, info in res])
            seen = {"match": sum(len(m) for m, _ in res) > 0,
                    "threshold": bool(np.any(reasons == mr.THRESHOLD)),
                    "ratio": bool(np.any(reasons == mr.RATIO)),
                    "cross-check": bool(np.any(reasons == mr.CROSS))}
            if c.ties:
                seen["ties"] = any(bool(np.any(info["tied"])) for _, info in res)
            for what, hit in seen.items():
                assert hit != (what in exempt), (c.name, len(pairs), thr, ratio, what)
            assert all(0 <= s < len(c.slots) for p in pairs for s in p) and len(pairs) <= c.max_pairs


def test_ragged_case_covers_the_stated_counts_and_lists(cases):
    c = next(x for x in cases if x.name == "ragged")
    assert tuple(len(s) for s in c.slots) == mr.RAGGED_COUNTS
    z = mr.RAGGED_COUNTS.index(0)
    assert [len(p) for p, _, _ in c.launches] == [8, 9, 13, 16, 17]
    for pairs, _, _ in c.launches:
        assert any(a == z and b != z for a, b in pairs) and any(a != z and b == z for a, b in pairs) and (z, z) in pairs
        assert any(a == b != z for a, b in pairs)
        lefts, rights = [a for a, _ in pairs], [b for _, b in pairs]
        assert any(lefts.count(s) >= 2 and s in rights for s in set(lefts))
        assert any(a > b for a, b in pairs) and any(abs(a - b) > 1 for a, b in pairs)
    lists = [p for p, _, _ in c.launches]
    assert not any(x is not y and x[:len(y)] == y for x in lists for y in lists)


def test_selection_case_selects_the_stated_numbers_of_columns(cases):
    c = next(x for x in cases if x.name == "selection")
    pairs, thr, ratio = c.launches[0]
    res = c.expected(pairs, thr, ratio, details=True)
    assert [info["n_selected"] for _, info in res[:6]] == list(mr.SELECTION_COUNTS)
    m6, i6 = res[6]
    assert i6["n_selected"] == 20 and np.sum(i6["reason"] != mr.THRESHOLD) >= 200    # many rows, one column
    assert res[7][1]["n_selected"] == 300 and res[9][1]["n_selected"] == 300 and len(res[7][0]) == 300
    assert res[8][1]["n_selected"] == 0 and len(res[8][0]) == 0


def test_tie_and_boundary_cases_hold_what_they_claim(cases):
    by = {c.name: c for c in cases}
    for ratio, name in ((1.2, "ties_1.2"), (1.0, "ties_1")):
        c = by[name]
        pairs, thr, _ = c.launches[0]
        res = c.expected(pairs, thr, ratio, details=True)
        m, info = res[0]                                         # (tie a, tie b)
        n = len(c.slots[1])
        D = mr.distances(c.slots[0], c.slots[1])
        for c0, c1 in ((31, 32), (63, 64), (255, 256), (n - 2, n - 1)):
            assert np.array_equal(c.slots[1][c0], c.slots[1][c1]) and np.array_equal(c.slots[0][c0], c.slots[0][c1])
            rows = np.nonzero(info["index"] == c0)[0]            # twin columns: the lower one is some row's best, shared
            assert any(info["tied"][r] and D[r, c1] == info["best"][r] for r in rows)
            if ratio == 1.0:
                assert any((m[:, 1] == c0) & np.isin(m[:, 0], rows)) and not np.any(m[:, 1] == c1)
        assert [0, 0] in m.tolist()
        m45 = res[4][0].tolist()                                 # (last a, last b): best match at index 0 and n - 1 of both
        assert [0, 0] in m45 and [len(c.slots[2]) - 1, len(c.slots[3]) - 1] in m45
        for s in (0, 1):
            pc = mr.POP8[c.slots[s].view(np.uint8)].reshape(-1, 32).sum(axis=1)
            assert 0 in pc and 256 in pc
    c = by["boundary_2048"]
    assert len(c.slots[0]) == 2048 and len(c.slots[1]) == 2047
    res = c.expected(*c.launches[0])
    assert [2046, 2047] in res[1].tolist() and [0, 2047] in res[2].tolist() and [2047, 2046] in res[0].tolist()
    c = by["boundary_2049"]
    assert len(c.slots[0]) == 2049 and max(len(s) for s in c.slots[1:]) <= 100
    res = c.expected(*c.launches[0])
    assert [99, 2048] in res[0].tolist() and [2048, 99] in res[1].tolist()
    for name, c in by.items():
        if name.startswith("threshold_"):
            assert all(len(p) == 9 and p[8] in ((0, 1), (1, 0)) for p, _, _ in c.launches)
            assert any(len(c.slots[b]) == 0 and len(c.slots[a]) > 0 for a, b in c.launches[0][0])
