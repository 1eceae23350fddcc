"""The host half of the pose graph's covariance calls (visual-slam_amd/csrc/pgo_cov_plan.h: pair validation, the class
of each pair, the fold relabelling, the unique column nodes and each pair's columns, the node-list plan of the marginal
call, the arena), compiled with g++ as plain C++ without HIP headers and driven by tests/cpp/pgo_cov_plan_test.cpp.  The literal values
are worked out by hand from the rules in the header; the program itself verifies the plan's properties on every plan it
prints and over a sweep of sizes.  A second build of the same program runs under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program: nothing is loaded into Python)."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "pgo_cov_plan_test.cpp"


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-pthread", *extra, "-I", str(ROOT / "visual-slam_amd" / "csrc"),
                    str(SRC), "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pgo_cov_plan") / "pgo_cov_plan_test")


def _run(exe, *args, stdin=""):
    r = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _fields(lines):
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines}


def _graph(fixed, pairs):
    return "%d\n%s\n%d\n%s\n" % (len(fixed), " ".join(map(str, fixed)), len(pairs), "\n".join("%d %d" % p for p in pairs))


# eight nodes, node 2 fixed: free indices 0 1 - 2 3 4 5 6
FIXED = [0, 0, 1, 0, 0, 0, 0, 0]
PAIRS = [(0, 1), (0, 7), (7, 3), (2, 4), (5, 1)]


def test_pair_rules(exe):
    assert _run(exe, "check", stdin=_graph(FIXED, PAIRS)) == ["0 -1"]
    assert _run(exe, "check", stdin=_graph(FIXED, [(0, 1), (8, 1)])) == ["1 1"]
    assert _run(exe, "check", stdin=_graph(FIXED, [(-1, 1)])) == ["1 0"]
    assert _run(exe, "check", stdin=_graph(FIXED, [(0, 1), (3, 4), (4, 4)])) == ["2 2"]
    assert _run(exe, "check", stdin=_graph([1, 0, 1], [(0, 1), (2, 0)])) == ["3 1"]
    assert _run(exe, "check", stdin=_graph(FIXED, [])) == ["0 -1"]


def test_band_plan_in_the_nodes_own_order(exe):
    # bw = 11: free distance 1 is read (6 + 5 = 11), everything further is solved for the node with the larger index
    p = _fields(_run(exe, "plan", 0, 0, 11, 0, 0, stdin=_graph(FIXED, PAIRS)))
    assert p["dims"] == [7, 42, 11, 1, 1, 1, 3]
    assert p["dev_free"] == [0, 1, -1, 2, 3, 4, 5, 6] and p["dev_node"] == list(range(8))
    assert p["kind"] == [1, 2, 2, 0, 2]
    assert p["col_nodes"] == [4, 6]
    assert p["col_unk"] == [24, 25, 26, 27, 28, 29, 36, 37, 38, 39, 40, 41, -1, -1, -1, -1]
    # (0, 7): node 7 (free 6) is solved, its columns are the second six; (7, 3) the same columns on the a side;
    # (5, 1): node 5 (free 4), the first six
    assert p["ca"] == [-1, -1, 6, -1, 0] and p["cb"] == [-1, 6, -1, -1, -1]
    assert p["row_lo"] == [0]


def test_the_diagnostic_solves_in_band_pairs_too(exe):
    p = _fields(_run(exe, "plan", 0, 0, 11, 1, 0, stdin=_graph(FIXED, PAIRS)))
    assert p["kind"] == [2, 2, 2, 0, 2] and p["col_nodes"] == [1, 4, 6]
    assert p["ca"] == [-1, -1, 12, -1, 6] and p["cb"] == [0, 12, -1, -1, -1]
    assert p["dims"][3:] == [2, 1, 0, 4] and p["row_lo"] == [0, 0]


def test_folded_numbering(exe):
    # seven free nodes: 0 1 2 3 go to 0 2 4 6, then back 4 5 6 -> 5 3 1; the fixed node behind them
    p = _fields(_run(exe, "plan", 1, 0, 11, 0, 0, stdin=_graph(FIXED, PAIRS)))
    assert p["dev_free"] == [0, 2, -1, 4, 6, 5, 3, 1] and p["dev_node"] == [0, 2, 7, 4, 6, 5, 3, 1]
    # (0, 7): ring neighbours, folded 0 | 1: read.  (0, 1): folded 0 | 2: distance 2 -> 17 > 11: solved
    assert p["kind"] == [2, 1, 2, 0, 2]
    assert p["fa"] == [0, 0, 1, -1, 5] and p["fb"] == [2, 1, 4, 6, 2]
    assert p["col_nodes"] == [2, 4, 5]
    assert p["ca"] == [-1, -1, -1, -1, 12] and p["cb"] == [0, -1, 6, -1, -1]
    # columns 12..17 of node 5 (partner: folded 2, row 12) lie in both blocks; block 0 also serves partner rows 0 and 6
    assert p["row_lo"] == [0, 12] and p["dims"][3] == 2


def test_dense_plan_gives_every_free_node_its_columns(exe):
    p = _fields(_run(exe, "plan", 0, 1, 0, 0, 1, stdin=_graph(FIXED, PAIRS)))
    assert p["kind"] == [2, 2, 2, 0, 2] and p["col_nodes"] == [0, 1, 2, 3, 4, 6]
    assert p["ca"] == [0, 0, 30, -1, 24] and p["cb"] == [6, 30, 12, 18, 6]
    assert p["dims"] == [7, 42, 0, 3, 1, 0, 4]


def _nodes(nodes):
    # a node list travels in the first column of the pair input
    return [(v, 0) for v in nodes]


def test_node_list_on_a_dense_four_node_graph(exe):
    # node 0 fixed: free indices - 0 1 2; the query is permuted and names nodes twice
    p = _fields(_run(exe, "nodes", 0, 1, 0, stdin=_graph([1, 0, 0, 0], _nodes([3, 1, 3, 2, 1]))))
    assert p["dims"] == [3, 18, 0, 2, 0]
    assert p["dev_free"] == [-1, 0, 1, 2]
    # unique and ascending, whatever the order of the query; every query points at its node's block
    assert p["q_free"] == [0, 1, 2] and p["q_slot"] == [2, 0, 2, 1, 0]
    # dense: the column nodes ARE the unique queried nodes, six columns each, sixteen per workgroup
    assert p["col_nodes"] == [0, 1, 2]
    assert p["col_unk"] == list(range(18)) + [-1] * 14
    # q_free 12 B | col_unk 128 B | row_lo 8 B || diag H 144 B | Linv one 32 x 32 panel | X 2 x 18 x 16 || blocks 3 x 288 B
    assert p["arena"] == [0, 0, 256, 512, 768, 768, 1024, 9216, 13824, 0, 1024, 14848]
    # a subset gets the same columns for its nodes' own slots: ascending, unique
    q = _fields(_run(exe, "nodes", 0, 1, 0, stdin=_graph([1, 0, 0, 0], _nodes([3, 3]))))
    assert q["q_free"] == [2] and q["q_slot"] == [0, 0] and q["col_unk"] == [12, 13, 14, 15, 16, 17] + [-1] * 10


def test_node_list_on_a_folded_ring_of_forty(exe):
    # node 0 fixed, 39 free: free index f goes to 2 f for f <= 19, else to 2 (38 - f) + 1
    fixed = [1] + [0] * 39
    p = _fields(_run(exe, "nodes", 1, 0, 17, stdin=_graph(fixed, _nodes([39, 1, 20, 21, 39]))))
    assert p["dims"] == [39, 234, 17, 0, 0]
    assert p["dev_free"][:4] == [-1, 0, 2, 4] and p["dev_free"][19:22] == [36, 38, 37] and p["dev_free"][39] == 1
    assert p["q_free"] == [0, 1, 37, 38] and p["q_slot"] == [1, 0, 3, 2, 1]
    # band routes: a diagonal block lies inside the band of the inverse, nothing is solved
    assert p["col_nodes"] == [] and p["col_unk"] == []
    # q_free 16 B || diag H 1872 B, no Linv, no X || blocks 4 x 288 B
    assert p["arena"] == [0, 0, 256, 256, 256, 256, 2304, 2304, 2304, 0, 1280, 3584]
    # the same ring where the folded band is too wide: dense columns in the folded numbering
    d = _fields(_run(exe, "nodes", 1, 1, 0, stdin=_graph(fixed, _nodes([39, 1]))))
    assert d["q_free"] == [0, 1] and d["q_slot"] == [1, 0] and d["col_unk"] == list(range(12)) + [-1] * 4


def test_empty_node_list(exe):
    p = _fields(_run(exe, "nodes", 0, 1, 0, stdin=_graph([1, 0, 0, 0], [])))
    assert p["q_free"] == [] and p["q_slot"] == [] and p["col_nodes"] == [] and p["col_unk"] == []
    assert p["dims"] == [3, 18, 0, 0, 0]
    # only the work buffers are left: diag H and the panel of Linv
    assert p["arena"] == [0, 0, 0, 0, 0, 0, 256, 8448, 8448, 0, 0, 8448]


def test_sweep(exe):
    (out,) = _run(exe, "sweep")
    w = out.split()
    # node lists: four per graph (empty, one node, random with duplicates, all free nodes in reverse) in the dense and
    # the band mode: 152 graphs per mode
    assert w[4] == "node_lists" and int(w[5]) == 152 * 2 * 4
    # 7 sizes x 3 fixed counts x both numberings x 3 modes x 4 widths x with / without candidates, less the two
    # combinations with as many fixed nodes as nodes (96 plans)
    assert w[0] == "checked" and int(w[1]) == 7 * 3 * 2 * 3 * 4 * 2 - 96 and w[2] == "solve" and int(w[3]) > 1000


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    san = _build(tmp_path / "pgo_cov_plan_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert _run(san, "sweep")
    assert _run(san, "plan", 1, 0, 11, 0, 1, stdin=_graph(FIXED, PAIRS))
    assert _run(san, "plan", 0, 1, 0, 0, 1, stdin=_graph(FIXED, PAIRS))
    assert _run(san, "nodes", 1, 0, 11, stdin=_graph(FIXED, _nodes([7, 0, 7, 3])))
    assert _run(san, "nodes", 0, 1, 0, stdin=_graph(FIXED, _nodes([7, 0, 7, 3])))
    assert _run(san, "nodes", 0, 1, 0, stdin=_graph(FIXED, []))
    assert _run(san, "check", stdin=_graph(FIXED, [(0, 1), (8, 1)]))
