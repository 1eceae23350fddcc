"""The host half of landmark fusion (include/visnav_amd/fusion_plan.h), compiled with g++ as plain C++ and driven by
tests/cpp/fusion_plan_test.cpp on hand-written maps.  Every expected map below is written out by hand from the rules in
the header; the same program is also built once with -fsanitize=address,undefined and run on the largest scenario."""
import itertools
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "fusion_plan_test.cpp"


def _build(path, *flags):
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "include"), str(SRC), "-o", str(path)],
                   check=True)
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("fusion_plan") / "fusion_plan_test", "-O2")


def text(cams, lms, table, views, mp=()):
    """cams {(frame, cam): active}; lms {tid: dict(p, frm, obs, all, out)} (FeatureTracks {(frame, cam): feature});
    views [((frame, cam), [(feature, table index), ...])]; mp [((frame, cam), tid, feature)]"""
    out = ["cam %d %d %d" % (k[0], k[1], a) for k, a in cams.items()]
    for tid, lm in lms.items():
        out.append("lm %d %r %r %r %d %d" % ((tid,) + tuple(lm.get("p", (tid + 0.5, 2.0, 3.0))) + tuple(lm.get("frm", (0, 0)))))
        for name in ("obs", "all", "out"):
            out += ["%s %d %d %d %d" % (name, tid, k[0], k[1], f) for k, f in lm.get(name, {}).items()]
    out += ["mp %d %d %d %d" % (k[0], k[1], tid, f) for k, tid, f in mp]
    out.append("table %d %s" % (len(table), " ".join(map(str, table))))
    out += ["view %d %d %d %s" % (k[0], k[1], len(p), " ".join("%d %d" % q for q in p)) for k, p in views]
    return "\n".join(out) + "\n"


def run(exe, *args, **kw):
    r = subprocess.run([str(exe)], input=text(*args, **kw), capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return parse(r.stdout), r.stdout


def parse(stdout):
    res = {"lm": {}, "mp": {}}
    for ln in stdout.splitlines():
        w = ln.split()
        if w[0] == "counts":
            res["counts"] = dict(zip(("added", "merged", "conflicts", "refused"), map(int, w[1:])))
        elif w[0] == "lm":
            res["lm"][int(w[1])] = dict(p=tuple(map(float, w[2:5])), p_c0=float(w[5]), frm=(int(w[6]), int(w[7])))
        elif w[0] in ("obs", "all", "out"):
            v = list(map(int, w[2:]))
            res["lm"][int(w[1])][w[0]] = {(v[i], v[i + 1]): v[i + 2] for i in range(0, len(v), 3)}
        elif w[0] == "mp":
            v = list(map(int, w[3:]))
            res["mp"][(int(w[1]), int(w[2]))] = {v[i]: v[i + 1] for i in range(0, len(v), 2)}
    return res


OLD0, OLD1, NEW6, NEW7, NEW8 = (0, 0), (1, 0), (6, 0), (7, 0), (8, 0)
CAMS = {OLD0: 0, OLD1: 0, NEW6: 1, NEW7: 1, NEW8: 0}  # the old pass has left the active window; so has keyframe 8


def test_add_observation(exe):
    lms = {10: dict(all={OLD0: 5, OLD1: 6}, obs={}), 11: dict(all={OLD0: 9, NEW7: 4}, obs={NEW7: 4})}
    views = [(NEW7, [(3, 0), (4, 1)]), (NEW8, [(2, 0)])]  # 7: feature 3 is free -> track 10; feature 4 already observes 11
    got, _ = run(exe, CAMS, lms, [10, 11], views)
    assert got["counts"] == dict(added=2, merged=0, conflicts=0, refused=0)
    assert got["lm"][10]["all"] == {OLD0: 5, OLD1: 6, NEW7: 3, NEW8: 2}
    assert got["lm"][10]["obs"] == {NEW7: 3}  # camera 7 is active, camera 8 is not
    assert got["lm"][11]["all"] == {OLD0: 9, NEW7: 4} and got["lm"][11]["obs"] == {NEW7: 4}


def test_add_refused_when_the_track_has_another_feature_in_that_camera(exe):
    lms = {10: dict(all={OLD0: 5, NEW7: 8}, obs={NEW7: 8})}
    got, _ = run(exe, CAMS, lms, [10], [(NEW7, [(3, 0)])])
    assert got["counts"] == dict(added=0, merged=0, conflicts=1, refused=0)
    assert got["lm"][10]["all"] == {OLD0: 5, NEW7: 8} and got["lm"][10]["obs"] == {NEW7: 8}


def test_merge_smaller_id_survives_and_keeps_its_position(exe):
    lms = {20: dict(p=(1.0, 2.0, 3.0), frm=(0, 0), all={OLD0: 1, OLD1: 2}, obs={}),
           12: dict(p=(1.5, 2.5, 3.5), frm=(6, 0), all={NEW6: 7, NEW7: 3}, obs={NEW6: 7, NEW7: 3})}
    got, _ = run(exe, CAMS, lms, [20], [(NEW7, [(3, 0)])])  # feature 3 of camera 7 observes 12 and matches 20
    assert got["counts"] == dict(added=0, merged=1, conflicts=0, refused=0)
    assert list(got["lm"]) == [12]
    s = got["lm"][12]
    assert s["p"] == (1.5, 2.5, 3.5) and s["p_c0"] == -1.5 and s["frm"] == (6, 0)
    assert s["all"] == {OLD0: 1, OLD1: 2, NEW6: 7, NEW7: 3} and s["obs"] == {NEW6: 7, NEW7: 3}


def test_chained_merge(exe):
    lms = {5: dict(all={OLD0: 1}), 9: dict(all={NEW6: 2}, obs={NEW6: 2}), 14: dict(all={NEW7: 3}, obs={NEW7: 3})}
    # 6: feature 2 (track 9) matches 5;  7: feature 3 (track 14) matches 9  ->  requests {5, 9}, {9, 14}
    got, _ = run(exe, CAMS, lms, [5, 9, 14], [(NEW6, [(2, 0)]), (NEW7, [(3, 1)])])
    assert got["counts"] == dict(added=0, merged=2, conflicts=0, refused=0)
    assert list(got["lm"]) == [5]
    assert got["lm"][5]["all"] == {OLD0: 1, NEW6: 2, NEW7: 3} and got["lm"][5]["obs"] == {NEW6: 2, NEW7: 3}


def test_merge_refused_on_a_camera_with_two_features(exe):
    lms = {5: dict(all={OLD0: 1, NEW7: 8}, obs={NEW7: 8}), 9: dict(all={NEW6: 2, NEW7: 3}, obs={NEW6: 2, NEW7: 3})}
    got, _ = run(exe, CAMS, lms, [5, 9], [(NEW6, [(2, 0)])])  # track 9 matches 5, but camera 7 sees 5 at feature 8, 9 at 3
    assert got["counts"] == dict(added=0, merged=0, conflicts=0, refused=1)
    assert got["lm"][5]["all"] == {OLD0: 1, NEW7: 8} and got["lm"][9]["all"] == {NEW6: 2, NEW7: 3}
    assert got["lm"][5]["obs"] == {NEW7: 8} and got["lm"][9]["obs"] == {NEW6: 2, NEW7: 3}


def test_map_points_are_repointed(exe):
    lms = {20: dict(all={OLD0: 1, OLD1: 2}), 12: dict(all={NEW6: 7, NEW7: 3}, obs={NEW6: 7, NEW7: 3}), 30: dict(all={OLD0: 4})}
    mp = [(OLD0, 20, 1), (OLD0, 30, 4), (OLD1, 20, 2), (OLD1, 12, 2), (NEW7, 12, 3), (NEW8, 20, 6)]
    got, _ = run(exe, CAMS, lms, [20, 30], [(NEW7, [(3, 0)])], mp=mp)
    assert got["counts"]["merged"] == 1 and sorted(got["lm"]) == [12, 30]
    assert got["mp"] == {OLD0: {12: 1, 30: 4}, OLD1: {12: 2}, NEW6: {}, NEW7: {12: 3}, NEW8: {12: 6}}
    assert not any(20 in m for m in got["mp"].values())


def test_outlier_obs_clean_up(exe):
    # the loser carries camera 0 as an outlier, the survivor as an inlier (same feature): the union keeps it in obs only;
    # the loser's other outlier entry stays
    lms = {12: dict(all={OLD0: 1, NEW7: 3}, obs={OLD0: 1, NEW7: 3}, out={NEW6: 5}),
           20: dict(all={OLD0: 1, OLD1: 2}, obs={OLD1: 2}, out={OLD0: 1, NEW8: 9})}
    got, _ = run(exe, {**CAMS, OLD0: 1, OLD1: 1}, lms, [20], [(NEW7, [(3, 0)])])
    assert got["counts"]["merged"] == 1 and list(got["lm"]) == [12]
    s = got["lm"][12]
    assert s["obs"] == {OLD0: 1, OLD1: 2, NEW7: 3} and s["out"] == {NEW6: 5, NEW8: 9}
    assert s["all"] == {OLD0: 1, OLD1: 2, NEW7: 3}


def _mixed():
    lms = {5: dict(all={OLD0: 1}), 9: dict(all={NEW6: 2}, obs={NEW6: 2}), 14: dict(all={NEW7: 3}, obs={NEW7: 3}),
           21: dict(all={OLD1: 4}), 22: dict(all={OLD0: 6, NEW7: 8}, obs={NEW7: 8}), 23: dict(all={NEW6: 12, NEW7: 13}, obs={NEW6: 12}),
           40: dict(all={OLD1: 7}, out={OLD0: 2})}
    table = [5, 9, 14, 21, 22, 40]
    views = [(NEW6, [(2, 0), (30, 3), (31, 3), (12, 4)]),  # merge 9 -> 5; features 30 AND 31 both want track 21; 23 -> 22 refused
             (NEW7, [(3, 1), (40, 5), (41, 4)]),           # merge 14 -> 9 (-> 5); add to 40; 22 already has feature 8 in camera 7
             (NEW8, [(50, 5), (51, 0)])]                   # inactive camera: all_obs only
    mp = [(NEW6, 9, 2), (NEW7, 14, 3), (OLD0, 5, 1)]
    return lms, table, views, mp


def test_result_does_not_depend_on_pair_or_view_order(exe):
    lms, table, views, mp = _mixed()
    ref, ref_out = run(exe, CAMS, lms, table, views, mp=mp)
    assert ref["counts"] == dict(added=4, merged=2, conflicts=2, refused=1)
    assert sorted(ref["lm"]) == [5, 21, 22, 23, 40]
    assert ref["lm"][21]["all"] == {OLD1: 4, NEW6: 30}  # the smaller feature wins the contested camera
    assert ref["lm"][5]["all"] == {OLD0: 1, NEW6: 2, NEW7: 3, NEW8: 51} and ref["lm"][5]["obs"] == {NEW6: 2, NEW7: 3}
    assert ref["lm"][40]["all"] == {OLD1: 7, NEW7: 40, NEW8: 50} and ref["lm"][40]["obs"] == {NEW7: 40}
    assert ref["mp"][NEW6] == {5: 2} and ref["mp"][NEW7] == {5: 3}
    for view_order in itertools.permutations(range(3)):
        for rev in (False, True):
            v = [(views[i][0], views[i][1][::-1] if rev else views[i][1]) for i in view_order]
            lm_rev = dict(reversed(list(lms.items()))) if rev else lms
            assert run(exe, CAMS, lm_rev, table, v, mp=mp)[1] == ref_out, (view_order, rev)


def test_sanitized_build_runs_clean(tmp_path):
    san = _build(tmp_path / "fusion_plan_test_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    lms, table, views, mp = _mixed()
    got, _ = run(san, CAMS, lms, table, views, mp=mp)
    assert got["counts"] == dict(added=4, merged=2, conflicts=2, refused=1)
