"""CPU: tests/map_refind_ref.py, the index-order restatement of MapMaker::ReFindInSingleKeyFrame / ReFindNewlyMade /
ReFindFromFailureQueue (src/MapMaker.cc:1028-1081) that the device call ptam_map_refind is checked against, run on the CPU
oracle on the scene of the GPU tests: the checker checked."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import map_refind_ref as R

MODES = [_abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE]


@pytest.fixture(scope="module")
def runs(oracle):
    """compose on the oracle, once per mode, each with a fresh finder"""
    ctx = host.Context(lib=oracle)
    scene = R.make_scene(ctx)
    out = {}
    for mode in MODES:
        points, work = R.make_work(mode, scene)
        rf = host.ReFinder(ctx)
        out[mode] = (points, work, R.compose(ctx, rf, mode, scene["kfs"], scene["poses"], points, scene["meas"], scene["never"], work))
        rf.close()
    yield scene, out
    scene["close"]()
    ctx.close()


def keys(t):
    return set(zip(t["kf"].tolist(), t["point"].tolist()))


def test_scene_tables_are_sorted_and_disjoint(runs):
    scene, _ = runs
    n = len(scene["points"])
    for t in (scene["meas"], scene["never"]):
        assert np.all(np.diff(t["kf"].astype(np.int64) * n + t["point"]) > 0)
    total = len(scene["kfs"]) * n
    assert 0.27 * total < len(scene["meas"]) < 0.33 * total and 0.05 * total < len(scene["never"]) < 0.09 * total
    assert not keys(scene["meas"]) & keys(scene["never"])


@pytest.mark.parametrize("mode", MODES)
def test_skipped_found_never_partition_the_pairs(runs, mode):
    scene, out = runs
    points, work, r = out[mode]
    kf, pt, skip, n_bad = R.pairs_for(mode, len(scene["kfs"]), points, scene["meas"], scene["never"], work)
    assert r["n_pairs"] == len(kf) == r["n_skipped"] + r["n_found"] + r["n_never"] and r["n_skipped"] == skip.sum()
    assert r["n_found"] > 0 and r["n_never"] > 0 and r["n_skipped"] > 0 and r["n_bad_points"] == n_bad
    visited, f, nv = list(zip(kf.tolist(), pt.tolist())), keys(r["found"]), keys(r["never"])
    assert len(f) == len(r["found"]) and len(nv) == len(r["never"]) and not f & nv
    assert f | nv == {kp for kp, s in zip(visited, skip) if not s}
    # no found or never pair was in the input tables
    assert not (f | nv) & (keys(scene["meas"]) | keys(scene["never"]))
    assert np.all(r["found"]["source"] == _abi.SRC_REFIND) and np.array_equal(r["found_subpix"], (r["found"]["level"] > 0).astype(np.int32))
    # visiting order
    order = {kp: i for i, kp in reversed(list(enumerate(visited)))}
    for t in (r["found"], r["never"]):
        assert np.all(np.diff([order[kp] for kp in zip(t["kf"].tolist(), t["point"].tolist())]) > 0)


@pytest.mark.parametrize("mode", MODES)
def test_merged_tables_are_sorted_unions(runs, mode):
    scene, out = runs
    _, _, r = out[mode]
    n = len(scene["points"])
    for merged, table, new in ((r["meas_merged"], scene["meas"], r["found"]), (r["never_merged"], scene["never"], r["never"])):
        assert len(merged) == len(table) + len(new)
        assert np.all(np.diff(merged["kf"].astype(np.int64) * n + merged["point"]) > 0)     # sorted, no pair twice
        assert keys(merged) == keys(table) | keys(new)
    # the rows come along whole
    m = r["meas_merged"]
    rows = {(int(x["kf"]), int(x["point"])): x.tobytes() for x in m}
    assert all(rows[(int(x["kf"]), int(x["point"]))] == x.tobytes() for x in scene["meas"][::97])
    assert all(rows[(int(x["kf"]), int(x["point"]))] == x.tobytes() for x in r["found"])


def test_new_points_keep_templates_and_bad_points_make_no_pair(runs):
    scene, out = runs
    points, work, r = out[_abi.MAP_REFIND_NEW_POINTS]
    assert r["n_bad_points"] == 3 and r["n_pairs"] == 57 * len(scene["kfs"]) and r["points_consumed"] == 60
    bad = set(work[[7, 30, 59]].tolist())
    assert not bad & set(r["found"]["point"].tolist()) and not bad & set(r["never"]["point"].tolist())
    assert 0 < r["n_template_kept"] < r["n_pairs"] - r["n_skipped"]
    # KEYFRAME does not look at bBad: the same table with the flags up visits every point
    kf, pt, skip, n_bad = R.pairs_for(_abi.MAP_REFIND_KEYFRAME, len(scene["kfs"]), points, scene["meas"], scene["never"], [0])
    assert len(pt) == len(points) and n_bad == 0


def test_later_of_two_equal_queue_pairs_is_skipped(runs):
    scene, out = runs
    points, work, r = out[_abi.MAP_REFIND_FAILURE_QUEUE]
    kf, pt, skip, _ = R.pairs_for(_abi.MAP_REFIND_FAILURE_QUEUE, len(scene["kfs"]), points, scene["meas"], scene["never"], work)
    assert len(kf) == 150 and np.all(np.diff(kf.astype(np.int64) * len(points) + pt) >= 0)      # the sort of :1074
    dup = np.flatnonzero((np.diff(kf) == 0) & (np.diff(pt) == 0)) + 1
    assert len(dup) == 3 and skip[dup].all()
    in_tables = keys(scene["meas"]) | keys(scene["never"])
    first = dup - 1
    assert [bool(s) for s in skip[first]] == [(int(kf[i]), int(pt[i])) in in_tables for i in first]
    assert r["n_pairs"] == 150 and r["points_consumed"] == 0


def test_known_answers_on_a_tiny_map():
    pts = np.zeros(4, R.POINT_DT)
    pts["bad"][2] = 1
    meas = np.zeros(2, R.MEAS_DT)
    meas["kf"], meas["point"] = [0, 1], [1, 3]
    never = np.zeros(1, R.PAIR_DT)
    never["kf"], never["point"] = [1], [0]
    kf, pt, skip, n_bad = R.pairs_for(_abi.MAP_REFIND_NEW_POINTS, 2, pts, meas, never, [3, 2, 0])
    assert list(zip(kf, pt)) == [(0, 3), (1, 3), (0, 0), (1, 0)] and list(skip) == [0, 1, 0, 1] and n_bad == 1
    kf, pt, skip, n_bad = R.pairs_for(_abi.MAP_REFIND_KEYFRAME, 2, pts, meas, never, [1])
    assert list(zip(kf, pt)) == [(1, 0), (1, 1), (1, 2), (1, 3)] and list(skip) == [1, 0, 0, 1] and n_bad == 0
    q = np.zeros(4, R.PAIR_DT)
    q["kf"], q["point"] = [1, 0, 1, 0], [2, 1, 2, 0]
    kf, pt, skip, n_bad = R.pairs_for(_abi.MAP_REFIND_FAILURE_QUEUE, 2, pts, meas, never, q)
    assert list(zip(kf, pt)) == [(0, 0), (0, 1), (1, 2), (1, 2)] and list(skip) == [0, 1, 0, 1]


def test_stop_before_the_call_visits_nothing(oracle):
    ctx = host.Context(lib=oracle)
    scene = R.make_scene(ctx)
    points, work = R.make_work(_abi.MAP_REFIND_NEW_POINTS, scene)
    rf = host.ReFinder(ctx)
    r = R.compose(ctx, rf, _abi.MAP_REFIND_NEW_POINTS, scene["kfs"], scene["poses"], points, scene["meas"], scene["never"], work, stop=True)
    assert r["stopped"] == 1 and r["n_pairs"] == 0 and r["points_consumed"] == 0 and len(r["found"]) == 0 and len(r["never"]) == 0
    assert np.array_equal(r["meas_merged"], scene["meas"]) and np.array_equal(r["never_merged"], scene["never"])
    rf.close()
    scene["close"]()
    ctx.close()
