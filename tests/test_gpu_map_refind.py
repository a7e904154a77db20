"""GPU: ptam_map_refind — MapMaker::ReFindInSingleKeyFrame / ReFindNewlyMade / ReFindFromFailureQueue (src/MapMaker.cc:1028-1081)
as one device call on the map tables — against the composed path it replaces (tests/map_refind_ref.py: the callers' loops and
set tests on the host -> ptam_refind_pairs -> the set updates and a numpy sort) on the product library bit for bit, and on the
CPU oracle by golden_util.assert_refind_equal's rule."""
import ctypes as C

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import map_refind_ref as R

pytestmark = pytest.mark.gpu
KEYFRAME, NEW_POINTS, QUEUE = _abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE


@pytest.fixture(scope="module")
def dev(hip):
    ctx = host.Context(lib=hip)
    scene = R.make_scene(ctx)
    yield ctx, scene
    scene["close"]()
    ctx.close()


@pytest.fixture(scope="module")
def ora(oracle):
    ctx = host.Context(lib=oracle)
    scene = R.make_scene(ctx)
    yield ctx, scene
    scene["close"]()
    ctx.close()


def tables(scene, points=None):
    return scene["kfs"], scene["poses"], scene["points"] if points is None else points, scene["meas"], scene["never"]


def one_call(ctx, scene, mode, points, work, finder=None, **kw):
    rf = finder or host.ReFinder(ctx)
    r = host.map_refind(ctx, rf, mode, *tables(scene, points), work, **kw)
    if finder is None:
        rf.close()
    return r


def composed(ctx, scene, mode, points, work, finder=None):
    rf = finder or host.ReFinder(ctx)
    r = R.compose(ctx, rf, mode, *tables(scene, points), work)
    if finder is None:
        rf.close()
    return r


def probe(ctx, scene, finder, point):
    """a two-pair ptam_refind_pairs call on `point` at the last keyframe's pose and one a hair off: template_kept tells whether the
    finder came with that point's template"""
    P = scene["points"][[point, point]]
    pose = np.array([scene["poses"][-1], scene["poses"][-1]])
    pose[1, 11] += 1e-4 * scene["z"]
    pairs = host.ReFinder.pairs([scene["kfs"][-1]] * 2, pose, P["pv"]["world"], P["pv"]["pixel_right_w"], P["pv"]["pixel_down_w"],
                                [scene["kfs"][1]] * 2, P["src_level"], np.stack([P["center_x"], P["center_y"]], 1), [point, point])
    return finder.find(pairs)[1]


@pytest.mark.parametrize("mode", [KEYFRAME, NEW_POINTS, QUEUE], ids=["keyframe", "new_points", "failure_queue"])
def test_one_call_equals_the_composed_path(dev, ora, mode):
    """KEYFRAME: one keyframe x 1244 points; NEW_POINTS: 60 points (3 bad) x 12 keyframes; FAILURE_QUEUE: 150 shuffled pairs with
    three duplicates.  Bit for bit against the product's own pair-level path, by the refind rule against the oracle."""
    (ctx, scene), (octx, oscene) = dev, ora
    points, work = R.make_work(mode, scene)
    r = one_call(ctx, scene, mode, points, work)
    R.assert_same_bits(r, composed(ctx, scene, mode, points, work))
    o = composed(octx, oscene, mode, points, work)
    R.assert_equal_by_refind_rule(r, o)
    assert o["n_found"] > 0 and o["n_never"] > 0 and o["n_skipped"] > 0
    if mode == NEW_POINTS:
        assert 0 < o["n_template_kept"] < o["n_pairs"] - o["n_skipped"] and o["n_bad_points"] == 3
    # without the merged tables the lists are the same
    r2 = one_call(ctx, scene, mode, points, work, merged=False)
    assert r2["found"].tobytes() == r["found"].tobytes() and r2["never"].tobytes() == r["never"].tobytes() and "meas_merged" not in r2


def test_pass_size_changes_nothing_and_the_state_survives(dev):
    """max_pairs_per_pass 1 (one point a pass), 13 (one point: 12 pairs) and 0 (the default: one pass here) give the same bits;
    afterwards each finder answers a two-pair ptam_refind_pairs call on the last visited point as the composed path's does"""
    ctx, scene = dev
    points, work = R.make_work(NEW_POINTS, scene)
    last = int(work[58])   # (work[59] is bBad)
    rf0 = host.ReFinder(ctx)
    want = composed(ctx, scene, NEW_POINTS, points, work, finder=rf0)
    kept0 = probe(ctx, scene, rf0, last)
    rf0.close()
    for per_pass in (1, 13, 0):
        rf = host.ReFinder(ctx)
        R.assert_same_bits(one_call(ctx, scene, NEW_POINTS, points, work, finder=rf, max_pairs_per_pass=per_pass), want)
        assert np.array_equal(probe(ctx, scene, rf, last), kept0), per_pass
        rf.close()
    assert want["n_template_kept"] > 0
    for mode in (KEYFRAME, QUEUE):   # the other modes split at any pair
        p2, w2 = R.make_work(mode, scene)
        R.assert_same_bits(one_call(ctx, scene, mode, p2, w2, max_pairs_per_pass=37), one_call(ctx, scene, mode, p2, w2))


def visible_point(ctx, scene):
    """a point keyframe 0 sees and nobody has in a table for keyframes 0 and 8 (the same pose twice)"""
    r = one_call(ctx, scene, KEYFRAME, None, [0])
    busy8 = set(scene["meas"]["point"][scene["meas"]["kf"] == 8].tolist()) | set(scene["never"]["point"][scene["never"]["kf"] == 8].tolist())
    return next(int(p) for p in r["found"]["point"] if int(p) not in busy8)


def queue(*kp):
    q = np.zeros(len(kp), R.PAIR_DT)
    q["kf"], q["point"] = [k for k, _ in kp], [p for _, p in kp]
    return q


def test_state_carries_from_call_to_call_and_a_raised_flag_stops(dev):
    ctx, scene = dev
    p = visible_point(ctx, scene)
    rf = host.ReFinder(ctx)
    a = one_call(ctx, scene, QUEUE, None, queue((0, p)), finder=rf)
    assert a["n_found"] == 1 and a["n_template_kept"] == 0
    # a raised flag: nothing is visited, the tables come back as copies, the finder is as it was
    points, work = R.make_work(NEW_POINTS, scene)
    s = one_call(ctx, scene, NEW_POINTS, points, work, finder=rf, stop=np.array([1], np.uint8))
    assert s["stopped"] == 1 and s["points_consumed"] == 0 and s["n_pairs"] == 0 and s["n_bad_points"] == 0
    assert len(s["found"]) == 0 and len(s["never"]) == 0 and s["n_template_kept"] == 0
    assert s["meas_merged"].tobytes() == scene["meas"].tobytes() and s["never_merged"].tobytes() == scene["never"].tobytes()
    R.assert_same_bits(s, R.compose(ctx, None, NEW_POINTS, *tables(scene, points), work, stop=True))
    # keyframe 8 has keyframe 0's pose: the first pair of the next call continues the previous call's last point
    b = one_call(ctx, scene, QUEUE, None, queue((8, p)), finder=rf)
    assert b["n_pairs"] == 1 and b["n_skipped"] == 0 and b["n_template_kept"] == 1
    rf.close()
    assert one_call(ctx, scene, QUEUE, None, queue((8, p)))["n_template_kept"] == 0   # a fresh finder re-makes it
    # a flag that stays down changes nothing
    R.assert_same_bits(one_call(ctx, scene, NEW_POINTS, points, work, stop=np.array([0], np.uint8)), one_call(ctx, scene, NEW_POINTS, points, work))


def test_merged_tables_feed_the_next_calls(dev):
    ctx, scene = dev
    points, work = R.make_work(NEW_POINTS, scene)
    r = one_call(ctx, scene, NEW_POINTS, points, work)
    depth = host.map_scene_depth(ctx, scene["poses"], points["pv"]["world"], r["meas_merged"])   # (refuses a table out of order)
    assert depth["n_meas"].sum() == len(r["meas_merged"])
    rf = host.ReFinder(ctx)
    again = host.map_refind(ctx, rf, NEW_POINTS, scene["kfs"], scene["poses"], points, r["meas_merged"], r["never_merged"], work)
    rf.close()
    assert again["n_pairs"] == r["n_pairs"] == again["n_skipped"] and again["n_found"] == 0 and again["n_never"] == 0
    assert again["meas_merged"].tobytes() == r["meas_merged"].tobytes() and again["never_merged"].tobytes() == r["never_merged"].tobytes()
    # no work at all: zero counts, copies
    none = one_call(ctx, scene, NEW_POINTS, points, np.zeros(0, np.int32))
    assert all(none[f] == 0 for f in R.COUNTS) and none["meas_merged"].tobytes() == scene["meas"].tobytes()
    assert none["never_merged"].tobytes() == scene["never"].tobytes()


def raw_call(ctx, finder, mode, handles, poses, points, meas, never, work, cap=None):
    """the C call with sentinel-filled outputs -> (status, every output buffer as bytes before, after)"""
    cnt = host.map_refind_pair_count(mode if mode in (KEYFRAME, NEW_POINTS, QUEUE) else NEW_POINTS, len(handles), len(points), len(work))
    cap = cnt if cap is None else cap
    bufs = [np.full(8, -7, np.int32), np.full(max(cnt, 1) * 8, -7, np.int32).view(R.MEAS_DT), np.full(max(cnt, 1), -7, np.int32),
            np.full(max(cnt, 1) * 2, -7, np.int32).view(R.PAIR_DT), np.full((len(meas) + cnt + 1) * 8, -7, np.int32).view(R.MEAS_DT),
            np.full((len(never) + cnt + 1) * 2, -7, np.int32).view(R.PAIR_DT)]
    before = [x.tobytes() for x in bufs]
    p = host._ptr
    rc = ctx.lib.map_refind(ctx.h, finder.h, None, mode, len(handles), p(handles), p(poses), len(points), p(points), len(meas), p(meas),
                            len(never), p(never), len(work), p(work), None, C.cast(p(bufs[0]), C.POINTER(_abi.MapRefindResult)), p(bufs[1]),
                            p(bufs[2]), p(bufs[3]), cap, p(bufs[4]), p(bufs[5]))
    return rc, before, [x.tobytes() for x in bufs]


def test_refusals_write_nothing_and_leave_the_finder_alone(dev, hip):
    ctx, scene = dev
    p = visible_point(ctx, scene)
    rf = host.ReFinder(ctx)
    assert one_call(ctx, scene, QUEUE, None, queue((0, p)), finder=rf)["n_found"] == 1
    K, N = len(scene["kfs"]), len(scene["points"])
    handles = np.array([k.h.value for k in scene["kfs"]], np.uint64)
    small = host.Context(lib=hip, size=(160, 128))
    kf_small = host.KeyFrame(small).MakeKeyFrame_Lite(np.zeros((128, 160), np.uint8))
    base = dict(mode=NEW_POINTS, handles=handles, poses=scene["poses"], points=scene["points"], meas=scene["meas"], never=scene["never"],
                work=np.array([5, 9, 700], np.int32))

    def changed(name, fn):
        x = base[name].copy()
        fn(x)
        return {name: x}

    def swap(x):
        x[[10, 11]] = x[[11, 10]]

    def repeat(x):
        x[11] = x[10]

    def field(f, i, v):
        def fn(x):
            x[f][i] = v
        return fn
    cases = {
        "meas out of order": changed("meas", swap), "meas repeated": changed("meas", repeat),
        "never out of order": changed("never", swap), "never repeated": changed("never", repeat),
        "meas keyframe out of range": changed("meas", field("kf", len(scene["meas"]) - 1, K)),
        "meas point out of range": changed("meas", field("point", len(scene["meas"]) - 1, N)),
        "never point negative": changed("never", field("point", 0, -1)),
        "meas level out of range": changed("meas", field("level", 3, 4)), "meas source out of range": changed("meas", field("source", 3, 5)),
        "point source keyframe out of range": changed("points", field("src_kf", 40, K)),
        "point source level out of range": changed("points", field("src_level", 40, 4)),
        "work point out of range": dict(work=np.array([5, N], np.int32)), "work point repeated": dict(work=np.array([5, 9, 5], np.int32)),
        "keyframe index out of range": dict(mode=KEYFRAME, work=np.array([K], np.int32)),
        "two keyframes in KEYFRAME": dict(mode=KEYFRAME, work=np.array([0, 1], np.int32)),
        "queue pair out of range": dict(mode=QUEUE, work=queue((0, 1), (K, 2))),
        "null keyframe": changed("handles", lambda x: x.__setitem__(3, 0)),
        "keyframe of another frame size": changed("handles", lambda x: x.__setitem__(3, kf_small.h.value)),
        "capacity too small": dict(cap=3 * K - 1), "unknown mode": dict(mode=3),
    }
    n_dev = C.c_int()
    hip.device_count(C.byref(n_dev))
    other = host.Context(lib=hip, device=1) if n_dev.value > 1 else None
    if other is not None:
        kf_other = host.KeyFrame(other).MakeKeyFrame_Lite(np.zeros((480, 640), np.uint8))
        cases["keyframe of another device"] = changed("handles", lambda x: x.__setitem__(3, kf_other.h.value))
    for name, change in cases.items():
        rc, before, after = raw_call(ctx, rf, **{**base, **change})
        assert rc == -1, name   # PTAM_E_ARG
        assert before == after, name
    # after every refusal the finder still holds the template of point p
    assert one_call(ctx, scene, QUEUE, None, queue((8, p)), finder=rf)["n_template_kept"] == 1
    rc, before, after = raw_call(ctx, rf, **base)   # (the call as it stands runs)
    assert rc == 0 and before != after
    for o in (rf, kf_small, small):
        o.close()
    if other is not None:
        kf_other.close()
        other.close()


def test_larger_map_in_several_passes(dev):
    """40 keyframe entries x 300 new points: 12 000 pairs, three passes at the default pass size"""
    ctx = dev[0]
    scene = R.make_scene(ctx, n_kf=40, seed=12)
    work = np.random.default_rng(5).permutation(len(scene["points"]))[:300].astype(np.int32)
    r = one_call(ctx, scene, NEW_POINTS, None, work)
    R.assert_same_bits(r, composed(ctx, scene, NEW_POINTS, None, work))
    assert r["n_pairs"] == 12000 and r["n_found"] > 0 and r["n_never"] > 0 and r["n_skipped"] > 0 and r["n_template_kept"] > 0
    scene["close"]()
