"""-m gpu: a session from the first frame — ptam_camera_tracker_enable_session / _session_frames (host.CameraTracker.EnableSession,
SessionFrame) — against tests/camera_session_ref.py: the trails of a twin ptam_trails frame by frame, then the map of the one call
ResidentMap.InitFromStereo(matches) and the frames of camera_tracker_ref.RefCameraTracker reset at the tracker's pose.  Results,
states, pools and every table of both maps are compared by == / tobytes()."""
import threading

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import camera_session_ref as R
from tests.camera_tracker_ref import CAP, MAX_KF, TRACKED
from tests.test_gpu_camera_tracker import same_frame
from tests.test_gpu_resident_map import check_invariants, same_tables

pytestmark = pytest.mark.gpu
S = _abi
E_STATE = -3
NOT_STARTED, STARTED, COMPLETE = S.TRAIL_TRACKING_NOT_STARTED, S.TRAIL_TRACKING_STARTED, S.TRAIL_TRACKING_COMPLETE
OPTS = dict(keyframe_gap=1, max_queue=3, shuffle_seed=0x9E3779B97F4A7C15, tag_base=1000, reports=8, keyframes=8, max_points=CAP,
            max_keyframes=MAX_KF)


def mm_opts(ctx):
    return host.MapMaker.mapmaker_opts(ctx, ba=dict(deterministic=1))


def handle(scene, session=True, **kw):
    h = host.CameraTracker(scene.ctx_t, scene.snap, scene.mm, **dict(OPTS, **kw))
    if session:
        h.EnableSession(R.MAX_TRAILS, R.MIN_GOOD, R.THRESHOLD, init=scene.init_opts())
    return h


def fresh_state(h, frame):
    """Tracker::Reset's state at the identity with `frame` frames counted, as bytes"""
    s = h.tracker().track_state(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    s.frame = frame
    return bytes(s)


def same_trails(h, ref):
    a, b = h.trails(), ref.tr
    assert a.read().tobytes() == b.read().tobytes() and a.patches().tobytes() == b.patches().tobytes()


def to_the_second_poke(x, y=None):
    """f0 without a poke, f0 with one, f1 .. f4, f5 with the second poke -> the last frame's session row"""
    h = x.tracker
    before = fresh_state(h, 0)
    assert h.stage() == NOT_STARTED and bytes(h.state()) == before and h.pool() == (8, OPTS["keyframes"])
    t, s = h.SessionFrame(x.d_frames[0])
    assert t is None and (s["stage_before"], s["stage_after"], s["poked"], s["n_trails"]) == (NOT_STARTED, NOT_STARTED, 0, 0)
    assert bytes(h.state()) == fresh_state(h, 1)                      # nothing but the frame count
    t, s = h.SessionFrame(x.d_frames[0], poke=True)
    assert t is None and (s["stage_after"], s["poked"]) == (STARTED, 1) and s["n_trails"] >= 100
    if y is not None:
        y.idle()
        assert y.start(x.frames[0]) == s["n_trails"]
        same_trails(h, y)
    for k in range(1, 6):
        t, s = h.SessionFrame(x.d_frames[k], poke=k == 5)
        assert t is None and s["stage_before"] == STARTED and s["trail_reset"] == 0 and s["n_good"] >= s["n_alive"] >= 100
        if y is not None:
            assert y.advance(x.frames[k]) == (s["n_good"], s["n_alive"])
            same_trails(h, y)
        assert (s["stage_after"], s["init_requested"], s["poked"]) == ((COMPLETE, 1, 1) if k == 5 else (STARTED, 0, 0))
    assert bytes(h.state()) == fresh_state(h, 7) and s["init_tag"] == OPTS["tag_base"] + 6 and s["n_trails"] == s["n_alive"]
    assert h.pool() == (8, OPTS["keyframes"] - 2) and x.mm.InitPoll()[0] == S.MM_INIT_PENDING       # two clones are out
    return s


@pytest.fixture(scope="module")
def pair(hip):
    x, y = R.Scene(hip, mm_opts), R.Scene(hip, mm_opts)
    x.tracker = handle(x)
    ref = R.RefSession(y, **OPTS)
    yield x, y, ref
    ref.close()
    x.close()
    y.close()


def test_from_the_first_frame_to_tracked_frames_against_the_composition(pair):
    x, y, ref = pair
    h = x.tracker
    to_the_second_poke(x, ref)
    # before the mapmaker's step: no error, nothing tracked
    t, s = h.SessionFrame(x.d_frames[6])
    assert t is None and (s["stage_before"], s["stage_after"], s["init_done"], s["tracked"]) == (COMPLETE, COMPLETE, 0, 0)
    assert bytes(h.state()) == fresh_state(h, 8)
    got = x.mm.Step()
    assert got["status"] == S.MM_INIT and got["stages"] == S.MM_STAGE_INIT | S.MM_STAGE_PUBLISH
    want = ref.make_map()
    assert want["status"] == S.INIT_MAP_OK
    ref.begin(want, 8, -20)
    same_tables(x.rmap.tables(), y.rmap.tables())
    for n, k in enumerate((7, 8, 9)):
        t, s = h.SessionFrame(x.d_frames[k])
        w = y.tracker.TrackFrame(y.d_frames[k])
        assert s["tracked"] == 1 and (s["init_done"], s["init_status"]) == ((1, S.INIT_MAP_OK) if n == 0 else (0, 0))
        same_frame(t, w, "frame %d" % k)
        assert bytes(h.state()) == bytes(y.tracker.state()) and h.state().frame == 9 + n
        assert h.pool() == (y.tracker.pool()[0], y.tracker.pool()[1] - 2)            # the handle's first two clones are the map's
        assert t["branch"] == TRACKED and t["report"]["n_records"] > 20
        if n == 0:
            res = h.init_result()
            assert res["tracker_pose"].tobytes() == want["tracker_pose"].tobytes() and res["counts"] == want["counts"]
        sx, sy = x.mm.Step(), y.mm.Step()
        for key in ("status", "stages", "queue_size", "converged_recent", "converged_full", "notes", "bad_points", "insert"):
            assert sx[key] == sy[key], (k, key, sx[key], sy[key])
        tx, ty = x.rmap.tables(), y.rmap.tables()
        same_tables(tx, ty)
        check_invariants(tx)


def test_one_call_with_a_camera_in_its_trail_stage_and_a_camera_on_the_map(pair):
    """after the test above: the tracking handle and a second session handle (its own context, STARTED) in ONE call, against the
    composed tracker and a twin ptam_trails called separately"""
    x, y, ref = pair
    ctx2 = host.Context(lib=x.ctx_t.lib, size=x.ctx_t.size)
    d2 = [host.DevBuf(ctx2, np.ascontiguousarray(f)) for f in x.frames[:3]]
    h2 = host.CameraTracker(ctx2, x.snap, x.mm, **OPTS)
    h2.EnableSession(R.MAX_TRAILS, R.MIN_GOOD, R.THRESHOLD, init=x.init_opts())
    twin = R.RefSession(y, **OPTS)
    assert h2.SessionFrame(d2[0], poke=True)[1]["n_trails"] == twin.start(x.frames[0])
    for k in (1, 2):
        (t, s), (t2, s2) = host.CameraTracker.session_frames([x.tracker, h2], [x.d_frames[9 - k], d2[k]])
        same_frame(t, y.tracker.TrackFrame(y.d_frames[9 - k]), "mixed %d" % k)
        assert bytes(x.tracker.state()) == bytes(y.tracker.state())
        assert t2 is None and (s2["n_good"], s2["n_alive"]) == twin.advance(x.frames[k]) and s2["stage_after"] == STARTED
        same_trails(h2, twin)
    h2.close()
    twin.close()
    for d in d2:
        d.free()
    ctx2.close()


def test_a_handle_without_a_session_is_as_before(pair):
    """on the good map of the tests above: the session entry is track_frames; on an empty snapshot: no map"""
    x, _, _ = pair
    pose = x.tracker.init_result()["tracker_pose"]
    a, b = handle(x, session=False, keyframe_gap=100), handle(x, session=False, keyframe_gap=100)
    for h in (a, b):
        h.reset(pose)
        assert h.stage() == COMPLETE and h.trails() is None
    for k in (6, 7):
        t, s = a.SessionFrame(x.d_frames[k])
        w = b.TrackFrame(x.d_frames[k])
        assert s["tracked"] == 1 and (s["stage_before"], s["stage_after"]) == (COMPLETE, COMPLETE)
        assert t["track"].tobytes() == w["track"].tobytes() and bytes(a.state()) == bytes(b.state()) and a.pool() == b.pool()
        for key in ("branch", "quality", "frame", "added_keyframe", "noted_frame", "tag", "report"):
            assert t[key] == w[key], key
    a.close()
    b.close()
    e = R.Scene(x.ctx_t.lib, mm_opts)
    e.tracker = handle(e, session=False)
    before = bytes(e.tracker.state())
    assert e.tracker.SessionFrame(e.d_frames[0], check=False) == E_STATE == e.tracker.TrackFrame(e.d_frames[0], check=False)
    assert bytes(e.tracker.state()) == before
    e.close()


def test_a_blank_frame_resets_the_trails_and_a_new_start_works(hip):
    x = R.Scene(hip, mm_opts)
    h = x.tracker = handle(x)
    n0 = h.SessionFrame(x.d_frames[0], poke=True)[1]["n_trails"]
    assert h.SessionFrame(x.d_frames[1])[1]["n_good"] >= 100
    t, s = h.SessionFrame(x.d_blank, poke=True)                       # :329-332 comes before the poke is looked at
    assert t is None and (s["n_good"], s["n_alive"], s["trail_reset"], s["init_requested"]) == (0, 0, 1, 0)
    assert (s["stage_before"], s["stage_after"], s["poked"]) == (STARTED, NOT_STARTED, 1)
    assert bytes(h.state()) == fresh_state(h, 0) and h.pool() == (8, OPTS["keyframes"]) and x.mm.InitPoll()[0] == S.MM_INIT_NONE
    assert h.SessionFrame(x.d_frames[0], poke=True)[1]["n_trails"] == n0 and h.stage() == STARTED
    assert h.SessionFrame(x.d_frames[1])[1]["n_good"] >= 100
    x.close()


def test_two_cameras_in_their_trail_stage_share_one_chain(hip):
    """two STARTED handles in one call go through ptam_trails_advance_batch (one alone takes the per-camera calls): each against a twin"""
    xs = [R.Scene(hip, mm_opts), R.Scene(hip, mm_opts)]
    for x in xs:
        x.tracker = handle(x)
    twins = [R.RefSession(x, **OPTS) for x in xs]
    hs = [x.tracker for x in xs]
    order = ([0, 1, 2, 3], [0, 2, 3, 4])                              # the second camera skips a frame: other trails, other counts
    got = host.CameraTracker.session_frames(hs, [x.d_frames[0] for x in xs], [True, True])
    for (t, s), tw, x in zip(got, twins, xs):
        assert t is None and s["stage_after"] == STARTED and s["n_trails"] == tw.start(x.frames[0])
    for step in (1, 2, 3):
        got = host.CameraTracker.session_frames(hs, [x.d_frames[o[step]] for x, o in zip(xs, order)])
        for (t, s), tw, x, o in zip(got, twins, xs, order):
            assert t is None and (s["n_good"], s["n_alive"]) == tw.advance(x.frames[o[step]]) and s["n_alive"] >= 50
            same_trails(x.tracker, tw)
    for tw in twins:
        tw.close()
    for x in xs:
        x.close()


def test_two_pokes_on_a_still_frame_end_without_a_map(hip):
    x = R.Scene(hip, mm_opts)
    h = x.tracker = handle(x)
    h.SessionFrame(x.d_frames[0], poke=True)
    s = h.SessionFrame(x.d_frames[0], poke=True)[1]
    assert s["init_requested"] == 1 and s["n_good"] >= s["n_alive"] >= 100 and h.pool()[1] == OPTS["keyframes"] - 2
    step = x.mm.Step()
    assert step["stages"] == S.MM_STAGE_INIT and step["status"] == S.MM_IDLE
    t, s = h.SessionFrame(x.d_frames[1])
    assert t is None and s["init_done"] == 1 and s["init_status"] in (S.INIT_MAP_ZERO_BASELINE, S.INIT_MAP_NO_HOMOGRAPHY)
    assert (s["stage_before"], s["stage_after"]) == (COMPLETE, NOT_STARTED) and h.stage() == NOT_STARTED
    assert h.pool() == (8, OPTS["keyframes"]) and x.rmap.counts()["n_kf"] == 0 and x.rmap.counts()["n_points"] == 0
    assert h.init_result()["status"] == s["init_status"] and bytes(h.state()) == fresh_state(h, 0)
    assert h.SessionFrame(x.d_frames[0], poke=True)[1]["stage_after"] == STARTED                  # and the session starts again
    x.close()


def test_one_free_clone_at_the_second_poke_is_refused(hip):
    x = R.Scene(hip, mm_opts)
    h = x.tracker = handle(x, keyframes=1)
    h.SessionFrame(x.d_frames[0], poke=True)
    h.SessionFrame(x.d_frames[1])
    before = (bytes(h.state()), h.trails().read().tobytes(), h.trails().patches().tobytes(), h.pool(), h.stage())
    assert h.SessionFrame(x.d_frames[2], poke=True, check=False) == E_STATE
    assert (bytes(h.state()), h.trails().read().tobytes(), h.trails().patches().tobytes(), h.pool(), h.stage()) == before
    assert x.mm.InitPoll()[0] == S.MM_INIT_NONE
    assert h.SessionFrame(x.d_frames[2])[1]["n_good"] >= 100                                        # without the poke it goes on
    x.close()


def test_a_tracker_thread_and_a_mapmaker_thread(hip):
    """the tracker's thread pokes at frames 0 and 5 and goes on to ten tracked frames; the mapmaker's thread steps beside it"""
    x = R.Scene(hip, mm_opts)
    h = x.tracker = handle(x, keyframe_gap=3, reports=32, keyframes=12)
    made, done, errors, rows, tracked = threading.Event(), threading.Event(), [], [], []

    def tracking():
        try:
            for k in range(6):
                rows.append(h.SessionFrame(x.d_frames[k], poke=k in (0, 5))[1])
            made.wait()                                               # (the map: set by the step that made it, or by its failure)
            for k in range(10):
                t, s = h.SessionFrame(x.d_frames[6 + k % 4])
                rows.append(s)
                tracked.append(t)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    def mapping():
        try:
            while not done.is_set():
                if x.mm.Step()["stages"] & S.MM_STAGE_INIT:
                    made.set()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
        finally:
            made.set()
    th = [threading.Thread(target=tracking), threading.Thread(target=mapping)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert rows[5]["init_requested"] == 1 and rows[6]["init_done"] == 1 and rows[6]["init_status"] == S.INIT_MAP_OK
    assert all(t is not None for t in tracked) and tracked[-1]["branch"] == TRACKED and h.stage() == COMPLETE
    for _ in range(4):
        x.mm.Step()
    assert x.mm.QueueSize() == 0
    added = sum(t["added_keyframe"] for t in tracked)
    last = h.SessionFrame(x.d_frames[8])[0]                           # reads what the mapmaker released: every tag is home
    out_now = int(bool(last["added_keyframe"] or last["noted_frame"]))
    assert h.pool() == (32 - out_now, 12 - 2 - added - last["added_keyframe"])
    tab = x.rmap.tables()
    check_invariants(tab)
    assert len(tab["poses"]) == 2 + added
    x.close()
