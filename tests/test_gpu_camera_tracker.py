"""-m gpu: ptam_camera_tracker (host.CameraTracker) — one frame of Tracker::TrackFrame for a good map with its hand-over as one call —
against tests/camera_tracker_ref.py, the same frame composed in Python from the existing calls.  Each side has its own resident map,
snapshot, finder and host.MapMaker (tests/camera_tracker_ref.Scene).  Results, states, report records, iteration sets, the map's
tables after a Step and the released tags are compared by == / tobytes(); a map's id is its own and is left out."""
import threading

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import camera_tracker_ref as R
from tests.test_gpu_mapmaker_step import BA, EPI
from tests.test_gpu_resident_map import check_invariants, same_tables

pytestmark = pytest.mark.gpu
E_STATE = -3
OPTS = dict(keyframe_gap=1, max_queue=3, shuffle_seed=0x9E3779B97F4A7C15, tag_base=1000, reports=8, keyframes=8, max_points=R.CAP,
            max_keyframes=R.MAX_KF)


def mm_opts(ctx):
    return host.MapMaker.mapmaker_opts(ctx, ba=BA, **EPI)


def no_id(d):
    return {k: v for k, v in d.items() if k != "map_id"}


def same_frame(got, want, tag):
    """a frame's result through the handle and through the composition"""
    assert got["track"].tobytes() == want["track"].tobytes(), tag
    for k in ("branch", "quality", "lost_frames", "frame", "added_keyframe", "noted_frame", "queue_size", "tag"):
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert no_id(got["report"]) == no_id(want["report"]), (tag, got["report"], want["report"])
    assert no_id(got["map_take"]) == no_id(want["map_take"]) and no_id(got["keyframes_take"]) == no_id(want["keyframes_take"]), tag
    gi, wi = got["info"], want["info"]
    assert (gi.closest_kf, gi.closest_kf_dist, gi.need_new_keyframe, gi.want_keyframe) == \
        (wi["closest_kf"], wi["closest_kf_dist"], wi["need_new_keyframe"], wi["want_keyframe"]), tag
    assert np.array(gi.frame.pose_in).tobytes() == wi["pose_in"].tobytes() and np.array(gi.reloc.pose).tobytes() == wi["reloc"]["pose"].tobytes(), tag
    assert (gi.reloc.best, bool(gi.reloc.good), gi.reloc.best_ssd) == (wi["reloc"]["best"], wi["reloc"]["good"], wi["reloc"]["best_ssd"]), tag


class Pair:
    """the handle on its scene (x) and the composition on a twin scene (y)"""

    def __init__(self, hip, **kw):
        o = dict(OPTS, **kw)
        self.x, self.y = R.Scene(hip, mm_opts), R.Scene(hip, mm_opts)
        self.x.tracker = host.CameraTracker(self.x.ctx_t, self.x.snap, self.x.mm, **o)
        self.y.tracker = R.RefCameraTracker(self.y.ctx_t, self.y.snap, self.y.mm, **o)
        pose = self.x.poses[0]
        self.x.tracker.reset(pose)
        self.y.tracker.reset(pose)

    def frame(self, k, tag, both=True):
        """frame k of the sequence (None: a blank frame) on both sides -> the handle's result"""
        dx = self.x.d_blank if k is None else self.x.d_frames[k]
        dy = self.y.d_blank if k is None else self.y.d_frames[k]
        got = self.x.tracker.TrackFrame(dx)
        want = self.y.tracker.TrackFrame(dy)
        self.check(got, want, tag)
        return got

    def check(self, got, want, tag):
        same_frame(got, want, tag)
        assert bytes(self.x.tracker.state()) == bytes(self.y.tracker.state()), tag
        assert self.x.tracker.pool()[0] == self.y.tracker.pool()[0], tag
        if got["branch"] != R.FAILED:
            assert self.x.tracker.tracker().iteration_set().tobytes() == self.y.tracker.tr.iteration_set().tobytes(), tag
            rx, ry = self.x.tracker.last_report(), self.y.tracker.last_report
            assert rx.read().tobytes() == ry.read().tobytes(), tag

    def step(self, tag):
        sx, sy = self.x.mm.Step(), self.y.mm.Step()
        for k in ("status", "stages", "queue_size", "converged_recent", "converged_full", "notes", "bad_points"):
            assert sx[k] == sy[k], (tag, k, sx[k], sy[k])
        assert {k: v for k, v in sx["insert"].items()} == {k: v for k, v in sy["insert"].items()}, tag
        tx, ty = self.x.rmap.tables(), self.y.rmap.tables()
        same_tables(tx, ty)
        check_invariants(tx)
        return sx

    def close(self):
        self.x.close()
        self.y.close()


@pytest.fixture(scope="module")
def pair(hip):
    p = Pair(hip)
    yield p
    p.close()


def test_frames_steps_loss_and_recovery_against_the_composition(pair):
    seen = []
    # frames 0-6 without a step: with a gap of 1 every other frame is far enough; keyframes go in until the queue holds 3, then the
    # frames are noted although they are far enough
    for k in range(7):
        seen.append(pair.frame(k, "frame %d" % k))
    assert [r["added_keyframe"] for r in seen] == [1, 0, 1, 0, 1, 0, 0] and [r["noted_frame"] for r in seen] == [0, 1, 0, 1, 0, 1, 1]
    assert [r["queue_size"] for r in seen] == [0, 1, 1, 2, 2, 3, 3] and all(r["report_in_chain"] == 1 and r["report"]["n_records"] > 100 for r in seen)
    assert [r["tag"] for r in seen] == [1000 + k for k in range(7)] and seen[0]["map_take"]["changed"] == 1 and seen[1]["map_take"]["changed"] == 0
    assert pair.x.tracker.pool() == (1, 5)
    # a step on both sides: the notes are counted, the first keyframe enters the map, the map is published
    s = pair.step("step 1")
    assert s["insert"]["n_made"] >= 0 and s["queue_size"] == 2 and s["notes"]["n_records"] > 100
    # the next frame reads the released tags on both sides (the four notes and the first keyframe: five reports are free again, the
    # clone stays with the map) and takes the new map and its four keyframes
    got = pair.frame(7, "the frame after the step")
    assert got["map_take"]["changed"] == 1 and got["keyframes_take"]["n_kf"] == 4 and got["map_take"]["n_points"] >= pair.x.n0
    handed = int(bool(got["added_keyframe"] or got["noted_frame"]))
    assert pair.x.tracker.pool() == (1 + 5 - handed, 8 - 3 - got["added_keyframe"]) and pair.y.tracker.pool()[0] == 1 + 5 - handed
    pair.step("step 2")
    pair.frame(6, "the frame after the second step")


def test_loss_recovery_and_a_recovery_that_fails(hip):
    """cameras A and A2 (another seed): three blank frames, then the sequence again — RECOVERED; both in ONE call on the handle's
    side, one after the other in the composition.  Camera B (reloc_max_score 1) never recovers"""
    a, a2, b = Pair(hip), Pair(hip, shuffle_seed=77), Pair(hip, state=dict(reloc_max_score=1.0))
    branches = {"a": [], "a2": [], "b": []}
    for k in (0, None, None, None, 4, 5):
        dx = [p.x.d_blank if k is None else p.x.d_frames[k] for p in (a, a2)]
        got = host.CameraTracker.track_frames([a.x.tracker, a2.x.tracker], dx)
        for p, g, name in ((a, got[0], "a"), (a2, got[1], "a2")):
            want = p.y.tracker.TrackFrame(p.y.d_blank if k is None else p.y.d_frames[k])
            p.check(g, want, "camera %s frame %s" % (name, k))
            branches[name].append(g["branch"])
        branches["b"].append(b.frame(k, "camera b frame %s" % k)["branch"])
    assert branches["a"] == branches["a2"] == [R.TRACKED] * 4 + [R.RECOVERED, R.TRACKED]
    assert branches["b"] == [R.TRACKED] * 4 + [R.FAILED, R.FAILED]
    # one call, one set of options: handles whose options differ are refused
    assert host.CameraTracker.track_frames([a.x.tracker, b.x.tracker], [a.x.d_frames[6], b.x.d_frames[6]], check=False) == -1
    # pool exhaustion: a handle with one report has it out after its first frame
    c = Pair(hip, reports=1)
    first = c.frame(0, "one report")
    assert first["added_keyframe"] == 1 and c.x.tracker.pool() == (0, 7)
    before = bytes(c.x.tracker.state())
    assert c.x.tracker.TrackFrame(c.x.d_frames[1], check=False) == E_STATE
    assert bytes(c.x.tracker.state()) == before and c.x.tracker.pool() == (0, 7) and c.x.mm.QueueSize() == 1
    c.step("the step that releases it")
    c.frame(1, "after the release")
    # reset: the state of ptam_track_state_reset, every report and clone back
    c.x.tracker.reset(c.x.poses[3])
    assert bytes(c.x.tracker.state()) == bytes(c.x.tracker.tracker().track_state(c.x.poses[3])) and c.x.tracker.pool() == (1, 8)
    for p in (a, a2, b, c):
        p.close()


def test_a_tracker_thread_and_a_mapmaker_thread(hip):
    """20 frames on the tracker's thread, 30 steps on the mapmaker's; the interleaving is free, so nothing is compared with a twin"""
    s = R.Scene(hip, mm_opts)
    s.tracker = host.CameraTracker(s.ctx_t, s.snap, s.mm, **dict(OPTS, keyframe_gap=3, keyframes=12, reports=32))
    s.tracker.reset(s.poses[0])
    results, steps, errors = [], [], []

    def tracking():
        try:
            for k in range(20):
                results.append(s.tracker.TrackFrame(s.d_frames[k % 14 if k % 14 < 8 else 14 - k % 14]))     # 0 .. 7, 6 .. 1, 0 ..
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    def mapping():
        try:
            for _ in range(30):
                steps.append(s.mm.Step())
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    th = [threading.Thread(target=tracking), threading.Thread(target=mapping)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert len(results) == 20 and len(steps) == 30
    for _ in range(4):                                   # whatever is still queued (at most max_queue keyframes) and pending
        s.mm.Step()
    assert s.mm.QueueSize() == 0
    added = sum(r["added_keyframe"] for r in results)
    handed = [r["tag"] for r in results if r["added_keyframe"] or r["noted_frame"]]
    assert added >= 1 and len(set(handed)) == len(handed) >= 10
    last = s.tracker.TrackFrame(s.d_frames[4])           # reads what the mapmaker released: every tag came back
    out_now = int(bool(last["added_keyframe"] or last["noted_frame"]))
    assert s.tracker.pool() == (32 - out_now, 12 - added - last["added_keyframe"])
    tab = s.rmap.tables()
    check_invariants(tab)
    assert len(tab["poses"]) == 3 + added
    s.close()
