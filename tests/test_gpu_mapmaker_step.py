"""-m gpu: ptam_mapmaker_step (host.MapMaker.Step) against tests/mapmaker_run_ref.RefMapMaker, the same loop in Python over the
separate calls, on a second resident map with its own snapshot, tracker and finder.  After every step: the step's result (status,
stages, every stage's counts, the flags, the queue, the draws) by ==, every table by tobytes(), check_invariants, the released tags.
Every bundle is deterministic.  The scene is tests/test_gpu_map_publish.py's (3 keyframes, about 600 points); more keyframes are the
new keyframe's image queued again under other poses."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import insert_keyframe_ref as I
from tests.mapmaker_run_ref import RefMapMaker
from tests.test_gpu_map_publish import TRACKER_CAP, dev, uploaded  # noqa: F401  (dev: the scene's fixture)
from tests.test_gpu_resident_map import check_invariants, same_tables

pytestmark = pytest.mark.gpu
EPI = dict(min_shi_tomasi=I.THRESHOLD)
BA = dict(deterministic=1)
S = _abi
ONLY_INSERT = S.MM_STAGE_BAD_POINTS | S.MM_STAGE_ADD_KEYFRAME | S.MM_STAGE_PUBLISH


class Side:
    """a resident map of the scene with its snapshot, tracker and finder, and the mapmaker over them: the handle or the reference"""

    def __init__(self, d, ref, snapshot=True, empty=False, **kw):
        self.d, self.ctx = d, d["ctx"]
        self.m = host.ResidentMap(self.ctx) if empty else uploaded(self.ctx, d["h"], list(d["kfs"]))
        self.snap = host.MapSnapshot(self.ctx, TRACKER_CAP) if snapshot else None
        self.tr, self.rf = host.Tracker(self.ctx, TRACKER_CAP), host.ReFinder(self.ctx)
        self.reports, self.frames = [], 0
        if ref:
            self.mm = RefMapMaker(self.m, self.rf, self.snap, ba=BA, **dict(EPI, **kw))
        else:
            self.mm = host.MapMaker(self.ctx, self.m, self.rf, self.snap,
                                    host.MapMaker.mapmaker_opts(self.ctx, ba=BA, **dict(EPI, **kw)))
        self.own = host.MapSnapshot(self.ctx, TRACKER_CAP)     # what this side's tracker takes: never the mapmaker's own snapshot,
                                                                 # so that a step's publish count stays the step's

    def report(self, tag):
        """the map as it stands to the tracker, one tracked frame, its report"""
        self.m.publish(self.own)
        self.tr.take_map(self.own)
        n = self.tr.n
        rng = np.random.default_rng(100 + self.frames)
        self.frames += 1
        self.tr.set_shuffle(rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32))
        self.tr.TrackMap(self.d["ka"], self.d["sp"], self.tr.opts())
        rep = host.FrameReport(self.ctx, TRACKER_CAP)
        info = self.tr.report_frame(rep, tag=tag)
        assert info["n_records"] > 20
        self.reports.append(rep)
        return rep

    def queue_keyframe(self, tag, i, kf=None, **kw):
        pose = self.d["sp"].copy()
        pose[9] += 0.015 * i                                     # another camera centre for every queued keyframe
        self.mm.AddKeyFrame(self.d["ka"] if kf is None else kf, pose, 0, self.report(tag), I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], tag, **kw)

    def close(self):
        if hasattr(self.mm, "close"):
            self.mm.close()
        for x in self.reports + [self.tr, self.rf, self.own] + ([self.snap] if self.snap else []) + [self.m]:
            x.close()


def sides(d, **kw):
    return Side(d, False, **kw), Side(d, True, **kw)


def step_both(a, b):
    """one step on both sides, compared -> the handle's result"""
    got, ref = a.mm.Step(), b.mm.Step()
    for k in ref:
        if k == "publish":
            assert {f: v for f, v in got[k].items() if f != "map_id"} == {f: v for f, v in ref[k].items() if f != "map_id"}, k
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])
    assert set(got) == set(ref)
    ta, tb = a.m.tables(), b.m.tables()
    same_tables(ta, tb)
    if len(ta["poses"]):
        check_invariants(ta)
    assert np.array_equal(a.m.point_serials(), b.m.point_serials())
    assert a.mm.flags() == b.mm.flags() and a.mm.QueueSize() == b.mm.QueueSize() == got["queue_size"]
    ra, rb = a.mm.released(), b.mm.released()
    assert ra == rb
    return got, ra


def close_all(*xs):
    for x in xs:
        x.close()


def test_three_keyframes_recent_is_skipped_and_the_flag_is_set(dev):
    a, b = sides(dev)
    for s in (a, b):
        s.mm.set_flags(0, 0)
    got, _ = step_both(a, b)
    # :790-793 sets the flag, so the same step goes on to the new points and the full bundle
    assert got["stages"] & S.MM_STAGE_BUNDLE_RECENT == 0 and got["recent"]["ran"] == 0
    assert got["stages"] & S.MM_STAGE_REFIND_NEW and got["stages"] & S.MM_STAGE_BUNDLE_ALL and got["all"]["ran"] == 1
    assert got["converged_recent"] == 1 and got["draws"] == got["converged_full"] and got["refind_new"]["n_pairs"] > 0   # (:103: both flags)
    assert bool(got["stages"] & S.MM_STAGE_PUBLISH) == (got["all"]["accepted"] > 0 or got["bad_points"]["n_removed"] > 0)
    close_all(a, b)


@pytest.mark.parametrize("recent,full", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_every_flag_state_with_an_empty_queue(dev, recent, full):
    """the rows of the decision table with queue == 0, failure_period = 1 (every draw hits); no snapshot: never a publish"""
    a, b = sides(dev, snapshot=False, failure_period=1)
    for s in (a, b):
        s.mm.set_flags(recent, full)
    got, _ = step_both(a, b)
    assert got["stages"] & S.MM_STAGE_PUBLISH == 0 and got["stages"] & S.MM_STAGE_BAD_POINTS
    if recent and full:
        assert got["stages"] & S.MM_STAGE_REFIND_FAILURE and got["draws"] == 1 and got["stages"] & S.MM_STAGE_BUNDLE_ALL == 0
    step_both(a, b)
    close_all(a, b)


def test_a_draw_is_consumed_only_when_both_flags_are_set(dev):
    a, b = sides(dev, snapshot=False, failure_period=3, failure_seed=7)
    hits = 0
    for i in range(6):                                           # both flags stay set: nothing clears them
        got, _ = step_both(a, b)
        assert got["draws"] == i + 1
        hits += bool(got["stages"] & S.MM_STAGE_REFIND_FAILURE)
    assert 0 < hits < 6
    for s in (a, b):
        s.mm.set_flags(1, 0)
    got, _ = step_both(a, b)                                     # the full bundle runs; a draw follows only if it leaves both flags set
    assert got["stages"] & S.MM_STAGE_BUNDLE_ALL and got["draws"] == 6 + int(got["converged_recent"] and got["converged_full"])
    close_all(a, b)


def test_a_queued_keyframe_only_bad_points_and_the_insert_run(dev):
    a, b = sides(dev)
    for s in (a, b):
        s.mm.set_flags(0, 0)
        s.queue_keyframe(11, 1)
        s.queue_keyframe(12, 2)
    got, rel = step_both(a, b)
    assert got["stages"] == ONLY_INSERT and got["queue_size"] == 1 and rel == [11]
    assert got["insert"]["kf"] == 3 and got["insert"]["n_rows"] > 20 and (got["converged_recent"], got["converged_full"]) == (0, 0)
    assert got["publish"]["n_kf"] == 4 and got["publish"]["generation"] == 1
    got, rel = step_both(a, b)
    assert got["stages"] == ONLY_INSERT and got["queue_size"] == 0 and rel == [12] and got["publish"]["generation"] == 2
    close_all(a, b)


def test_a_keyframe_without_its_rest_gets_it(dev):
    a, b = sides(dev)
    kfs = [host.KeyFrame(dev["ctx"]).MakeKeyFrame_Lite(I.views()["ia"]) for _ in range(2)]
    a.queue_keyframe(5, 1, kf=kfs[0])
    b.queue_keyframe(5, 1, kf=kfs[1], rest_made=False)
    got, rel = step_both(a, b)
    assert got["stages"] & S.MM_STAGE_ADD_KEYFRAME and got["insert"]["n_made"] > 0 and rel == [5]
    close_all(a, b)
    close_all(*kfs)


def test_pending_notes_are_counted_before_the_bad_points(dev):
    """Every third point has 21 outlier votes and no inlier vote: HandleBadPoints removes it (:136) unless the pending report,
    noted 22 times, is counted first and gives the points it found as inliers 22 inlier votes."""
    a, b = sides(dev)
    for s in (a, b):
        rep = s.report(21)
        for _ in range(22):
            s.mm.NoteFrame(rep, 21)
        voted = np.arange(0, s.m.counts()["n_points"], 3, dtype=np.int32)
        s.m.note_tracked(np.repeat(voted, 21), np.ones(21 * len(voted), np.uint8))
    rec = a.reports[-1].read()
    saved, _ = a.m.resolve_serials(rec["serial"][rec["outlier"] == 0])
    expect = len(np.setdiff1d(voted, saved))
    assert 0 < expect < len(voted)
    got, rel = step_both(a, b)
    assert got["stages"] & S.MM_STAGE_NOTES and got["notes"]["n_records"] == 22 * len(rec) and rel == [21] * 22
    assert got["bad_points"]["n_removed"] == expect and got["stages"] & S.MM_STAGE_PUBLISH
    close_all(a, b)


def test_a_reset_and_an_empty_map(dev):
    a, b = sides(dev)
    for s in (a, b):
        s.queue_keyframe(31, 1)
        s.mm.NoteFrame(s.report(32), 32)
        s.mm.set_flags(0, 0)
        s.mm.RequestReset()
        assert not s.mm.ResetDone()
    got, rel = step_both(a, b)
    assert got["status"] == S.MM_RESET and got["stages"] == 0 and sorted(rel) == [31, 32] and got["queue_size"] == 0
    assert (got["converged_recent"], got["converged_full"]) == (1, 1) and a.mm.ResetDone() and b.mm.ResetDone()
    assert a.m.counts()["n_kf"] == 0
    got, rel = step_both(a, b)                                   # an empty map: nothing to do (:79)
    assert got["status"] == S.MM_IDLE and got["stages"] == 0 and rel == []
    close_all(a, b)
    a, b = sides(dev, empty=True)
    assert step_both(a, b)[0]["status"] == S.MM_IDLE
    close_all(a, b)


def test_from_two_queued_keyframes_to_nine_and_to_convergence(dev):
    """two keyframes queued, then four more: nine keyframes, where BundleAdjustRecent runs; then steps until both flags are set and
    the queue is empty.  Every tag comes back exactly once."""
    a, b = sides(dev, failure_period=1)
    tags, seen, stages = list(range(100, 106)), [], 0
    for s in (a, b):
        for i, t in enumerate(tags[:2]):
            s.queue_keyframe(t, i + 1)
    for i, t in enumerate(tags[2:]):
        got, rel = step_both(a, b)
        seen += rel
        for s in (a, b):
            s.queue_keyframe(t, i + 3)
    for _ in range(40):                                          # the bound: 6 inserts, then a few bundles of 9 keyframes
        got, rel = step_both(a, b)
        seen += rel
        stages |= got["stages"]
        if got["converged_recent"] and got["converged_full"] and got["queue_size"] == 0:
            break
    else:
        pytest.fail("no convergence in 40 steps: %r" % (got,))
    assert a.m.counts()["n_kf"] == 9 and sorted(seen) == tags
    assert stages & S.MM_STAGE_BUNDLE_RECENT and stages & S.MM_STAGE_BUNDLE_ALL and stages & S.MM_STAGE_REFIND_NEW
    got, _ = step_both(a, b)                                     # converged: the failure queue's turn
    assert got["stages"] & S.MM_STAGE_REFIND_FAILURE
    close_all(a, b)
