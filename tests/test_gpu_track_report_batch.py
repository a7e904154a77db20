"""-m gpu: ptam_track_frames_report_batch — ptam_track_frames_recover_batch with every frame's report filled inside the chain and the
frame's two random orders drawn there — against the sequence it replaces on twin cameras: ptam_shuffle_order_host + ptam_tracker_set_shuffle,
ptam_track_frames_recover_batch, ptam_tracker_report_frames.  Both sides run the same kernels on the same data: results, states, infos,
iteration sets, report infos and report records are compared by == / tobytes(), nothing else.
The cameras are those of tests/test_gpu_track_recover_batch.py; their maps go through a resident map and a snapshot, because a frame
report names points by the serials a take hands over."""
import numpy as np
import pytest

from ptam_cg_amd import host, synth
from tests import sbi_cases as SC
from tests import track_state_ref as T
from tests.test_gpu_map_publish import synthetic, uploaded
from tests.test_gpu_track_recover_batch import RecCamera, _blank, _copy_state, _sequence_bank
from tests.test_gpu_trackmap import _setup

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3
SEED = 0x2545F4914F6CDD1D
GS_LIMIT = 1024                      # the fused pose kernels' slots (trackmap.hip): a longer fine list takes the long path
EMPTY = dict(map_id=0, tag=0, n_records=0, n_entries=0, n_outliers=0)


def same(a, b):
    """dicts, lists, arrays and scalars, to the byte"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def map_tables(world, pixel_right_w, pixel_down_w, src_level, center):
    """whole-map tables of a tracking map whose points all come from keyframe 0"""
    n = len(world)
    h = synthetic(n, K=1)
    p = h["points"]
    p["pv"]["world"], p["pv"]["pixel_right_w"], p["pv"]["pixel_down_w"] = world, pixel_right_w, pixel_down_w
    p["src_kf"], p["src_level"] = 0, src_level
    c = np.asarray(center, np.int32).reshape(n, 2)
    p["center_x"], p["center_y"] = c[:, 0], c[:, 1]
    h["sources"]["src_kf"] = 0
    h["points3"] = np.ascontiguousarray(p["pv"]["world"])
    return h


class Serials:
    """a tracking map published through a resident map: trackers that take it know their points' serials"""

    def __init__(self, ctx, kf0, m):
        self.n = len(m["world"])
        self.rmap = uploaded(ctx, map_tables(m["world"], m["pixel_right_w"], m["pixel_down_w"], m["src_level"], m["center"]), kfs=[kf0])
        self.snap = host.MapSnapshot(ctx, max(self.n, 32))
        self.rmap.publish(self.snap)

    def give(self, tr):
        r = tr.take_map(self.snap)
        assert r["changed"] and r["n_points"] == self.n and r["map_id"] != 0
        self.map_id = r["map_id"]
        return tr

    def close(self):
        self.snap.close()
        self.rmap.close()


class Cam(RecCamera):
    """a camera of the recover batch whose tracker took its map from a snapshot, with a report of its own"""

    def __init__(self, hip, bank=True, **kw):
        super().__init__(hip, **kw)
        self.ser = Serials(self.ctx, self.kf0, self.map)
        self.ser.give(self.tr)
        self.n = self.ser.n
        self.report = host.FrameReport(self.ctx, max(self.n, 1))
        if bank:
            _sequence_bank(self)

    def close(self):
        self.report.close()
        self.ser.close()
        super().close()


def chain(cams, ks, state_opts=None, opts=None, seeds=True, reports=None, check=True):
    """one ptam_track_frames_report_batch, camera i on its frame ks[i], tag = 100 i + the frame's number"""
    return host.Tracker.track_frames_report_batch(
        [c.tr for c in cams], [c.kf for c in cams], [c.d_frames[k] for c, k in zip(cams, ks)], [c.state for c in cams], [c.est for c in cams],
        [c.rel for c in cams], opts, state_opts, reports=[c.report for c in cams] if reports is None else reports,
        tags=[100 * i + c.state.frame for i, c in enumerate(cams)], shuffle_seeds=[SEED + i for i in range(len(cams))] if seeds else None, check=check)


def composed(cams, ks, state_opts=None, opts=None, seeds=True):
    """what the chain replaces -> (results, infos, the reports' infos or None for a frame that tracked nothing)"""
    tags = [100 * i + c.state.frame for i, c in enumerate(cams)]
    if seeds:
        for i, c in enumerate(cams):
            c.tr.set_shuffle(*[host.shuffle_order(c.lib, SEED + i, c.state.frame, w, c.n) for w in (0, 1)])
    res, infos = host.Tracker.track_frames_recover_batch([c.tr for c in cams], [c.kf for c in cams], [c.d_frames[k] for c, k in zip(cams, ks)],
                                                         [c.state for c in cams], [c.est for c in cams], [c.rel for c in cams], opts, state_opts)
    rinfos = []
    for c, f, tag in zip(cams, infos, tags):
        rinfos.append(None if f["branch"] == T.RECOVERY_FAILED else c.tr.report_frame(c.report, tag))
    return res, infos, rinfos


def but_map(info):
    """a report's info without the map's id: every resident map has its own (the serials count from 1 in each)"""
    return {k: v for k, v in info.items() if k != "map_id"}


def assert_same_frame(X, Y, got, want, tag):
    """cameras X (the chain) and Y (the composition) after one call each"""
    (res, infos, rinfos, rc), (res2, infos2, rinfos2) = got, want
    assert rc == 0, tag
    assert res.tobytes() == res2.tobytes(), tag
    assert same(infos, infos2), tag
    for i, (x, y) in enumerate(zip(X, Y)):
        assert bytes(x.state) == bytes(y.state), (tag, i)
        if rinfos2[i] is None:      # a failed recovery: nothing was tracked, the tracker still holds the frame before — the report is empty
            assert infos[i]["branch"] == T.RECOVERY_FAILED
            assert rinfos[i] == dict(EMPTY, report_in_chain=1, report_too_small=0) and x.report.info() == EMPTY, (tag, i)
            continue
        assert x.tr.iteration_set().tobytes() == y.tr.iteration_set().tobytes(), (tag, i)
        assert y.report.info() == rinfos2[i] and rinfos2[i]["map_id"] == y.ser.map_id, (tag, i)
        assert but_map(x.report.info()) == but_map(rinfos2[i]) and x.report.info()["map_id"] == x.ser.map_id, (tag, i, x.report.info(), rinfos2[i])
        assert rinfos[i] == dict(x.report.info(), report_in_chain=1, report_too_small=0), (tag, i)
        assert x.report.read().tobytes() == y.report.read().tobytes(), (tag, i)


# ---- 1. four cameras over seven rounds: tracked, lost, three blank frames, recovered, tracked; one that never recovers --------------------
@pytest.fixture(scope="module")
def sides(hip):
    """two equal sets of tests/test_gpu_track_recover_batch.py's four cameras: X for the chain, Y for the composition"""
    seq = SC.tracking_sequence()[0]
    f1 = [seq[0], _blank(), _blank(), _blank(), seq[4], seq[5], seq[6]]
    out = [[Cam(hip), Cam(hip, frames=f1), Cam(hip, estimator=False), Cam(hip)] for _ in range(2)]
    yield out
    for cams in out:
        for c in cams:
            c.close()


def test_seven_rounds_equal_the_composition(sides):
    X, Y = sides
    for cams in sides:
        cams[3].lose()
    never = X[3].tr.state_opts(reloc_max_score=1.0)
    branches, records = [], []
    for rnd in range(7):
        got = chain(X[:3], [rnd] * 3)
        want = composed(Y[:3], [rnd] * 3)
        assert_same_frame(X[:3], Y[:3], got, want, "round %d" % rnd)
        branches.append(got[1][1]["branch"])
        records.append([r["n_records"] for r in got[2]])
        assert [r["tag"] for r in got[2]] == [100 * i + rnd for i in range(3)]
        # camera 3: lost, and no alignment scores below 1.  Its report held another frame's records before the call
        k3 = 1 + rnd % 6
        ser, it = X[3].tr.point_serials(), X[0].tr.iteration_set()
        assert X[3].report.from_host(5, ser, it)["n_records"] > 100
        got3 = chain([X[3]], [k3], never)
        want3 = composed([Y[3]], [k3], never)
        assert want3[2] == [None]
        assert_same_frame([X[3]], [Y[3]], got3, want3, "round %d camera 3" % rnd)
        assert X[3].lib.frame_report_read(X[3].report.h, 0, 1, None) == E_ARG          # nothing to read: not the records it held
    assert branches == [T.TRACKED] * 4 + [T.RECOVERED] + [T.TRACKED] * 2
    assert all(r[0] > 100 and r[2] > 100 for r in records)
    assert [r[1] for r in records][1:4] == [0, 0, 0] and records[4][1] > 100             # the blank frames find nothing; the recovery does


def test_without_seeds_the_shuffles_are_the_callers(sides):
    """shuffle_seeds NULL: the orders set through ptam_tracker_set_shuffle stand, as in the recover batch"""
    X, Y = sides
    n = X[2].n
    rng = np.random.default_rng(8)
    pa, pb = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    for c in (X[2], Y[2]):
        c.state = c.tr.track_state(c.poses[0])
        c.tr.set_shuffle(pa, pb)
    got = chain([X[2]], [1], seeds=False)
    want = composed([Y[2]], [1], seeds=False)
    assert_same_frame([X[2]], [Y[2]], got, want, "no seeds")
    a, b = X[2].tr.read_shuffle()
    assert np.array_equal(a, pa) and np.array_equal(b, pb)


# ---- 2. a report too small for its frame ------------------------------------------------------------------------------------------
def test_a_report_one_record_too_small(sides):
    X, Y = sides
    for c in (X[0], X[2], Y[0], Y[2]):
        c.state = c.tr.track_state(c.poses[0])
    want = composed([Y[0], Y[2]], [0, 0])
    found = want[2][1]["n_records"]
    assert found > 100
    small = host.FrameReport(X[2].ctx, found - 1)
    res, infos, rinfos, rc = chain([X[0], X[2]], [0, 0], reports=[X[0].report, small])
    assert rc == E_ARG                                                       # ... and every frame is delivered, every state has moved
    assert res.tobytes() == want[0].tobytes() and same(infos, want[1])
    assert bytes(X[0].state) == bytes(Y[0].state) and bytes(X[2].state) == bytes(Y[2].state)
    assert small.info() == EMPTY and rinfos[1] == dict(EMPTY, report_in_chain=1, report_too_small=1) and rinfos[0]["report_too_small"] == 0
    assert but_map(X[0].report.info()) == but_map(want[2][0]) and X[0].report.read().tobytes() == Y[0].report.read().tobytes()
    for c in (X[0], X[2], Y[0], Y[2]):
        c.state = c.tr.track_state(c.poses[0])
    want = composed([Y[0], Y[2]], [1, 1])
    exact = host.FrameReport(X[2].ctx, want[2][1]["n_records"])             # exactly as many records as the frame has
    res, infos, rinfos, rc = chain([X[0], X[2]], [1, 1], reports=[X[0].report, exact])
    assert rc == 0 and but_map(rinfos[1]) == but_map(dict(want[2][1], report_in_chain=1, report_too_small=0)) and rinfos[1]["n_records"] == exact.info()["n_records"] > 100
    assert exact.read().tobytes() == Y[2].report.read().tobytes()
    for r in (small, exact):
        r.close()


# ---- 3. the smallest chain: empty maps ---------------------------------------------------------------------------------------------------
def test_two_cameras_with_empty_maps(hip):
    size = (163, 121)
    seq = SC.tracking_sequence()[0]
    fr = [np.ascontiguousarray(f[:size[1], :size[0]]) for f in seq[:3]]
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    cams = [Cam(hip, bank=False, size=size, empty=True, frames=fr) for _ in range(2)]
    for c in cams:
        c.state = c.tr.track_state(pose)
    for k in range(2):
        res, infos, rinfos, rc = chain(cams, [k, k + 1])
        assert rc == 0 and [f["branch"] for f in infos] == [T.TRACKED] * 2
        for c, r in zip(cams, rinfos):
            assert r == dict(map_id=c.report.info()["map_id"], tag=r["tag"], n_records=0, n_entries=0, n_outliers=0, report_in_chain=1, report_too_small=0)
            assert r["map_id"] != 0 and c.state.frame == k + 1
        assert not res["n_meas"].any()
    for c in cams:
        c.close()


# ---- 4. a frame on the long path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile, budget, long_path", [(1, 2000, True), (4, 1000, False), (4, 2000, True)],
                         ids=["2561pts_long_path", "10244pts_drawn_in_the_chain", "10244pts_long_path"])
def test_large_maps_and_the_long_path(hip, tile, budget, long_path):
    """2 561 points and a patch budget of 2 000: the fine pose list outgrows the fused kernel's 1 024 slots, the frame is finished by
    launches the host enqueues behind the wait, and its report with it.  The same map four times over, 10 244 points: more than the
    draw sorts in LDS — inside the chain the orders come from the sort in global memory, camera by camera"""
    ctx, kfa, kfb, case = _setup(hip, (1000, 900, 700, 500))
    case = {k: np.concatenate([case[k]] * tile) if k in ("world", "pixel_right_w", "pixel_down_w", "src_level", "center") else case[k] for k in case}
    _, b = synth.make_frame_pair()
    d_frame = host.DevBuf(ctx, np.ascontiguousarray(b))
    n = len(case["world"])
    ser = Serials(ctx, kfa, case)
    out = []
    for side in range(2):
        tr = ser.give(host.Tracker(ctx, n))
        kf, rep = host.KeyFrame(ctx), host.FrameReport(ctx, n)
        state = tr.track_state(case["pose_in"])
        opts = tr.opts(max_patches=budget)
        if side == 0:
            res, infos, rinfos, rc = host.Tracker.track_frames_report_batch([tr], [kf], [d_frame], [state], opts=opts, reports=[rep], tags=[9],
                                                                            shuffle_seeds=[SEED])
            assert rc == 0 and rinfos[0]["report_in_chain"] == (0 if long_path else 1)
            drawn = tr.read_shuffle()
            assert all(np.array_equal(drawn[w], host.shuffle_order(hip, SEED, 0, w, n)) for w in (0, 1))
        else:
            tr.set_shuffle(*[host.shuffle_order(hip, SEED, 0, w, n) for w in (0, 1)])
            ctx.sync()      # (beyond 8192 points the orders go up asynchronously from the context's pinned block, which the batch call fills next)
            res, infos = host.Tracker.track_frames_recover_batch([tr], [kf], [d_frame], [state], opts=opts)
            tr.report_frame(rep, 9)
        assert (res[0]["n_meas"] > GS_LIMIT) == long_path and res[0]["n_meas"] > 500   # the list the fused kernel cannot hold
        out.append((res.tobytes(), bytes(state), tr.iteration_set().tobytes(), rep.info(), rep.read().tobytes()))
        if side == 0:
            assert dict(rep.info(), report_in_chain=0 if long_path else 1, report_too_small=0) == rinfos[0] and rep.info()["n_records"] > 500
        for o in (rep, kf, tr):
            o.close()
    assert out[0] == out[1]
    assert (n > 8192) == (tile > 1)
    d_frame.free()
    ser.close()
    for o in (kfa, kfb):
        o.close()
    ctx.close()


# ---- 5. refusals (last: only the chain's side sees these frames) ----------------------------------------------------------------------
def test_refusals_leave_states_and_reports(sides, hip):
    X, _ = sides
    A, C2 = X[0], X[2]
    for c in (A, C2):
        c.state = c.tr.track_state(c.poses[0])
    chain([A, C2], [0, 0])
    plain = RecCamera(hip, estimator=False)                                  # its map was set by hand: no serials
    rep_plain = host.FrameReport(plain.ctx, 2000)
    plain.report, plain.n = rep_plain, len(plain.map["world"])
    before = [(bytes(c.state), c.report.info(), c.report.read().tobytes(), c.tr.iteration_set().tobytes()) for c in (A, C2)]
    plain_state = bytes(plain.state)
    assert chain([A, C2], [1, 1], reports=[A.report, A.report], check=False) == E_ARG      # a report named twice
    assert chain([A, plain], [1, 1], check=False) == E_STATE                                 # a tracker without serials
    assert hip.track_frames_report_batch(0, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None) == E_ARG
    assert [(bytes(c.state), c.report.info(), c.report.read().tobytes(), c.tr.iteration_set().tobytes()) for c in (A, C2)] == before
    assert bytes(plain.state) == plain_state and rep_plain.info() == EMPTY
    # without a report the tracker's map may come from anywhere
    res, infos, rinfos, rc = chain([A, plain], [1, 1], reports=[A.report, None])
    assert rc == 0 and rinfos[1] == dict(EMPTY, report_in_chain=0, report_too_small=0) and rinfos[0]["n_records"] > 100 and res[1]["n_meas"] > 100
    rep_plain.close()
    plain.close()
