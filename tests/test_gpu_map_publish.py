"""-m gpu: the resident map published to the tracker on the device — the serial column of ptam_rmap, ptam_rmap_publish into a
ptam_map_snapshot, ptam_tracker_take_map, ptam_rmap_resolve_serials — against tests/map_publish_ref.py (the numpy form) and against
the composed host path the calls replace: ptam_rmap_download of the point rows, prev_index composed from `kept` and the appends,
ptam_tracker_update_map.  Serials, indices and counts by ==; tracked frames, iteration sets and tables by tobytes().
The scene is the one of tests/test_gpu_insert_keyframe.py (tests/insert_keyframe_ref.py: 3 keyframes, about 600 points)."""
import threading

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import insert_keyframe_ref as I
from tests import map_edit_ref as E
from tests import map_publish_ref as P
from tests.test_gpu_map_edit import PATTERNS, removed_pattern
from tests.test_gpu_resident_map import UPLOAD_KEYS, same_tables

pytestmark = pytest.mark.gpu
E_ARG = -1
KF_RECORD = 64                       # what ptam_rmap_publish sends up per keyframe (ptam_hip.h); the bound is RMAP_KF_RECORD_BYTES
TRACKER_CAP = 4096


# ---- synthetic maps: K keyframes that all are one small image, N points, one row per point ---------------------------------------
@pytest.fixture(scope="module")
def ctx(hip):
    c = host.Context(lib=hip)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_kf(ctx):
    kf = host.KeyFrame(ctx).MakeKeyFrame_Lite(I.views()["ia"])
    yield kf
    kf.close()


def synthetic(n, bad=None, K=4, seed=3):
    """whole-map tables of n points: the redundant columns agree, every point is measured once in keyframe i % K"""
    rng = np.random.default_rng(seed + n)
    _, pts, src = E.point_columns(seed, n)
    pts["src_kf"] = rng.integers(0, K, n)
    pts["src_level"] = rng.integers(0, 4, n)
    bad = np.zeros(n, np.uint8) if bad is None else np.asarray(bad, np.uint8)
    pts["bad"], src["src_kf"] = bad, pts["src_kf"]
    pt = np.arange(n, dtype=np.int32)
    order = np.lexsort((pt, pt % K))
    meas = np.zeros(n, E.MEAS_DT)
    meas["kf"], meas["point"], meas["level"] = (pt % K)[order], pt[order], rng.integers(0, 4, n)
    poses = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (K, 1))
    poses[:, 9] = 0.01 * np.arange(K)
    return dict(poses=poses, fixed=(np.arange(K) == 0).astype(np.uint8), points3=np.ascontiguousarray(pts["pv"]["world"]), points=pts, sources=src,
                bad=bad, meas=meas, never=np.zeros(0, E.PAIR_DT), new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT),
                outlier_count=np.zeros(n, np.int32), inlier_count=np.zeros(n, np.int32))


def uploaded(ctx, h, kfs=None, **reserve):
    m = host.ResidentMap(ctx)
    if reserve:
        m.reserve(**reserve)
    m.upload(kfs=kfs, **{k: h[k] for k in UPLOAD_KEYS})
    return m


def made_like(h, seed, n):
    """n new-point records that repeat seeded points of the scene (source keyframe I.THIRD): points a tracker can search"""
    pick = np.random.default_rng(seed).integers(0, len(h["points"]), n)
    made = E.make_made(seed, n)
    made["point"], made["level"] = h["points"]["pv"][pick], h["points"]["src_level"][pick]
    made["center_x"], made["center_y"] = h["points"]["center_x"][pick], h["points"]["center_y"][pick]
    return made


def moved(m, call):
    """-> (what the call returned, bytes up, bytes down)"""
    up0, down0 = m.traffic()
    r = call()
    up, down = m.traffic()
    return r, up - up0, down - down0


# ---- 1. the serial column -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_serial_column_follows_every_edit(ctx, n, pattern):
    """upload, handle_bad_points, add_points with growth from capacity count + 1, a refused upload, a re-upload: the column equals
    the numpy form after each, and the existing calls move what they moved before the column existed"""
    h = synthetic(n, bad=removed_pattern(n, pattern))
    ref = P.NpMap()
    m = host.ResidentMap(ctx)
    m.reserve(n_points=n + 1)
    _, up, down = moved(m, lambda: m.upload(**{k: h[k] for k in UPLOAD_KEYS}))
    assert (up, down) == (sum(h[k].nbytes for k in UPLOAD_KEYS), _abi.RMAP_WORD_BYTES)
    ref.upload(n)
    assert np.array_equal(m.point_serials(), ref.serials)
    _, up, down = moved(m, lambda: m.point_serials(n // 2, n - n // 2))
    assert (up, down) == (0, 8 * (n - n // 2))
    # HandleBadPoints: one more compacted column
    r, up, down = moved(m, lambda: m.handle_bad_points())
    assert (up, down) == (0, _abi.RMAP_WORD_BYTES)
    ref.remove(h["bad"] == 0)
    nk = r["n_kept"]
    assert nk == len(ref.serials) and np.array_equal(m.point_serials(), ref.serials)
    # a refused call leaves it: a re-upload whose measurement table is out of order
    if n >= 2:
        broken = h["meas"].copy()
        broken[[0, 1]] = broken[[1, 0]]
        assert m.upload(check=False, **dict({k: h[k] for k in UPLOAD_KEYS}, meas=broken)) == E_ARG
        assert np.array_equal(m.point_serials(), ref.serials)
    # AddPoints: with nothing removed the point tables hold the count + 1 (or the least capacity, 64) and grow, the column with them
    made = E.make_made(n, 70)
    _, up, down = moved(m, lambda: m.add_points(1, 0, made))
    assert (up, down) == (made.nbytes, 0)
    ref.append(len(made))
    got = m.point_serials()
    assert np.array_equal(got, ref.serials) and np.all(np.diff(got) > 0)
    assert m.lib.rmap_point_serials(m.h, 1, len(got), None) == E_ARG
    # a re-uploaded map is a new map: fresh serials, none of them seen before
    m.upload(**{k: h[k] for k in UPLOAD_KEYS})
    ref.upload(n)
    assert np.array_equal(m.point_serials(), ref.serials) and m.point_serials().min() > got.max()
    m.close()


# ---- 2. prev at the edges: synthetic serial lists through publish and take -----------------------------------------------------------
APPEND_TO = {0: 1, 1: 64, 64: 65, 65: 1025, 1025: 1026}


@pytest.mark.parametrize("edit", ["all_kept", "none_kept", "first_removed", "last_removed", "appended"])
@pytest.mark.parametrize("n_old", [0, 1, 64, 65, 1025])
def test_prev_at_the_edges(ctx, one_kf, n_old, edit):
    bad = np.zeros(n_old, np.uint8)
    if edit == "none_kept":
        bad[:] = 1
    elif edit == "first_removed":
        bad[:1] = 1
    elif edit == "last_removed":
        bad[-1:] = 1
    m = uploaded(ctx, synthetic(n_old, bad=bad), kfs=[one_kf] * 4)
    snap = host.MapSnapshot(ctx, 64)                    # (too small for 1 025 points: the publish grows its slot)
    tr = host.Tracker(ctx, 2048)
    ref_m, ref_s, ref_t = P.NpMap(), P.NpSnapshot(), P.NpTracker()
    ref_m.upload(n_old)
    pub = m.publish(snap)
    ref_s.publish(ref_m)
    assert pub["generation"] == 1 and pub["n_points"] == n_old and pub["grew"] == int(n_old > 64)
    got, want = tr.take_map(snap), ref_t.take(ref_s)
    assert got["changed"] == 1 and all(got[f] == want[f] for f in ("generation", "n_points", "n_carried", "n_new", "n_dropped"))
    assert got["n_carried"] == 0 and got["n_new"] == n_old and np.array_equal(tr.point_serials(), ref_t.serials)
    # the edit, a second generation, the take
    m.handle_bad_points()
    ref_m.remove(bad == 0)
    if edit == "appended":
        made = E.make_made(5, APPEND_TO[n_old] - n_old)
        m.add_points(1, 0, made)
        ref_m.append(len(made))
    pub = m.publish(snap)
    ref_s.publish(ref_m)
    assert pub["generation"] == 2 and pub["n_points"] == len(ref_m.serials)
    got, want = tr.take_map(snap), ref_t.take(ref_s)
    for f in ("changed", "generation", "n_points", "n_carried", "n_new", "n_dropped"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert got["link_bytes"] <= 64
    assert np.array_equal(tr.point_serials(), ref_t.serials) and np.array_equal(tr.point_serials(), m.point_serials())
    assert got["n_carried"] == {"none_kept": 0, "first_removed": max(n_old - 1, 0), "last_removed": max(n_old - 1, 0)}.get(edit, n_old)
    # the poll: nothing published since
    again = tr.take_map(snap)
    assert again["changed"] == 0 and again["link_bytes"] == 0 and again["generation"] == 2 and again["n_points"] == len(ref_m.serials)
    assert tr.lib.tracker_point_serials(tr.h, 0, len(ref_m.serials) + 1, None) == E_ARG
    for x in (tr, snap, m):
        x.close()


# ---- 3. resolve -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65, 1025])
def test_resolve_serials_against_the_numpy_form(ctx, n):
    N = 1500
    bad = (np.random.default_rng(4).random(N) < 0.3).astype(np.uint8)
    m = uploaded(ctx, synthetic(N, bad=bad))
    before = m.point_serials()
    m.handle_bad_points()
    m.add_points(1, 0, E.make_made(6, 40))
    col = m.point_serials()
    rng = np.random.default_rng(n)
    pool = np.concatenate([before, col[-40:], np.array([0, -3, col.max() + 1, col.max() + 1000, 2 ** 40], np.int64)])    # live, removed, never given
    ask = rng.choice(pool, size=n, replace=True) if n else np.zeros(0, np.int64)
    (idx, gone), up, down = moved(m, lambda: m.resolve_serials(ask))
    want = P.resolve(col, ask)
    assert np.array_equal(idx, want) and gone == int((want < 0).sum())
    assert (up, down) == ((8 * n, 4 * n + _abi.RMAP_WORD_BYTES) if n else (0, 0))
    if n >= 65:
        assert (want < 0).any() and (want >= 0).any()
    m.close()


# ---- the scene: two trackers in one context, A through snapshots, B through the composed host path ----------------------------------------
@pytest.fixture(scope="module")
def dev(hip):
    """tests/test_gpu_insert_keyframe.py's scene, made with the product's own calls; read-only"""
    c = host.Context(lib=hip)
    kfs, ka, poses, sp = I.make_keyframes(c)
    m = uploaded(c, I.empty_tables(poses), kfs)
    made, _ = host.MapMaker(c).AddSomeMapPoints(kfs[I.THIRD], poses[I.THIRD], kfs[I.TARGET], poses[I.TARGET],
                                                host.MapMaker(c).opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH))
    m.add_points(I.THIRD, I.TARGET, made)
    h = m.tables()
    m.close()
    assert len(h["points3"]) > 300
    for a in h.values():
        a.setflags(write=False)
    yield dict(ctx=c, kfs=kfs, ka=ka, sp=sp, h=h)
    c.close()


class Pair:
    """the resident map, a snapshot, tracker A (take_map) and tracker B (download + composed prev_index + update_map)"""

    def __init__(self, d, h=None):
        self.d, self.ctx = d, d["ctx"]
        self.kfs = list(d["kfs"])
        self.m = uploaded(self.ctx, d["h"] if h is None else h, self.kfs)
        self.snap = host.MapSnapshot(self.ctx, TRACKER_CAP)
        self.a, self.b = host.Tracker(self.ctx, TRACKER_CAP), host.Tracker(self.ctx, TRACKER_CAP)
        self.rf = host.ReFinder(self.ctx)
        self.labels = np.arange(self.m.counts()["n_points"])     # one label per point of the map, carried through the edits
        self.next_label = len(self.labels)
        self.ref = P.NpMap()                                     # the serial column in its numpy form, through the same edits
        self.ref.upload(len(self.labels))
        self.b_labels = np.zeros(0, np.int64)                    # ... and of the map B was handed last
        self.frames = 0

    # -- the mapmaker's edits, each mirrored in the labels (the host's composition of `kept` lists and appends)
    def handle_bad_points(self, share=0.12, seed=1):
        n = self.m.counts()["n_points"]
        sel = np.flatnonzero(np.random.default_rng(seed).random(n) < share).astype(np.int32)
        self.m.note_tracked(np.repeat(sel, 21), np.ones(21 * len(sel), np.uint8))       # outlier count 21 > 20 and > inlier count
        r = self.m.handle_bad_points(kept=True, new_index=True)
        assert r["n_removed"] == len(sel) > 0
        self.labels = self.labels[r["kept"]]
        self.ref.serials = self.ref.serials[r["kept"]]
        return r

    def insert_keyframe(self):
        t = self.m.tables()
        rows = I.tracker_rows(t, self.d["sp"])
        o = self.m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH)
        r = self.m.InsertKeyFrame(self.rf, self.d["ka"], self.d["sp"], 0, rows, o)
        self.kfs.append(self.d["ka"])
        assert r["n_made"] > 0
        self.labels = np.concatenate([self.labels, np.arange(self.next_label, self.next_label + r["n_made"])])
        self.next_label += r["n_made"]
        self.ref.append(r["n_made"])
        assert np.array_equal(self.m.point_serials(), self.ref.serials)          # InsertKeyFrame appends the next serials
        return r

    def bundle(self):
        r = self.m.bundle_adjust(_abi.MAP_BA_ALL)
        print("bundle:", {k: v for k, v in r.items() if not isinstance(v, np.ndarray)})
        return r

    # -- the hand-over, both ways
    def publish(self):
        assert np.array_equal(self.m.point_serials(), self.ref.serials)
        r, up, down = moved(self.m, lambda: self.m.publish(self.snap))
        K = self.m.counts()["n_kf"]
        assert up == KF_RECORD * K <= _abi.RMAP_KF_RECORD_BYTES * K and down <= _abi.RMAP_WORD_BYTES
        return r

    def take(self):
        """A takes the snapshot; B is handed the same map through the host -> A's result"""
        r = self.a.take_map(self.snap)
        assert r["link_bytes"] <= 64
        pts = self.m.download("points")
        where = {int(l): i for i, l in enumerate(self.b_labels)}
        prev = np.array([where.get(int(l), -1) for l in self.labels], np.int32)
        self.b.update_map(pts["pv"]["world"], pts["pv"]["pixel_right_w"], pts["pv"]["pixel_down_w"], [self.kfs[k] for k in pts["src_kf"]],
                          pts["src_level"], np.stack([pts["center_x"], pts["center_y"]], axis=1), prev)
        self.b_labels = self.labels.copy()
        if r["changed"]:
            assert (r["n_points"], r["n_carried"]) == (len(pts), int((prev >= 0).sum()))
            assert np.array_equal(self.a.point_serials(), self.m.point_serials())
        return r

    def frame(self):
        """one tracked frame on both trackers with the same shuffles -> (A's result, A's iteration set); B's are the same bits"""
        n = self.a.n
        assert n == self.b.n
        rng = np.random.default_rng(100 + self.frames)
        self.frames += 1
        sl, sf = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
        out = []
        for tr in (self.a, self.b):
            tr.set_shuffle(sl, sf)
            res = tr.TrackMap(self.d["ka"], self.d["sp"], tr.opts()).copy()
            out.append((res, tr.iteration_set()))
        (ra, ia), (rb, ib) = out
        assert ra.tobytes() == rb.tobytes(), [(f, ra[f], rb[f]) for f in ra.dtype.names if np.asarray(ra[f]).tobytes() != np.asarray(rb[f]).tobytes()]
        assert ia.tobytes() == ib.tobytes() and ra["n_meas"] > 20
        return ra, ia

    def close(self):
        for x in (self.a, self.b, self.snap, self.rf, self.m):
            x.close()


def test_take_equals_the_composed_host_path_frame_by_frame(dev):
    p = Pair(dev)
    assert p.publish()["generation"] == 1
    first = p.take()
    n0 = len(dev["h"]["points3"])
    assert first["changed"] == 1 and first["n_new"] == n0 and first["n_carried"] == 0
    r1, _ = p.frame()
    r2, it2 = p.frame()
    assert r1["templates_reused"] == 0 and r2["templates_reused"] > 0.8 * len(it2)    # the same prediction: the finders keep their templates
    # nothing was published: the poll, and the next frame is still B's
    idle = p.a.take_map(p.snap)
    assert idle["changed"] == 0 and idle["link_bytes"] == 0 and idle["generation"] == 1
    # the iteration set in the tracker's numbering, and its serials for the way back
    ser = p.a.iteration_serials()
    assert len(ser) == len(it2) and np.array_equal(ser, p.m.point_serials()[it2["point"]])
    hb = p.handle_bad_points()
    idx, gone = p.m.resolve_serials(ser)
    want = hb["new_index"][it2["point"]]
    assert np.array_equal(idx, want) and gone == int((want < 0).sum()) and 0 < gone < len(ser)
    # sorted by serial, the found entries are the rows of InsertKeyFrame sorted by point
    live = np.sort(ser[idx >= 0])
    rows_idx, _ = p.m.resolve_serials(live)
    assert np.all(np.diff(rows_idx) > 0)
    ins = p.insert_keyframe()
    ba = p.bundle()
    assert ba["accepted"] > 0
    assert p.publish()["generation"] == 2
    t = p.take()
    assert t["changed"] == 1 and t["generation"] == 2 and t["n_dropped"] == hb["n_removed"] and t["n_new"] == ins["n_made"]
    assert t["n_carried"] == n0 - hb["n_removed"]
    r3, it3 = p.frame()
    assert 0 < r3["templates_reused"] < len(it3)                                      # the carry happened, and the new points are searched
    # ptam_tracker_set_map clears the serial list: the next take of the same generation treats every point as new
    pts = p.m.download("points")
    p.a.set_map(pts["pv"]["world"], pts["pv"]["pixel_right_w"], pts["pv"]["pixel_down_w"], [p.kfs[k] for k in pts["src_kf"]], pts["src_level"],
                np.stack([pts["center_x"], pts["center_y"]], axis=1))
    assert len(p.a.point_serials()) == 0
    again = p.a.take_map(p.snap)
    assert again["changed"] == 1 and again["n_carried"] == 0 and again["n_new"] == len(pts) and again["n_dropped"] == len(pts)
    # a second ptam_rmap holding the same tables is another map
    m2 = uploaded(p.ctx, p.m.tables(), p.kfs)
    assert m2.publish(p.snap)["generation"] == 3
    other = p.a.take_map(p.snap)
    assert other["changed"] == 1 and other["n_carried"] == 0 and other["map_id"] != again["map_id"]
    assert np.array_equal(p.a.point_serials(), m2.point_serials())
    m2.close()
    p.close()


def test_two_publishes_with_edits_between_them_before_one_take(dev):
    p = Pair(dev)
    p.publish()
    p.take()
    p.frame()
    hb = p.handle_bad_points(seed=2)
    assert p.publish()["generation"] == 2
    ins = p.insert_keyframe()
    assert p.publish()["generation"] == 3
    t = p.take()                                                                      # the tracker never saw generation 2
    assert t["generation"] == 3 and t["n_dropped"] == hb["n_removed"] and t["n_new"] == ins["n_made"]
    r, it = p.frame()
    assert 0 < r["templates_reused"] < len(it)
    p.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_tracker_snapshot_and_map_as_they_were(dev, hip):
    p = Pair(dev)
    p.publish()
    p.take()
    p.frame()
    before = p.m.tables()
    small = host.Tracker(p.ctx, 100)                                                  # fewer points than the snapshot holds
    assert small.take_map(p.snap, check=False) == E_ARG and small.n == 0
    empty = host.MapSnapshot(p.ctx, 16)                                               # never published into
    assert p.a.take_map(empty, check=False) == E_ARG
    other = host.Context(lib=hip, size=(320, 240))                                    # a snapshot of another frame size
    half = host.MapSnapshot(other, TRACKER_CAP)
    p.m.publish(half)
    assert p.a.take_map(half, check=False) == E_ARG
    bare = uploaded(p.ctx, dev["h"], None)                                            # a map whose keyframes have no handles
    assert bare.publish(p.snap, check=False) == E_ARG
    assert p.snap.info() == dict(generation=1, map_id=p.a.take_map(p.snap)["map_id"], n_points=len(dev["h"]["points3"]))
    assert p.a.take_map(p.snap)["changed"] == 0
    same_tables(p.m.tables(), before)
    p.frame()                                                                         # A's next frame is B's, which saw none of this
    for x in (small, empty, half, bare, other):
        x.close()
    p.close()


# ---- 6. traffic does not grow with the map -----------------------------------------------------------------------------------------------
def test_traffic_is_the_same_with_twenty_thousand_more_points(dev):
    h = {k: np.array(v) for k, v in dev["h"].items()}
    extra = 20000
    rng = np.random.default_rng(8)
    pad = h["points"][rng.integers(0, len(h["points"]), extra)].copy()
    pad["pv"]["world"][:, 2] -= 1e3                                                   # out of every view
    big = dict(h, points=np.concatenate([h["points"], pad]), points3=np.concatenate([h["points3"], pad["pv"]["world"]]),
               sources=np.concatenate([h["sources"], h["sources"][:1].repeat(extra)]), bad=np.concatenate([h["bad"], np.zeros(extra, np.uint8)]),
               outlier_count=np.zeros(len(h["bad"]) + extra, np.int32), inlier_count=np.zeros(len(h["bad"]) + extra, np.int32))
    big["sources"]["src_kf"] = big["points"]["src_kf"]
    seen = []
    for tables in (h, big):
        m = uploaded(dev["ctx"], tables, dev["kfs"])
        snap, tr = host.MapSnapshot(dev["ctx"], 32768), host.Tracker(dev["ctx"], 32768)
        _, up, down = moved(m, lambda: m.publish(snap))
        t1 = tr.take_map(snap)
        m.handle_bad_points()
        _, up2, down2 = moved(m, lambda: m.publish(snap))
        t2 = tr.take_map(snap)
        assert t2["n_carried"] == len(tables["points3"]) and up <= _abi.RMAP_KF_RECORD_BYTES * 3 and down <= _abi.RMAP_WORD_BYTES
        assert t1["link_bytes"] <= 64 and t2["link_bytes"] <= 64
        seen.append((up, down, up2, down2, t1["link_bytes"], t2["link_bytes"]))
        for x in (tr, snap, m):
            x.close()
    assert seen[0] == seen[1]


# ---- 7. two threads -------------------------------------------------------------------------------------------------------------------------
def test_mapmaker_and_tracker_threads_hand_over_through_the_snapshot(dev, hip):
    """the pattern of tests/test_gpu_trackmap.test_tracker_and_mapmaker_threads_run_side_by_side: the mapmaker edits and publishes
    twenty times in its context while the tracker, in its own, polls, takes and tracks — every list the tracker took is the map's
    list of that generation"""
    ctx_t = host.Context(lib=hip)
    m = uploaded(dev["ctx"], dev["h"], dev["kfs"])
    snap = host.MapSnapshot(dev["ctx"], TRACKER_CAP)
    tr = host.Tracker(ctx_t, TRACKER_CAP)
    kf_cur = host.KeyFrame(ctx_t).MakeKeyFrame_Lite(I.views()["ia"])
    published, taken, errors, done = {}, [], [], threading.Event()

    def mapmaker():
        try:
            for r in range(20):
                n = m.counts()["n_points"]
                if r % 2:
                    sel = np.flatnonzero(np.random.default_rng(r).random(n) < 0.05).astype(np.int32)
                    m.note_tracked(np.repeat(sel, 21), np.ones(21 * len(sel), np.uint8))
                    m.handle_bad_points()
                else:
                    m.add_points(I.THIRD, I.TARGET, made_like(dev["h"], r, 11))
                ser = m.point_serials()
                published[m.publish(snap)["generation"]] = ser
        except Exception as e:      # noqa: BLE001 (reported by the main thread)
            errors.append(e)
        finally:
            done.set()

    def tracker():
        try:
            while True:
                last = done.is_set()
                t = tr.take_map(snap, check=False)
                if t != E_ARG:                  # (refused until the first publish)
                    if t["changed"]:
                        taken.append((t["generation"], tr.point_serials()))
                    tr.TrackMap(kf_cur, dev["sp"], tr.opts())
                if last:
                    return
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=mapmaker), threading.Thread(target=tracker)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not errors, errors
    final = tr.take_map(snap)                                                         # after the join: nothing is newer than generation 20
    assert final["generation"] == 20 and np.array_equal(tr.point_serials(), published[20])
    gens = [g for g, _ in taken]
    assert gens == sorted(set(gens)) and len(gens) >= 1 and gens[-1] == 20             # increasing; the tracker's last pass came after the last publish
    for g, ser in taken:
        assert np.array_equal(ser, published[g]), g
    assert snap.info()["generation"] == 20 and sorted(published) == list(range(1, 21))
    for x in (tr, kf_cur, snap, m, ctx_t):
        x.close()
