"""Reference for the map-table edits ptam_map_apply_outliers / ptam_map_handle_bad_points / ptam_map_add_points, twice:
  * a literal restatement with Python objects — one dict of measurements per keyframe keyed by the point object, the two sets
    sMeasurementKFs / sNeverRetryKFs per point, the lists vpPoints / mqNewQueue / mvFailureQueue — that follows the outlier loop
    of MapMaker::BundleAdjust (src/MapMaker.cc:916-932), HandleBadPoints (:131-153) with Map::MoveBadPointsToTrash
    (src/Map.cc:20-30) and the table side of AddPointEpipolar (:670-685) statement by statement, with converters from and to
    the tables (index order stands in for pointer order, as in the device calls);
  * a vectorised numpy version of each entry for the larger sizes, returning the dicts of the host.map_* calls.
And the seeded tables the tests run on."""
import numpy as np

from ptam_cg_amd import _abi, host
from tests import map_ba_ref

MEAS_DT, PAIR_DT, OUTLIER_DT = host.MAP_MEAS_DT, host.MAP_PAIR_DT, host.MAP_OUTLIER_DT
POINT_DT, SOURCE_DT, MADE_DT = host.MAP_REFIND_POINT_DT, host.MAP_POINT_SOURCE_DT, host.NEW_MAP_POINT_DT
OUTLIER_COUNTS = ("n_point_bad", "n_failure_added", "n_never_added", "n_meas_out", "n_never_out", "n_failure_out")
BAD_COUNTS = ("n_marked", "n_removed", "n_kept", "n_meas_out", "n_never_out", "n_new_out", "n_new_dropped", "n_failure_out")


# ---- the literal restatement ------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self):
        self.bBad = False
        self.nMEstimatorOutlierCount = self.nMEstimatorInlierCount = 0
        self.sMeasurementKFs, self.sNeverRetryKFs = set(), set()   # MapMakerData
        self.old_index = -1          # where the point sat in the table it came from (-1: made since)
        self.made = None             # the ptam_new_map_point record and the source keyframe of a point made since


class KeyFrame:
    def __init__(self):
        self.mMeasurements = {}      # MapPoint -> (nLevel, Source, (x, y))


class Map:
    def __init__(self):
        self.vpKeyFrames, self.vpPoints, self.vpPointsTrash = [], [], []
        self.mqNewQueue, self.mvFailureQueue = [], []


def map_from_tables(n_kf, n_points, meas, never, bad=None, outlier_count=None, inlier_count=None, new_queue=(), failure=()):
    m = Map()
    m.vpKeyFrames = [KeyFrame() for _ in range(n_kf)]
    m.vpPoints = [MapPoint() for _ in range(n_points)]
    for i, p in enumerate(m.vpPoints):
        p.old_index = i
        p.bBad = bool(bad[i]) if bad is not None else False
        if outlier_count is not None:
            p.nMEstimatorOutlierCount, p.nMEstimatorInlierCount = int(outlier_count[i]), int(inlier_count[i])
    for r in meas:
        k, p = m.vpKeyFrames[r["kf"]], m.vpPoints[r["point"]]
        k.mMeasurements[p] = (int(r["level"]), int(r["source"]), (float(r["root_pos"][0]), float(r["root_pos"][1])))
        p.sMeasurementKFs.add(k)
    for r in never:
        m.vpPoints[r["point"]].sNeverRetryKFs.add(m.vpKeyFrames[r["kf"]])
    m.mqNewQueue = [m.vpPoints[i] for i in new_queue]
    m.mvFailureQueue = [(m.vpKeyFrames[r["kf"]], m.vpPoints[r["point"]]) for r in failure]
    return m


def tables_from_map(m):
    """-> dict: the tables in index order.  A trashed point is in no table: a queue entry that names one is left out — the new
    queue's as ReFindNewlyMade pops and skips it (:1056-1059, counted in n_new_dropped), the failure queue's by the defined
    deviation of ptam_map_handle_bad_points."""
    kfi = {k: i for i, k in enumerate(m.vpKeyFrames)}
    pti = {p: i for i, p in enumerate(m.vpPoints)}
    rows = sorted((kfi[k], pti[p], v) for k in m.vpKeyFrames for p, v in k.mMeasurements.items())
    meas = np.zeros(len(rows), MEAS_DT)
    for i, (k, p, (lv, src, pos)) in enumerate(rows):
        meas[i] = (k, p, lv, src, pos)
    nv = sorted((kfi[k], pti[p]) for p in m.vpPoints for k in p.sNeverRetryKFs)
    never = np.array(nv, np.int32).reshape(-1, 2).copy().view(PAIR_DT).reshape(-1)
    nq = np.array([pti[p] for p in m.mqNewQueue if p in pti], np.int32)
    fq = np.array([(kfi[k], pti[p]) for k, p in m.mvFailureQueue if p in pti], np.int32).reshape(-1, 2).copy().view(PAIR_DT).reshape(-1)
    new_index = np.full(sum(1 for p in m.vpPoints + m.vpPointsTrash if p.old_index >= 0), -1, np.int32)
    for p, i in pti.items():
        if p.old_index >= 0:
            new_index[p.old_index] = i
    return dict(meas=meas, never=never, new_queue=nq, failure=fq, bad=np.array([p.bBad for p in m.vpPoints], np.uint8),
                new_index=new_index, kept=np.array([p.old_index for p in m.vpPoints], np.int32),
                n_new_dropped=sum(1 for p in m.mqNewQueue if p not in pti), n_failure_dropped=sum(1 for _, p in m.mvFailureQueue if p not in pti))


def literal_apply_outliers(m, outlier_pairs):
    """:916-932 for (point index, keyframe index) pairs in GetOutlierMeasurements order -> the action taken per pair"""
    actions = []
    for pi, ki in outlier_pairs:
        pp, pk = m.vpPoints[pi], m.vpKeyFrames[ki]
        meas = pk.mMeasurements[pp]
        if len(pp.sMeasurementKFs) <= 2 or meas[1] == _abi.SRC_ROOT:                   # :921
            pp.bBad = True
            actions.append(_abi.OUT_POINT_BAD)
        else:
            if meas[1] in (_abi.SRC_TRACKER, _abi.SRC_EPIPOLAR):                        # :925
                m.mvFailureQueue.append((pk, pp))
                actions.append(_abi.OUT_FAILURE_QUEUE)
            else:
                pp.sNeverRetryKFs.add(pk)                                               # :928
                actions.append(_abi.OUT_NEVER_RETRY)
            del pk.mMeasurements[pp]                                                    # :929
            pp.sMeasurementKFs.discard(pk)                                              # :930
    return actions


def literal_handle_bad_points(m):
    """:131-153 and src/Map.cc:20-30 -> how many points the counts marked that were not bad before"""
    n_marked = 0
    for p in m.vpPoints:                                                                # :134-138
        if p.nMEstimatorOutlierCount > 20 and p.nMEstimatorOutlierCount > p.nMEstimatorInlierCount:
            n_marked += not p.bBad
            p.bBad = True
    for p in m.vpPoints:                                                                # :142-151
        if p.bBad:
            for k in m.vpKeyFrames:
                if p in k.mMeasurements:
                    del k.mMeasurements[p]
    for i in range(len(m.vpPoints) - 1, -1, -1):                                        # Map.cc:23-29
        if m.vpPoints[i].bBad:
            m.vpPointsTrash.append(m.vpPoints[i])
            del m.vpPoints[i]
    return n_marked


def literal_add_points(m, src_kf, target_kf, made, target_source):
    """:670-685 (and :352-362 with SRC_TRAIL) per record of a device call's output"""
    kSrc, kTarget = m.vpKeyFrames[src_kf], m.vpKeyFrames[target_kf]
    for r in made:
        pNew = MapPoint()
        pNew.made = (r, src_kf)
        m.vpPoints.append(pNew)                                                         # :670
        m.mqNewQueue.append(pNew)                                                       # :671
        lv = int(r["level"])
        kSrc.mMeasurements[pNew] = (lv, _abi.SRC_ROOT, (float(r["src_root_pos"][0]), float(r["src_root_pos"][1])))      # :673-678
        kTarget.mMeasurements[pNew] = (lv, int(target_source), (float(r["target_pos"][0]), float(r["target_pos"][1])))  # :680-682
        pNew.sMeasurementKFs.add(kSrc)                                                  # :684-685
        pNew.sMeasurementKFs.add(kTarget)


def point_rows_of_made(m):
    """the point-side rows of the points made since the tables were read, in vpPoints order"""
    new = [p for p in m.vpPoints if p.made is not None]
    pts, src = np.zeros(len(new), POINT_DT), np.zeros(len(new), SOURCE_DT)
    for i, p in enumerate(new):
        r, k = p.made
        pts[i]["pv"], pts[i]["src_kf"], pts[i]["src_level"] = r["point"], k, r["level"]
        pts[i]["center_x"], pts[i]["center_y"] = r["center_x"], r["center_y"]
        src[i]["src_kf"] = k
        for f in ("center_nc", "one_right_nc", "one_down_nc"):
            src[i][f] = r[f]
    return pts, src


# ---- the vectorised version: the dicts of host.map_apply_outliers / map_handle_bad_points / map_add_points --------------------
def sort_pairs(t):
    return t[np.lexsort((t["point"], t["kf"]))]


def pairs_of(rows):
    q = np.zeros(len(rows), PAIR_DT)
    q["kf"], q["point"] = rows["kf"], rows["point"]
    return q


def np_apply_outliers(n_kf, bad, meas, never, failure, outliers):
    bad = np.array(bad, np.uint8)
    act = outliers["action"]
    bad[outliers["point"][act == _abi.OUT_POINT_BAD]] = 1
    erased = np.zeros(len(meas), bool)
    erased[outliers["meas"][act != _abi.OUT_POINT_BAD]] = True
    nf, nn = outliers[act == _abi.OUT_FAILURE_QUEUE], outliers[act == _abi.OUT_NEVER_RETRY]
    d = dict(bad=bad, meas=meas[~erased], never=sort_pairs(np.concatenate([never, pairs_of(nn)])),
             failure=np.concatenate([failure, pairs_of(nf)]))
    d.update(n_point_bad=int((act == _abi.OUT_POINT_BAD).sum()), n_failure_added=len(nf), n_never_added=len(nn),
             n_meas_out=len(d["meas"]), n_never_out=len(d["never"]), n_failure_out=len(d["failure"]))
    return d


def np_handle_bad_points(n_kf, n_points, meas, never, bad=None, outlier_count=None, inlier_count=None, new_queue=None, failure=None,
                         columns=()):
    flag = np.zeros(n_points, bool) if bad is None else np.asarray(bad) != 0
    marked = np.zeros(n_points, bool)
    if outlier_count is not None:
        oc, ic = np.asarray(outlier_count), np.asarray(inlier_count)
        marked = (oc > 20) & (oc > ic)
    removed = flag | marked
    kept = np.flatnonzero(~removed).astype(np.int32)
    new_index = np.full(n_points, -1, np.int32)
    new_index[kept] = np.arange(len(kept), dtype=np.int32)
    nq = np.zeros(0, np.int32) if new_queue is None else np.asarray(new_queue, np.int32)
    fq = np.zeros(0, PAIR_DT) if failure is None else np.asarray(failure, PAIR_DT)

    def remap(t):
        t = t[new_index[t["point"]] >= 0].copy()
        t["point"] = new_index[t["point"]]
        return t
    cols = []
    for c in columns:
        c = np.array(c, order="C")
        c[:len(kept)] = c[kept]
        cols.append(c)
    q = new_index[nq]
    d = dict(new_index=new_index, kept=kept, meas=remap(meas), never=remap(never), new_queue=q[q >= 0], failure=remap(fq), columns=cols)
    d.update(n_marked=int((marked & ~flag).sum()), n_removed=int(removed.sum()), n_kept=len(kept), n_meas_out=len(d["meas"]),
             n_never_out=len(d["never"]), n_new_out=len(d["new_queue"]), n_new_dropped=len(nq) - len(d["new_queue"]),
             n_failure_out=len(d["failure"]))
    return d


def np_add_points(n_kf, n_points, meas, src_kf, target_kf, made, target_source=_abi.SRC_EPIPOLAR):
    A = len(made)
    rows = np.zeros(2 * A, MEAS_DT)
    rows["kf"][:A], rows["kf"][A:] = src_kf, target_kf
    rows["point"][:A] = rows["point"][A:] = n_points + np.arange(A)
    rows["level"][:A] = rows["level"][A:] = made["level"]
    rows["source"][:A], rows["source"][A:] = _abi.SRC_ROOT, target_source
    rows["root_pos"][:A], rows["root_pos"][A:] = made["src_root_pos"], made["target_pos"]
    pts, src = np.zeros(A, POINT_DT), np.zeros(A, SOURCE_DT)
    pts["pv"], pts["src_kf"], pts["src_level"], pts["center_x"], pts["center_y"] = made["point"], src_kf, made["level"], made["center_x"], made["center_y"]
    src["src_kf"] = src_kf
    for f in ("center_nc", "one_right_nc", "one_down_nc"):
        src[f] = made[f]
    return dict(meas=sort_pairs(np.concatenate([meas, rows])), points=pts, sources=src,
                new_queue=np.arange(n_points, n_points + A, dtype=np.int32))


# ---- the rule the device calls enforce on their input tables -----------------------------------------------------------------
def tables_valid(n_kf, n_points, meas, never):
    def ordered(t):
        key = t["kf"].astype(np.int64) * (1 << 32) + t["point"].astype(np.int64)
        in_range = ((t["kf"] >= 0) & (t["kf"] < n_kf) & (t["point"] >= 0) & (t["point"] < n_points)).all()
        return bool(in_range and (np.diff(key) > 0).all())
    ok_meas = ((meas["level"] >= 0) & (meas["level"] < _abi.LEVELS) & (meas["source"] >= 0) & (meas["source"] <= _abi.SRC_EPIPOLAR)).all()
    both = set(zip(meas["kf"].tolist(), meas["point"].tolist())) & set(zip(never["kf"].tolist(), never["point"].tolist()))
    return ordered(meas) and ordered(never) and bool(ok_meas) and not both


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def make_tables(seed, n_kf, n_points, n_meas, n_never=None, n_new=None, n_failure=None, bad_share=0.03, count_share=0.03, lonely=3):
    """distinct (kf, point) pairs, sorted; sources and levels uniform; never pairs from the complement; a new queue without
    repeats (partly of bad points); a failure queue with duplicates (partly of bad points); bBad flags, tracker counts that mark
    further points.  lonely > 0: the last keyframe measures only `lonely` points, all of them bad — it loses every row."""
    rng = np.random.default_rng(seed)
    n_never = n_meas // 8 if n_never is None else n_never
    n_new = min(n_points, max(n_points // 10, 4)) if n_new is None else n_new
    n_failure = max(n_meas // 50, 8) if n_failure is None else n_failure
    kf_free = n_kf - 1 if lonely else n_kf
    cells = rng.choice(kf_free * n_points, size=n_meas + n_never, replace=False)
    mcell, ncell = np.sort(cells[:n_meas]), np.sort(cells[n_meas:])
    meas = np.zeros(n_meas, MEAS_DT)
    meas["kf"], meas["point"] = mcell // n_points, mcell % n_points
    bad = (rng.random(n_points) < bad_share).astype(np.uint8)
    if lonely:
        lone = np.sort(rng.choice(n_points, size=lonely, replace=False))
        bad[lone] = 1
        extra = np.zeros(lonely, MEAS_DT)
        extra["kf"], extra["point"] = n_kf - 1, lone
        meas = np.concatenate([meas, extra])
    meas["level"] = rng.integers(0, 4, len(meas))
    meas["source"] = rng.integers(0, 5, len(meas))
    meas["root_pos"] = rng.random((len(meas), 2)) * 600
    never = np.zeros(n_never, PAIR_DT)
    never["kf"], never["point"] = ncell // n_points, ncell % n_points
    marked = rng.random(n_points) < count_share
    oc = np.where(marked, rng.integers(21, 60, n_points), rng.integers(0, 21, n_points)).astype(np.int32)
    ic = np.where(marked, rng.integers(0, 21, n_points), rng.integers(0, 60, n_points)).astype(np.int32)
    new_queue = rng.choice(n_points, size=n_new, replace=False).astype(np.int32)
    failure = np.zeros(n_failure, PAIR_DT)
    failure["kf"], failure["point"] = rng.integers(0, n_kf, n_failure), rng.integers(0, n_points, n_failure)
    if n_failure >= 4:
        failure[-2:] = failure[:2]
    return dict(n_kf=n_kf, n_points=n_points, meas=meas, never=never, bad=bad, outlier_count=oc, inlier_count=ic, new_queue=new_queue,
                failure=failure)


def make_outliers(seed, n_kf, n_points, meas, n_outliers):
    """a random subset of the rows in random order, routed by tests/map_ba_ref.route: the actions are the reference's routing"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(len(meas), size=min(n_outliers, len(meas)), replace=False)
    pairs = [(int(meas["point"][r]), int(meas["kf"][r])) for r in rows]
    return map_ba_ref.route(meas, np.arange(n_kf), np.arange(n_points), pairs, n_points).astype(OUTLIER_DT)


def make_made(seed, n_made):
    """ptam_new_map_point records as ptam_add_map_points_epipolar returns them, with seeded content"""
    rng = np.random.default_rng(seed)
    made = np.zeros(n_made, MADE_DT)
    for f in ("world", "pixel_right_w", "pixel_down_w"):
        made["point"][f] = rng.standard_normal((n_made, 3))
    for f in ("center_nc", "one_right_nc", "one_down_nc"):
        made[f] = rng.standard_normal((n_made, 3))
    made["src_root_pos"], made["target_pos"] = rng.random((n_made, 2)) * 600, rng.random((n_made, 2)) * 600
    made["level"] = rng.integers(0, 4, n_made)
    made["center_x"], made["center_y"] = rng.integers(0, 640, n_made), rng.integers(0, 480, n_made)
    made["candidate"], made["target_corner"], made["best_zmssd"] = rng.integers(0, 999, n_made), rng.integers(0, 999, n_made), rng.integers(0, 9999, n_made)
    return made


def point_columns(seed, n_points):
    """point-side tables as a caller keeps them: points3, the re-find point table, the point sources"""
    rng = np.random.default_rng(seed)
    pts = np.zeros(n_points, POINT_DT)
    pts["pv"]["world"] = rng.standard_normal((n_points, 3))
    pts["src_kf"], pts["center_x"] = rng.integers(0, 4, n_points), np.arange(n_points)
    src = np.zeros(n_points, SOURCE_DT)
    src["center_nc"] = rng.standard_normal((n_points, 3))
    return [rng.standard_normal((n_points, 3)), pts, src]


def gpu_case():
    """the tables of tests/test_gpu_map_edit.py's comparison against the vectorised reference"""
    t = make_tables(42, 7, 2500, 9000)
    t["outliers"] = make_outliers(43, 7, 2500, t["meas"], 400)
    return t


def assert_every_class(t):
    """-> the two reference results; every class of entry 1 and entry 2 is non-empty on these inputs"""
    a = np_apply_outliers(t["n_kf"], t["bad"], t["meas"], t["never"], t["failure"], t["outliers"])
    assert a["n_point_bad"] > 0 and a["n_failure_added"] > 0 and a["n_never_added"] > 0
    b = np_handle_bad_points(t["n_kf"], t["n_points"], t["meas"], t["never"], t["bad"], t["outlier_count"], t["inlier_count"],
                               t["new_queue"], t["failure"])
    by_count = (t["outlier_count"] > 20) & (t["outlier_count"] > t["inlier_count"])
    assert b["n_marked"] > 0 and ((t["bad"] != 0) & ~by_count).any()
    assert b["n_new_dropped"] > 0 and b["n_failure_out"] < len(t["failure"])
    had, has = np.bincount(t["meas"]["kf"], minlength=t["n_kf"]), np.bincount(b["meas"]["kf"], minlength=t["n_kf"])
    assert ((had > 0) & (has == 0)).any()
    return a, b


def assert_same(a, b, counts, arrays):
    for f in counts:
        assert a[f] == b[f], (f, a[f], b[f])
    for f in arrays:
        assert a[f].dtype == b[f].dtype and a[f].tobytes() == b[f].tobytes(), f
