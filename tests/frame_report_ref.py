"""The frame report in numpy and in objects: what ptam_tracker_report_frames / ptam_frame_report_from_host write, and what
ptam_rmap_note_reports / ptam_rmap_insert_keyframe_report make of it.

The numpy form follows the device: a mark per point (the last found slot that names it), the marked points walked in index order.
The object form follows the reference: TrackMap builds mCurrentKF.mMeasurements, a map from MapPoint* to Measurement, in the order
of vIterationSet (src/Tracker.cc:667-676: `mMeasurements[&p] = m`, so a later entry replaces an earlier one); CalcPoseUpdate bumps
the found points' counts (:989-997); AddKeyFrameFromTopOfQueue stamps the measurements into the points that still exist
(src/MapMaker.cc:501-506).  Walked in the map's point order, the object form gives the numpy form's rows."""
import numpy as np

MEAS_DT = np.dtype([("point", "<i4"), ("level", "<i4"), ("found", "<i4"), ("did_subpix", "<i4"), ("outlier", "<i4"), ("pad_", "<i4"),
                    ("v2_found", "<f8", (2,))])                     # ptam_trackmap_meas
RECORD_DT = np.dtype([("serial", "<i8"), ("level", "<i4"), ("outlier", "u1"), ("did_subpix", "u1"), ("pad_", "u1", (2,)),
                      ("root_pos", "<f8", (2,))])                   # ptam_frame_record
KF_ROW_DT = np.dtype([("point", "<i4"), ("level", "<i4"), ("root_pos", "<f8", (2,))])      # ptam_map_kf_row
assert MEAS_DT.itemsize == 40 and RECORD_DT.itemsize == 32 and KF_ROW_DT.itemsize == 24


# ---- the numpy form -------------------------------------------------------------------------------------------------------------------
def report(point_serials, entries):
    """-> (records RECORD_DT sorted by serial, dict(n_records, n_entries, n_outliers))"""
    ser = np.asarray(point_serials, np.int64)
    entries = np.asarray(entries, MEAS_DT)
    mark = np.full(len(ser), -1, np.int64)
    slots = np.flatnonzero(entries["found"] != 0)
    np.maximum.at(mark, entries["point"][slots], slots)            # the later slot wins
    pts = np.flatnonzero(mark >= 0)
    e = entries[mark[pts]]
    rec = np.zeros(len(pts), RECORD_DT)
    rec["serial"], rec["level"] = ser[pts], e["level"]
    rec["outlier"], rec["did_subpix"] = e["outlier"] != 0, e["did_subpix"] != 0
    rec["root_pos"] = e["v2_found"]
    return rec, dict(n_records=len(rec), n_entries=len(entries), n_outliers=int(rec["outlier"].sum()))


def resolve(col, serials):
    """the index of each serial in the strictly increasing column, -1 where it is not there"""
    col, serials = np.asarray(col, np.int64), np.asarray(serials, np.int64)
    at = np.searchsorted(col, serials)
    hit = (at < len(col)) & (col[np.minimum(at, max(len(col) - 1, 0))] == serials) if len(col) else np.zeros(len(serials), bool)
    return np.where(hit, at, -1).astype(np.int32)


def note(col, counts, rec):
    """counts = (outlier_count, inlier_count) of the map whose serial column is col -> (the two columns after the report, n_gone)"""
    oc, ic = (np.array(c, np.int32) for c in counts)
    at = resolve(col, rec["serial"])
    live = at >= 0
    np.add.at(oc, at[live & (rec["outlier"] != 0)], 1)
    np.add.at(ic, at[live & (rec["outlier"] == 0)], 1)
    return (oc, ic), int((~live).sum())


def kf_rows(col, rec):
    """-> (the new keyframe's rows KF_ROW_DT, sorted by point; n_gone)"""
    at = resolve(col, rec["serial"])
    live = at >= 0
    rows = np.zeros(int(live.sum()), KF_ROW_DT)
    rows["point"], rows["level"], rows["root_pos"] = at[live], rec["level"][live], rec["root_pos"][live]
    return rows, int((~live).sum())


# ---- the object form ------------------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, serial):
        self.serial, self.outlier_count, self.inlier_count = int(serial), 0, 0


class Measurement:
    def __init__(self, e):
        self.level, self.outlier, self.did_subpix = int(e["level"]), bool(e["outlier"]), bool(e["did_subpix"])
        self.root_pos = (float(e["v2_found"][0]), float(e["v2_found"][1]))


def object_measurements(points, entries):
    """mCurrentKF.mMeasurements: a dict from the tracker's MapPoint to its Measurement, filled in iteration-set order"""
    meas = {}
    for e in np.asarray(entries, MEAS_DT):
        if e["found"]:
            meas[points[int(e["point"])]] = Measurement(e)
    return meas


def object_report(points, entries):
    """the dict walked in the tracker's point order -> records"""
    meas = object_measurements(points, entries)
    out = []
    for p in points:
        if p in meas:
            m = meas[p]
            out.append((p.serial, m.level, m.outlier, m.did_subpix, (0, 0), m.root_pos))
    return np.array(out, RECORD_DT) if out else np.zeros(0, RECORD_DT)


def object_note(map_points, meas):
    """CalcPoseUpdate's bumps on the points that are still the map's (a trashed point's counts are nobody's) -> n_gone"""
    alive = set(map_points)
    gone = 0
    for p, m in meas.items():
        if p not in alive:
            gone += 1
        elif m.outlier:
            p.outlier_count += 1
        else:
            p.inlier_count += 1
    return gone


def object_kf_rows(map_points, meas):
    """the measurements of the points that are still the map's, in the map's point order -> rows"""
    out = [(i, meas[p].level, meas[p].root_pos) for i, p in enumerate(map_points) if p in meas]
    return np.array(out, KF_ROW_DT) if out else np.zeros(0, KF_ROW_DT)
