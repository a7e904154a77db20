"""CPU: the two forms of tests/frame_report_ref.py agree — the numpy form (marks and an index-order walk, what the device does) and
the object form (a dict from point object to measurement filled in iteration-set order, what the reference does) — on the cases
where they could part: nothing found, everything found, a point named twice, a map that has lost every point, serials the map
never gave out."""
import numpy as np
import pytest

from tests import frame_report_ref as F


def iteration_set(n_points, n_entries, found, seed, repeat=None):
    """n_entries entries over distinct points in a shuffled order; found: a share or a bool array; repeat: entries appended that
    name the points of the first `repeat` entries again, with other values"""
    rng = np.random.default_rng(seed)
    e = np.zeros(n_entries, F.MEAS_DT)
    e["point"] = rng.permutation(n_points)[:n_entries]
    e["level"] = rng.integers(0, 4, n_entries)
    e["found"] = (rng.random(n_entries) < found) if np.isscalar(found) else found
    e["did_subpix"] = rng.integers(0, 2, n_entries)
    e["outlier"] = rng.integers(0, 2, n_entries) * e["found"]
    e["v2_found"] = rng.random((n_entries, 2)) * 640
    if repeat:
        again = e[:repeat].copy()
        again["level"] = (again["level"] + 1) % 4
        again["found"], again["outlier"] = 1, 1 - again["outlier"]
        again["v2_found"] += 1.0
        e = np.concatenate([e, again])
    return e


def both_forms(serials, entries, map_col):
    """-> the numpy form's and the object form's (records, counts after a note, n_gone, keyframe rows) for a tracker whose points
    have `serials` and a map whose points, by now, have `map_col`"""
    points = [F.MapPoint(s) for s in serials]
    by_serial = {p.serial: p for p in points}
    map_points = [by_serial.get(int(s)) or F.MapPoint(s) for s in map_col]          # (a serial the tracker never saw: another object)
    rec, info = F.report(serials, entries)
    (oc, ic), gone = F.note(map_col, (np.zeros(len(map_col), np.int32), np.zeros(len(map_col), np.int32)), rec)
    rows, gone_rows = F.kf_rows(map_col, rec)
    meas = F.object_measurements(points, entries)
    o_rec = F.object_report(points, entries)
    o_gone = F.object_note(map_points, meas)
    o_rows = F.object_kf_rows(map_points, meas)
    o_oc = np.array([p.outlier_count for p in map_points], np.int32)
    o_ic = np.array([p.inlier_count for p in map_points], np.int32)
    assert gone == gone_rows and info["n_records"] == len(rec) and info["n_entries"] == len(entries)
    assert info["n_outliers"] == int(rec["outlier"].sum())
    return (rec, oc, ic, gone, rows), (o_rec, o_oc, o_ic, o_gone, o_rows)


def assert_same(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        else:
            assert x == y


SER = np.arange(1, 301, dtype=np.int64) * 3          # strictly increasing, with gaps


def test_none_found():
    a, b = both_forms(SER, iteration_set(300, 200, 0.0, 1), SER)
    assert_same(a, b)
    assert len(a[0]) == 0 and a[3] == 0 and len(a[4]) == 0 and not a[1].any() and not a[2].any()


def test_all_found():
    e = iteration_set(300, 300, 1.0, 2)
    a, b = both_forms(SER, e, SER)
    assert_same(a, b)
    rec = a[0]
    assert len(rec) == 300 and np.array_equal(rec["serial"], SER) and np.all(np.diff(rec["serial"]) > 0)
    assert np.array_equal(a[1] + a[2], np.ones(300, np.int32)) and np.array_equal(a[4]["point"], np.arange(300))
    # index order, not entry order
    back = np.empty(300, np.int64)
    back[e["point"]] = np.arange(300)
    assert np.array_equal(rec["level"], e["level"][back])


def test_a_repeated_point_the_later_entry_wins():
    e = iteration_set(300, 120, 1.0, 3, repeat=7)
    a, b = both_forms(SER, e, SER)
    assert_same(a, b)
    rec = a[0]
    assert len(rec) == 120 and len(np.unique(rec["serial"])) == 120
    for first, again in zip(e[:7], e[120:]):
        r = rec[rec["serial"] == SER[first["point"]]][0]
        assert r["level"] == again["level"] != first["level"] and tuple(r["root_pos"]) == tuple(again["v2_found"])
        assert r["outlier"] == again["outlier"]
    # a later entry that is NOT found does not replace a found one
    e2 = e.copy()
    e2["found"][120:] = 0
    a2, b2 = both_forms(SER, e2, SER)
    assert_same(a2, b2)
    assert a2[0].tobytes() == F.report(SER, e[:120])[0].tobytes()


def test_every_point_removed():
    e = iteration_set(300, 150, 0.7, 4)
    a, b = both_forms(SER, e, np.zeros(0, np.int64))
    assert_same(a, b)
    assert a[3] == len(a[0]) > 0 and len(a[4]) == 0
    # ... and a map that kept every third point, then grew
    col = np.concatenate([SER[::3], SER[-1] + 1 + np.arange(40)])
    a, b = both_forms(SER, e, col)
    assert_same(a, b)
    assert 0 < a[3] < len(a[0]) and np.all(np.diff(a[4]["point"]) > 0) and len(a[4]) == len(a[0]) - a[3]


def test_serials_never_given_out():
    """a report whose serials lie between, below and above the map's: nothing resolves, nothing is counted"""
    e = iteration_set(300, 300, 1.0, 5)
    odd = np.concatenate([[-5, 0], SER[:-2] + 1])      # none of them a multiple of 3 above 0 ... none is in SER
    assert not np.isin(odd, SER).any() and np.all(np.diff(odd) > 0)
    a, b = both_forms(odd, e, SER)
    assert_same(a, b)
    assert a[3] == 300 and not a[1].any() and not a[2].any() and len(a[4]) == 0
    assert np.array_equal(F.resolve(SER, np.array([SER[0] - 1, SER[-1] + 1, 2 ** 40], np.int64)), [-1, -1, -1])
    assert np.array_equal(F.resolve(np.zeros(0, np.int64), SER[:3]), [-1, -1, -1])


@pytest.mark.parametrize("seed", range(4))
def test_random_half_found_shuffled(seed):
    e = iteration_set(300, 260, 0.5, 10 + seed, repeat=seed)
    keep = np.random.default_rng(seed).random(300) < 0.8
    a, b = both_forms(SER, e, SER[keep])
    assert_same(a, b)


def test_the_dtypes_are_the_library_s():
    from ptam_cg_amd import host
    assert host.FRAME_RECORD_DT == F.RECORD_DT and host.TRACKMAP_MEAS_DT == F.MEAS_DT and host.MAP_KF_ROW_DT == F.KF_ROW_DT
