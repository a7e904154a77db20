"""-m gpu: the resident map (ptam_rmap, host.ResidentMap) against the references the host-table calls are tested with:
tests/map_edit_ref.py for the edits, tests/plane_ref.py for the scene depth.  Tables are compared by tobytes(), counts by ==.
After every call the redundant columns of the point side are equal and tests/map_edit_ref.tables_valid holds (check_invariants)."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import map_ba_ref as R
from tests import map_edit_ref as E
from tests import map_refind_ref as F
from tests import plane_ref as PR

pytestmark = pytest.mark.gpu
E_ARG = -1      # PTAM_E_ARG
TABLES = tuple(host.ResidentMap.TABLES)
UPLOAD_KEYS = ("poses", "fixed", "points3", "points", "sources", "bad", "meas", "never", "new_queue", "failure", "outlier_count", "inlier_count")
# depth mean and sigma against tests/plane_ref.scene_depth: the tolerance of tests/test_gpu_plane_align.py, derived there
DEPTH_TOL = 9.5e-13


@pytest.fixture(scope="module")
def ctx(hip):
    c = host.Context(lib=hip)
    yield c
    c.close()


def with_point_side(t, seed=9):
    """the tables of tests/map_edit_ref.make_tables with a keyframe side and a point side whose redundant columns agree"""
    rng = np.random.default_rng(seed)
    K, N = t["n_kf"], t["n_points"]
    _, pts, src = E.point_columns(seed, N)
    pts["src_kf"] = rng.integers(0, K, N)
    pts["bad"], src["src_kf"] = t["bad"], pts["src_kf"]
    h = dict(poses=np.stack([PR._small_pose(rng, 0.2) for _ in range(K)]).reshape(K, 12), fixed=(np.arange(K) == 0).astype(np.uint8),
             points3=pts["pv"]["world"].copy(), points=pts, sources=src)
    for k in ("bad", "meas", "never", "new_queue", "failure", "outlier_count", "inlier_count"):
        h[k] = t[k].copy()
    h["points3"][:, 2] += 3.0          # (in front of the cameras: a depth worth comparing)
    h["points"]["pv"]["world"] = h["points3"]
    return h


@pytest.fixture(scope="module")
def case():
    """7 keyframes x 2500 points x about 9000 rows (tests/map_edit_ref.gpu_case), read-only"""
    t = E.gpu_case()
    E.assert_every_class(t)
    h = with_point_side(t)
    h["outliers"], h["made"] = t["outliers"], E.make_made(10, 300)
    for a in h.values():
        a.setflags(write=False)
    return h


def uploaded(ctx, h, **reserve):
    m = host.ResidentMap(ctx)
    if reserve:
        m.reserve(**reserve)
    m.upload(**{k: h[k] for k in UPLOAD_KEYS})
    return m


def same_tables(got, want, keys=TABLES):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k


def check_invariants(tab):
    assert tab["points3"].tobytes() == np.ascontiguousarray(tab["points"]["pv"]["world"]).tobytes()
    assert np.array_equal(tab["bad"], tab["points"]["bad"]) and np.array_equal(tab["sources"]["src_kf"], tab["points"]["src_kf"])
    assert E.tables_valid(len(tab["poses"]), len(tab["points3"]), tab["meas"], tab["never"])
    q, f = tab["new_queue"], tab["failure"]
    assert len(np.unique(q)) == len(q) and (len(q) == 0 or (q.min() >= 0 and q.max() < len(tab["points3"])))
    assert len(f) == 0 or (f["point"].min() >= 0 and f["point"].max() < len(tab["points3"]) and f["kf"].max() < len(tab["poses"]))


# ---- the same edits composed on the host from the references ------------------------------------------------------------------
def tables_of(h):
    return {k: np.array(h[k]) for k in TABLES}


def ref_apply_outliers(h, outliers):
    r = E.np_apply_outliers(len(h["poses"]), h["bad"], h["meas"], h["never"], h["failure"], outliers)
    out = dict(h, bad=r["bad"], meas=r["meas"], never=r["never"], failure=r["failure"], points=h["points"].copy())
    out["points"]["bad"] = r["bad"]
    return out, {f: r[f] for f in E.OUTLIER_COUNTS}


def ref_handle_bad_points(h):
    cols = [h[k] for k in ("points3", "points", "sources", "outlier_count", "inlier_count")]
    r = E.np_handle_bad_points(len(h["poses"]), len(h["points3"]), h["meas"], h["never"], h["bad"], h["outlier_count"], h["inlier_count"],
                               h["new_queue"], h["failure"], cols)
    nk = r["n_kept"]
    out = dict(h, meas=r["meas"], never=r["never"], new_queue=r["new_queue"], failure=r["failure"], bad=np.zeros(nk, np.uint8))
    for k, c in zip(("points3", "points", "sources", "outlier_count", "inlier_count"), r["columns"]):
        out[k] = c[:nk].copy()
    return out, r


def ref_add_points(h, src_kf, target_kf, made, target_source=_abi.SRC_EPIPOLAR):
    r = E.np_add_points(len(h["poses"]), len(h["points3"]), h["meas"], src_kf, target_kf, made, target_source)
    A = len(made)
    return dict(h, meas=r["meas"], points=np.concatenate([h["points"], r["points"]]), sources=np.concatenate([h["sources"], r["sources"]]),
                points3=np.concatenate([h["points3"], made["point"]["world"]]), bad=np.concatenate([h["bad"], np.zeros(A, np.uint8)]),
                outlier_count=np.concatenate([h["outlier_count"], np.zeros(A, np.int32)]),
                inlier_count=np.concatenate([h["inlier_count"], np.zeros(A, np.int32)]), new_queue=np.concatenate([h["new_queue"], r["new_queue"]]))


def ref_add_keyframe(h, pose, fixed, rows):
    new = np.zeros(len(rows), E.MEAS_DT)
    new["kf"], new["point"], new["level"], new["source"], new["root_pos"] = len(h["poses"]), rows["point"], rows["level"], _abi.SRC_TRACKER, rows["root_pos"]
    return dict(h, poses=np.concatenate([h["poses"], np.reshape(pose, (1, 12))]), fixed=np.concatenate([h["fixed"], np.array([fixed], np.uint8)]),
                meas=np.concatenate([h["meas"], new]))


def kf_rows(seed, n_points, n):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, host.MAP_KF_ROW_DT)
    rows["point"] = np.sort(rng.choice(n_points, size=n, replace=False))
    rows["level"], rows["root_pos"] = rng.integers(0, 4, n), rng.random((n, 2)) * 600
    return rows


# ---- 1. round trip ------------------------------------------------------------------------------------------------------------
def test_upload_download_round_trip(ctx, case):
    m = uploaded(ctx, case)
    assert m.counts() == dict(n_kf=7, n_points=2500, n_meas=len(case["meas"]), n_never=len(case["never"]), n_new=len(case["new_queue"]),
                              n_failure=len(case["failure"]))
    tab = m.tables()
    same_tables(tab, tables_of(case))
    check_invariants(tab)
    part = m.download("points", 2400, 100)                 # the tracker's hand-off: a row range
    assert part.tobytes() == case["points"][2400:].tobytes()
    assert m.download("meas", 17, 0).shape == (0,) and m.lib.rmap_download(m.h, _abi.RMAP_MEAS, 17, len(case["meas"]), None) == E_ARG
    up, down = m.traffic()
    assert up == sum(case[k].nbytes for k in UPLOAD_KEYS)
    assert down == _abi.RMAP_WORD_BYTES + sum(case[k].nbytes for k in TABLES) + part.nbytes
    m.close()


def test_upload_without_counts_gives_zero_counts(ctx, case):
    m = host.ResidentMap(ctx)
    m.upload(**{k: case[k] for k in UPLOAD_KEYS if not k.endswith("_count")})
    assert not m.download("outlier_count").any() and not m.download("inlier_count").any()
    m.close()


# ---- 2. the upload's check, on the device ---------------------------------------------------------------------------------------
# the boundaries of a wave (64 rows), of a workgroup of the check kernels (256) and of a compaction tile (1024), and the table's end
ROWS = 2049
PAIRS = [(0, 1), (63, 64), (255, 256), (1023, 1024), (ROWS - 2, ROWS - 1)]


@pytest.fixture(scope="module")
def long_tables():
    """2 049 rows in each of meas, never, failure and new_queue: 5 keyframes x 3 000 points"""
    t = E.make_tables(77, 5, 3000, ROWS, n_never=ROWS, n_new=ROWS, n_failure=ROWS, lonely=0)
    h = with_point_side(t)
    assert all(len(h[k]) == ROWS for k in ("meas", "never", "new_queue", "failure"))
    for a in h.values():
        a.setflags(write=False)
    return h


@pytest.fixture(scope="module")
def checked(ctx, case, long_tables):
    """a map that holds `case`; every refused upload must leave exactly that"""
    m = uploaded(ctx, case)
    before = m.tables()
    yield m, before
    same_tables(m.tables(), before)
    assert m.upload(**{k: long_tables[k] for k in UPLOAD_KEYS}) == 0      # the valid tables are taken
    same_tables(m.tables(), tables_of(long_tables))
    m.close()


def refused(checked, h, table, row, **edits):
    m, before = checked
    a = {k: h[k] for k in UPLOAD_KEYS}
    a.update(edits)
    assert m.upload(check=False, **a) == E_ARG
    assert m.last_refusal() == (table, row), (m.last_refusal(), table, row)
    same_tables(m.tables(), before)


def edited(table, row, **fields):
    t = table.copy()
    for f, v in fields.items():
        t[f][row] = v
    return t


@pytest.mark.parametrize("lo,hi", PAIRS)
def test_upload_names_the_offending_row(checked, long_tables, lo, hi):
    h = long_tables
    K, N = len(h["poses"]), len(h["points3"])
    for key, table in (("meas", _abi.RMAP_MEAS), ("never", _abi.RMAP_NEVER)):
        t = h[key]
        swapped = t.copy()
        swapped[[lo, hi]] = swapped[[hi, lo]]
        refused(checked, h, table, hi, **{key: swapped})                                    # out of order: against its predecessor
        refused(checked, h, table, hi, **{key: edited(t, hi, kf=t["kf"][lo], point=t["point"][lo])})   # a repeated pair
        for row in (lo, hi):
            refused(checked, h, table, row, **{key: edited(t, row, kf=K)})
            refused(checked, h, table, row, **{key: edited(t, row, kf=-1)})
            refused(checked, h, table, row, **{key: edited(t, row, point=N)})
            refused(checked, h, table, row, **{key: edited(t, row, point=-1)})
    for row in (lo, hi):
        for f, v in (("level", 4), ("level", -1), ("source", 5), ("source", -1)):
            refused(checked, h, _abi.RMAP_MEAS, row, meas=edited(h["meas"], row, **{f: v}))
        refused(checked, h, _abi.RMAP_FAILURE, row, failure=edited(h["failure"], row, kf=K))
        refused(checked, h, _abi.RMAP_FAILURE, row, failure=edited(h["failure"], row, point=-1))
        q = h["new_queue"].copy()
        q[row] = N
        refused(checked, h, _abi.RMAP_NEW_QUEUE, row, new_queue=q)
    q = h["new_queue"].copy()
    q[hi] = q[lo]                                                                               # the later entry of a repeated point
    refused(checked, h, _abi.RMAP_NEW_QUEUE, hi, new_queue=q)
    q[hi] = q[0]                                                                                # ... however far back the first one is
    refused(checked, h, _abi.RMAP_NEW_QUEUE, hi, new_queue=q)


def test_upload_names_the_lower_of_two_defects(checked, long_tables):
    h = long_tables
    two = edited(edited(h["meas"], 1500, level=7), 300, source=9)
    refused(checked, h, _abi.RMAP_MEAS, 300, meas=two)
    two = edited(h["never"], 2000, kf=-1)
    two[[64, 65]] = two[[65, 64]]
    refused(checked, h, _abi.RMAP_NEVER, 65, never=two)
    q = h["new_queue"].copy()
    q[1030], q[70] = q[3], -5
    refused(checked, h, _abi.RMAP_NEW_QUEUE, 70, new_queue=q)
    # the first offending table in the documented order is the one named
    refused(checked, h, _abi.RMAP_MEAS, 9, meas=edited(h["meas"], 9, level=4), failure=edited(h["failure"], 2, kf=99))


def test_upload_refuses_redundant_columns_that_differ(checked, long_tables):
    h = long_tables
    p = h["points"].copy()
    p["pv"]["world"][255, 1] = np.nextafter(p["pv"]["world"][255, 1], 1.0)
    refused(checked, h, _abi.RMAP_REFIND_POINTS, 255, points=p)
    refused(checked, h, _abi.RMAP_REFIND_POINTS, 1024, bad=edited(h["bad"].view([("v", "u1")]), 1024, v=1 - h["bad"][1024]).view(np.uint8))
    refused(checked, h, _abi.RMAP_REFIND_POINTS, 64, sources=edited(h["sources"], 64, src_kf=(h["sources"]["src_kf"][64] + 1) % 5))


# ---- 3. each resident form against its reference --------------------------------------------------------------------------------
def test_apply_outliers_matches_reference(ctx, case):
    m = uploaded(ctx, case)
    want, counts = ref_apply_outliers(case, case["outliers"])
    assert m.apply_outliers(case["outliers"]) == counts
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    assert m.apply_outliers(case["outliers"][:0])["n_meas_out"] == counts["n_meas_out"]
    m.close()


@pytest.mark.parametrize("counts", [True, False])
def test_handle_bad_points_matches_reference(ctx, case, counts):
    h = dict(case)
    if not counts:
        h["outlier_count"] = h["inlier_count"] = np.zeros(len(case["bad"]), np.int32)
    m = uploaded(ctx, h)
    want, r = ref_handle_bad_points(h)
    got = m.handle_bad_points(kept=True, new_index=True)
    E.assert_same(got, r, E.BAD_COUNTS, ("kept", "new_index"))
    assert (r["n_marked"] > 0) == counts
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    m.close()


@pytest.mark.parametrize("target_source", [_abi.SRC_EPIPOLAR, _abi.SRC_TRAIL])
@pytest.mark.parametrize("src_kf,target_kf", [(6, 2), (1, 5), (0, 6), (6, 5)])
def test_add_points_matches_reference(ctx, case, src_kf, target_kf, target_source):
    m = uploaded(ctx, case)
    m.add_points(src_kf, target_kf, case["made"], target_source)
    tab = m.tables()
    same_tables(tab, tables_of(ref_add_points(case, src_kf, target_kf, case["made"], target_source)))
    check_invariants(tab)
    m.add_points(src_kf, target_kf, case["made"][:0])       # nothing to add: nothing changes
    same_tables(m.tables(), tab)
    m.close()


def test_add_points_into_an_empty_map(ctx, case):
    h = {k: case[k][:0] for k in UPLOAD_KEYS}
    h["poses"], h["fixed"] = case["poses"][:2], case["fixed"][:2]
    m = uploaded(ctx, h)
    m.add_points(1, 0, case["made"][:5])
    tab = m.tables()
    same_tables(tab, tables_of(ref_add_points(h, 1, 0, case["made"][:5])))
    check_invariants(tab)
    m.close()


def test_add_keyframe_matches_reference(ctx, case):
    m = uploaded(ctx, case)
    rng = np.random.default_rng(4)
    h = case
    for i, n in enumerate((300, 0, 65)):
        pose, rows = PR._small_pose(rng, 0.2), kf_rows(20 + i, 2500, n)
        m.add_keyframe(pose, i == 1, rows)
        h = ref_add_keyframe(h, pose, i == 1, rows)
    tab = m.tables()
    same_tables(tab, tables_of(h))
    check_invariants(tab)
    assert m.counts()["n_kf"] == 10
    m.add_points(9, 3, case["made"])                          # the new keyframes are keyframes of the table
    same_tables(m.tables(), tables_of(ref_add_points(h, 9, 3, case["made"])))
    m.close()


def test_note_tracked_matches_reference(ctx, case):
    m = uploaded(ctx, case)
    rng = np.random.default_rng(6)
    pts = np.concatenate([rng.permutation(2500)[:1500], np.full(70, 11), rng.integers(0, 2500, 500)]).astype(np.int32)   # (one point 70 times)
    flags = (rng.random(len(pts)) < 0.4).astype(np.uint8)
    oc, ic = case["outlier_count"].copy(), case["inlier_count"].copy()
    np.add.at(oc, pts[flags != 0], 1)
    np.add.at(ic, pts[flags == 0], 1)
    m.note_tracked(pts, flags)
    tab = m.tables()
    same_tables(tab, tables_of(dict(case, outlier_count=oc, inlier_count=ic)))
    assert m.lib.rmap_note_tracked(m.h, 1, host._ptr(np.array([2500], np.int32)), host._ptr(flags)) == E_ARG
    same_tables(m.tables(), tab)
    m.close()


def test_scene_depth_matches_reference(ctx, case):
    m = uploaded(ctx, case)
    got = m.scene_depth()
    ref = PR.scene_depth(case["poses"], case["points3"], case["meas"])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    figures = dict(mean=rel(got["depth_mean"], ref[:, 0]), sigma=rel(got["depth_sigma"], ref[:, 1]))
    print(figures)
    assert got["n_meas"].tolist() == ref[:, 2].astype(int).tolist() and max(figures.values()) <= DEPTH_TOL
    assert got.tobytes() == host.map_scene_depth(ctx, case["poses"], case["points3"], case["meas"]).tobytes()   # the same kernel
    m.close()


# the compaction's boundaries, through the resident handle_bad_points (the 1024^2 scan round: tests/test_gpu_map_edit.py)
def removed_pattern(n, pattern):
    bad = np.zeros(n, np.uint8)
    if pattern == "all":
        bad[:] = 1
    elif pattern == "first":
        bad[:1] = 1
    elif pattern == "last":
        bad[-1:] = 1
    elif pattern == "alternating":
        bad[::2] = 1
    return bad


@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "alternating"])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_handle_bad_points_at_the_compaction_boundaries(ctx, n, pattern):
    """n points, n rows, n queue entries: one row per point, keyframe = point % 3"""
    t = E.make_tables(n, 3, n, 0, n_never=0, n_new=n, n_failure=n, lonely=0)
    pt = np.arange(n, dtype=np.int32)
    order = np.lexsort((pt, pt % 3))
    t["meas"] = np.zeros(n, E.MEAS_DT)
    t["meas"]["kf"], t["meas"]["point"], t["meas"]["level"] = (pt % 3)[order], pt[order], pt % 4
    t["bad"] = removed_pattern(n, pattern)
    t["outlier_count"][:] = 0
    h = with_point_side(t, seed=n)
    m = uploaded(ctx, h)
    want, r = ref_handle_bad_points(h)
    E.assert_same(m.handle_bad_points(kept=True), r, E.BAD_COUNTS, ("kept",))
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    m.close()


# ---- 4. transactions ------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_map_as_it_was(ctx, case):
    m = uploaded(ctx, case)
    before = m.tables()
    out = case["outliers"]
    N = len(case["points3"])
    nv = np.flatnonzero(out["action"] == _abi.OUT_NEVER_RETRY)[0]
    wrong_row = edited(out, 130, point=(out["point"][130] + 1) % N)
    twice = out.copy()
    twice[300] = twice[4]
    both = twice.copy()
    both[70] = wrong_row[130]
    both[70]["point"] = (both[70]["point"] + 1) % N
    for name, lst, row in (("an outlier that names another row", wrong_row, 130), ("a row named twice", twice, 300),
                           ("two offences: the lower index", both, 70)):
        assert m.apply_outliers(lst, check=False) == E_ARG, name
        assert m.last_refusal() == (_abi.RMAP_OUTLIERS, row), name
        same_tables(m.tables(), before)
    for name, lst in (("action 0", edited(out, 2, action=0)), ("row outside the table", edited(out, 2, meas=len(case["meas"])))):
        assert m.apply_outliers(lst, check=False) == E_ARG, name                  # (decided on the host, from the list)
        same_tables(m.tables(), before)
    want, counts = ref_apply_outliers(case, out)
    assert m.apply_outliers(out) == counts                                       # the same call with valid input
    same_tables(m.tables(), tables_of(want))
    # a never pair that is already present: the list once more, after its NEVER_RETRY pairs have entered the table.  Row
    # numbers have moved, so the list is rebuilt for the new table from one surviving row and one pair now in never
    tab = m.tables()
    again = np.zeros(2, E.OUTLIER_DT)
    again[0] = (tab["meas"]["point"][5], tab["meas"]["kf"][5], _abi.OUT_FAILURE_QUEUE, 5)
    again[1] = (tab["meas"]["point"][9], tab["meas"]["kf"][9], _abi.OUT_NEVER_RETRY, 9)
    clash = tab["never"].copy()
    m2 = uploaded(ctx, dict(want, never=E.sort_pairs(np.concatenate([clash, E.pairs_of(again[1:])]))))
    before2 = m2.tables()
    assert m2.apply_outliers(again, check=False) == E_ARG and m2.last_refusal() == (_abi.RMAP_OUTLIERS, 1)
    same_tables(m2.tables(), before2)
    assert out["action"][nv] == _abi.OUT_NEVER_RETRY
    m2.close()
    # add_points and add_keyframe
    before = m.tables()
    assert m.add_points(3, 3, case["made"], check=False) == E_ARG
    assert m.add_points(7, 3, case["made"], check=False) == E_ARG
    assert m.add_points(6, 3, edited(case["made"], 9, level=4), check=False) == E_ARG
    rows = kf_rows(1, N, 50)
    unsorted_rows = rows.copy()
    unsorted_rows[[20, 21]] = unsorted_rows[[21, 20]]
    pose = case["poses"][0]
    assert m.add_keyframe(pose, 0, unsorted_rows, check=False) == E_ARG
    assert m.add_keyframe(pose, 0, edited(rows, 49, point=N), check=False) == E_ARG
    assert m.add_keyframe(pose, 0, edited(rows, 3, level=-1), check=False) == E_ARG
    same_tables(m.tables(), before)
    m.add_points(6, 3, case["made"])
    m.add_keyframe(pose, 0, rows)
    same_tables(m.tables(), tables_of(ref_add_keyframe(ref_add_points(want, 6, 3, case["made"]), pose, 0, rows)))
    m.close()


# ---- 5. growth --------------------------------------------------------------------------------------------------------------------
def test_growth_gives_the_same_tables(ctx, case):
    c = dict(n_kf=7, n_points=2500, n_meas=len(case["meas"]), n_never=len(case["never"]), n_new=len(case["new_queue"]),
             n_failure=len(case["failure"]))
    tight = uploaded(ctx, case, **{k: v + 1 for k, v in c.items()})
    roomy = uploaded(ctx, case, **{k: 8 * v + 4096 for k, v in c.items()})
    for m in (tight, roomy):
        m.apply_outliers(case["outliers"])                                        # never and failure grow in `tight`
    h, counts = ref_apply_outliers(case, case["outliers"])
    assert counts["n_never_added"] > 1 and counts["n_failure_added"] > 1
    rng = np.random.default_rng(8)
    for step in range(3):
        made = E.make_made(30 + step, 200)
        pose, rows = PR._small_pose(rng, 0.2), kf_rows(40 + step, len(h["points3"]), 400)
        for m in (tight, roomy):
            m.add_points(6, step, made)
            m.add_keyframe(pose, 0, rows)
        h = ref_add_keyframe(ref_add_points(h, 6, step, made), pose, 0, rows)
    # the capacities of `tight` that have been passed: meas, the six point-side tables, new_queue (and never and failure above)
    assert len(h["meas"]) > c["n_meas"] + 1 and len(h["points3"]) > 2501 and len(h["new_queue"]) > c["n_new"] + 1
    a, b = tight.tables(), roomy.tables()
    same_tables(a, b)
    same_tables(a, tables_of(h))
    check_invariants(a)
    tight.close()
    roomy.close()


# ---- 6. the bundle ------------------------------------------------------------------------------------------------------------------
BA_COUNTS = tuple(f for f, _ in _abi.MapBaResult._fields_)


def with_ba_tables(poses, fixed, points, meas, seed=3):
    """the four tables of tests/map_ba_ref.map_from_problem as a whole map: a point side around them, empty queues"""
    rng = np.random.default_rng(seed)
    N = len(points)
    _, pts, src = E.point_columns(seed, N)
    pts["pv"]["world"], pts["src_kf"] = points, rng.integers(0, len(poses), N)
    src["src_kf"] = pts["src_kf"]
    return dict(poses=np.array(poses), fixed=np.array(fixed, np.uint8), points3=np.array(points), points=pts, sources=src, bad=np.zeros(N, np.uint8),
                meas=np.array(meas), never=np.zeros(0, E.PAIR_DT), new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT),
                outlier_count=np.zeros(N, np.int32), inlier_count=np.zeros(N, np.int32))


def ref_bundle(ctx, h, mode, **kw):
    """tests/map_ba_ref.compose on the host tables -> the tables after it, the composed path's result"""
    r = R.compose(ctx, mode, h["poses"], h["fixed"], h["points3"], h["meas"], **kw)
    out = dict(h, poses=r["poses"], points3=r["points"], points=h["points"].copy())
    out["points"]["pv"]["world"] = r["points"]
    return out, r


def same_bundle(got, ref):
    for k in BA_COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("cam_kf", "point_ids", "outliers"):
        assert got[k].tobytes() == ref[k].tobytes(), k


@pytest.mark.parametrize("mode", [_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL])
@pytest.mark.parametrize("K,P", [(8, 400), (20, 1500), (50, 3000)])
def test_bundle_equals_the_composed_path_bit_for_bit(ctx, mode, K, P):
    """the sizes of tests/test_gpu_map_ba.py's bit-for-bit test, and its maps"""
    prob = synth.make_ba_problem(K, P, K, window=6)
    h = with_ba_tables(*R.map_from_problem(prob, seed=K, extra_fixed=(K // 2, K // 3)))
    want, ref = ref_bundle(ctx, h, mode, deterministic=1)
    m = uploaded(ctx, h)
    up0, down0 = m.traffic()
    got = m.bundle_adjust(mode, deterministic=1)
    up, down = m.traffic()
    assert got["ran"] == 1 and got["accepted"] > 0 and got["n_meas"] > 0
    same_bundle(got, ref)
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    assert up - up0 <= 97 * K
    assert down - down0 <= 32 + 4 * K + 96 * K + got["outliers"].nbytes + got["point_ids"].nbytes
    m.close()


def test_bundle_that_does_not_run_or_is_aborted_leaves_the_map(ctx):
    h = with_ba_tables(*R.map_from_problem(synth.make_ba_problem(7, 300, 2, window=6), seed=2, extra_fixed=(3, 2)))
    m = uploaded(ctx, h)
    got = m.bundle_adjust(_abi.MAP_BA_RECENT)                                     # below 8 keyframes (:790-793)
    assert all(got[k] == 0 for k in BA_COUNTS) and len(got["outliers"]) == 0
    same_tables(m.tables(), tables_of(h))
    m.close()
    h = with_ba_tables(*R.map_from_problem(synth.make_ba_problem(12, 600, 6, window=6), seed=6, extra_fixed=(6, 4)))
    m = uploaded(ctx, h)
    for mode in (_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL):
        got = m.bundle_adjust(mode, abort=np.ones(1, np.uint8))
        assert got["ran"] == 1 and got["accepted"] == 0
        same_tables(m.tables(), tables_of(h))
    m.close()


# ---- 7. / 8. the calls of one iteration in a row, nothing downloaded in between, and what crossed the host link --------------------
def test_one_iteration_stays_on_the_device(ctx):
    """bundle RECENT, its outliers, bundle ALL, its outliers, the tracker's counts, HandleBadPoints, a keyframe, new points, the
    scene depth — on the resident map, and composed on the host from the references with each step's tables fed to the next.  (The
    whole iteration, with its three re-find steps, on a map that has keyframes to search: tests/test_gpu_resident_map_refind.py.)"""
    prob = synth.make_ba_problem(14, 900, 21, window=6, outlier_frac=0.1)
    h = with_ba_tables(*R.map_from_problem(prob, seed=21))
    K = 14
    m = uploaded(ctx, h)
    up0, down0 = m.traffic()
    up_bound = down_bound = 0
    W = _abi.RMAP_WORD_BYTES
    n_outliers = 0
    for mode in (_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL):
        h, ref = ref_bundle(ctx, h, mode, deterministic=1)
        got = m.bundle_adjust(mode, deterministic=1)
        same_bundle(got, ref)
        h, counts = ref_apply_outliers(h, ref["outliers"])
        assert m.apply_outliers(got["outliers"]) == counts
        n_outliers += len(got["outliers"])
        up_bound += 97 * K + got["outliers"].nbytes                               # the mirror's poses; the outlier list
        down_bound += (32 + 4 * K) + 96 * K + got["outliers"].nbytes + got["point_ids"].nbytes + W
    assert n_outliers > 0
    rng = np.random.default_rng(12)
    pts = rng.integers(0, 900, 4000).astype(np.int32)
    flags = (rng.random(4000) < 0.3).astype(np.uint8)
    pts[:60], flags[:60] = 17, 1                                                  # one point the counts mark
    np.add.at(h["outlier_count"], pts[flags != 0], 1)
    np.add.at(h["inlier_count"], pts[flags == 0], 1)
    m.note_tracked(pts, flags)
    h, r = ref_handle_bad_points(h)
    got = m.handle_bad_points(kept=True)
    E.assert_same(got, r, E.BAD_COUNTS, ("kept",))
    assert r["n_marked"] >= 1 and r["n_removed"] > r["n_marked"]
    pose, rows, made = PR._small_pose(rng, 0.2), kf_rows(13, r["n_kept"], 300), E.make_made(14, 120)
    m.add_keyframe(pose, 0, rows)
    m.add_points(K, 5, made)
    h = ref_add_points(ref_add_keyframe(h, pose, 0, rows), K, 5, made)
    depth = m.scene_depth()
    up, down = m.traffic()
    # 8. sums over the arguments passed and the outputs asked for; no term grows with the measurement table
    up_bound += pts.nbytes + flags.nbytes + (96 + 1 + rows.nbytes) + made.nbytes
    down_bound += W + got["kept"].nbytes + depth.nbytes
    assert up - up0 <= up_bound and down - down0 <= down_bound, (up - up0, up_bound, down - down0, down_bound)
    tab = m.tables()                                                              # the one download, at the end
    same_tables(tab, tables_of(h))
    check_invariants(tab)
    assert depth.tobytes() == host.map_scene_depth(ctx, h["poses"], h["points3"], h["meas"]).tobytes()
    m.close()


# ---- the edits alone, on the larger tables of the edit tests ----------------------------------------------------------------------
def test_a_sequence_of_edits_stays_on_the_device(ctx, case):
    m = uploaded(ctx, case)
    up0, down0 = m.traffic()
    rng = np.random.default_rng(12)
    pts = rng.integers(0, 2500, 900).astype(np.int32)
    flags = (rng.random(900) < 0.5).astype(np.uint8)
    pose, rows = PR._small_pose(rng, 0.2), None
    h = dict(case, outlier_count=case["outlier_count"].copy(), inlier_count=case["inlier_count"].copy())
    np.add.at(h["outlier_count"], pts[flags != 0], 1)
    np.add.at(h["inlier_count"], pts[flags == 0], 1)
    m.note_tracked(pts, flags)
    h, counts = ref_apply_outliers(h, case["outliers"])
    assert m.apply_outliers(case["outliers"]) == counts
    h, r = ref_handle_bad_points(h)
    got = m.handle_bad_points(kept=True)
    E.assert_same(got, r, E.BAD_COUNTS, ("kept",))
    rows = kf_rows(13, r["n_kept"], 500)
    m.add_keyframe(pose, 0, rows)
    h = ref_add_keyframe(h, pose, 0, rows)
    m.add_points(7, 2, case["made"])
    h = ref_add_points(h, 7, 2, case["made"])
    depth = m.scene_depth()
    up, down = m.traffic()
    W = _abi.RMAP_WORD_BYTES
    # 8. the bytes of the small inputs passed, and of the outputs asked for plus the word block of the calls that read one
    assert up - up0 <= pts.nbytes + flags.nbytes + case["outliers"].nbytes + (96 + 1 + rows.nbytes) + case["made"].nbytes
    assert down - down0 <= 2 * W + got["kept"].nbytes + depth.nbytes
    tab = m.tables()                                                              # the one download, at the end
    same_tables(tab, tables_of(h))
    check_invariants(tab)
    assert depth.tobytes() == host.map_scene_depth(ctx, h["poses"], h["points3"], h["meas"]).tobytes()
    m.close()


# ---- 9. empty tables: every zero-sized piece of a call's layout ------------------------------------------------------------------
def test_empty_tables_in_both_forms(ctx):
    """2 keyframes, 3 points and no row, never pair, queue entry or failure pair: HandleBadPoints, two new points and a KEYFRAME
    re-find, each on the host tables and on a freshly uploaded resident map, against tests/map_edit_ref.py / tests/map_refind_ref.py
    and against each other."""
    scene = F.make_scene(ctx, n_kf=2)
    K, N = 2, 3
    pts = scene["points"][:N].copy()
    src = np.zeros(N, host.MAP_POINT_SOURCE_DT)
    src["src_kf"] = pts["src_kf"]
    for f in ("center_nc", "one_right_nc", "one_down_nc"):
        src[f] = (0.1, -0.2, 1.0)
    h = dict(poses=np.array(scene["poses"]), fixed=np.array([1, 0], np.uint8), points3=np.ascontiguousarray(pts["pv"]["world"]), points=pts,
             sources=src, bad=np.zeros(N, np.uint8), meas=np.zeros(0, E.MEAS_DT), never=np.zeros(0, E.PAIR_DT), new_queue=np.zeros(0, np.int32),
             failure=np.zeros(0, E.PAIR_DT), outlier_count=np.zeros(N, np.int32), inlier_count=np.zeros(N, np.int32))

    def fresh():
        m = host.ResidentMap(ctx)
        m.upload(kfs=scene["kfs"], **{k: h[k] for k in UPLOAD_KEYS})
        return m
    # HandleBadPoints: nothing is bad, nothing moves
    want, r = ref_handle_bad_points(h)
    cols = [h[k] for k in ("points3", "points", "sources", "outlier_count", "inlier_count")]
    got = host.map_handle_bad_points(ctx, K, N, h["meas"], h["never"], h["bad"], h["outlier_count"], h["inlier_count"], h["new_queue"], h["failure"], cols)
    E.assert_same(got, r, E.BAD_COUNTS, ("new_index", "kept", "meas", "never", "new_queue", "failure"))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["columns"], r["columns"]))
    m = fresh()
    E.assert_same(m.handle_bad_points(kept=True, new_index=True), r, E.BAD_COUNTS, ("kept", "new_index"))
    assert r["n_kept"] == N and r["n_meas_out"] == 0
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    m.close()
    # two new points
    made = E.make_made(3, 2)
    ref = E.np_add_points(K, N, h["meas"], 1, 0, made)
    E.assert_same(host.map_add_points(ctx, K, N, h["meas"], 1, 0, made), ref, (), ("meas", "points", "sources", "new_queue"))
    m = fresh()
    m.add_points(1, 0, made)
    tab = m.tables()
    same_tables(tab, tables_of(ref_add_points(h, 1, 0, made)))
    assert tab["meas"].tobytes() == ref["meas"].tobytes() and len(ref["meas"]) == 4
    check_invariants(tab)
    m.close()
    # a KEYFRAME re-find: three pairs, the merged tables are the found rows and the new never pairs alone
    work = np.array([0], np.int32)
    rf = [host.ReFinder(ctx) for _ in range(3)]
    ref = F.compose(ctx, rf[0], _abi.MAP_REFIND_KEYFRAME, scene["kfs"], h["poses"], h["points"], h["meas"], h["never"], work)
    got = host.map_refind(ctx, rf[1], _abi.MAP_REFIND_KEYFRAME, scene["kfs"], h["poses"], h["points"], h["meas"], h["never"], work)
    m = fresh()
    res = m.refind(rf[2], _abi.MAP_REFIND_KEYFRAME, work)
    lists = ("found", "found_subpix", "never")
    assert ref["n_pairs"] == N and ref["n_skipped"] == 0 and ref["n_found"] + ref["n_never"] == N
    E.assert_same(got, ref, F.COUNTS, lists + ("meas_merged", "never_merged"))
    E.assert_same(res, ref, F.COUNTS, lists)
    tab = m.tables()
    same_tables(tab, tables_of(dict(h, meas=ref["meas_merged"], never=ref["never_merged"])))
    check_invariants(tab)
    m.close()
    for f in rf:
        f.close()
    scene["close"]()

