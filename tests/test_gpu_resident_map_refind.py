"""-m gpu: the resident forms of re-find and of the global transform (ptam_rmap_refind, ptam_rmap_apply_global_transform) and one
whole MapMaker::run() iteration on a resident map, against the references of the host-table calls: tests/map_refind_ref.compose on
tests/map_refind_ref.make_scene, tests/plane_ref.apply_global_transform, tests/map_ba_ref.compose(deterministic=1) and
tests/map_edit_ref.  Tables by tobytes(), counts by ==; the transform's continuous results under the tolerance of
tests/test_gpu_plane_align.py beside bit equality with the host-table form."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import map_edit_ref as E
from tests import map_refind_ref as F
from tests import plane_ref as PR
from tests.test_gpu_resident_map import (TABLES, UPLOAD_KEYS, check_invariants, kf_rows, ref_add_keyframe, ref_add_points, ref_apply_outliers,
                                         ref_bundle, ref_handle_bad_points, same_bundle, same_tables, tables_of)

pytestmark = pytest.mark.gpu
KEYFRAME, NEW_POINTS, QUEUE = _abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE
LISTS = ("found", "found_subpix", "never")
TRANSFORM_TOL = 9.5e-13      # tests/test_gpu_plane_align.py: derived there for the maps of tests/plane_ref.make_map


@pytest.fixture(scope="module")
def dev(hip):
    ctx = host.Context(lib=hip)
    scene = F.make_scene(ctx)
    yield ctx, scene
    scene["close"]()
    ctx.close()


def scene_map(scene, points=None, new_queue=None, failure=None, seed=5):
    """the scene's tables as a whole map: sources that agree with the point rows, zero counts"""
    rng = np.random.default_rng(seed)
    pts = np.array(scene["points"] if points is None else points)
    N, K = len(pts), len(scene["kfs"])
    src = np.zeros(N, host.MAP_POINT_SOURCE_DT)
    src["src_kf"] = pts["src_kf"]
    for f in ("center_nc", "one_right_nc", "one_down_nc"):
        src[f] = rng.uniform(-0.3, 0.3, (N, 3))
        src[f][:, 2] = 1.0
    return dict(poses=np.array(scene["poses"]), fixed=(np.arange(K) == 0).astype(np.uint8), points3=np.ascontiguousarray(pts["pv"]["world"]),
                points=pts, sources=src, bad=(pts["bad"] != 0).astype(np.uint8), meas=np.array(scene["meas"]), never=np.array(scene["never"]),
                new_queue=np.zeros(0, np.int32) if new_queue is None else np.array(new_queue, np.int32),
                failure=np.zeros(0, E.PAIR_DT) if failure is None else np.array(failure),
                outlier_count=np.zeros(N, np.int32), inlier_count=np.zeros(N, np.int32))


def uploaded(ctx, h, kfs):
    m = host.ResidentMap(ctx)
    m.upload(kfs=kfs, **{k: h[k] for k in UPLOAD_KEYS})
    return m


def ref_refind(ctx, finder, h, kfs, mode, work):
    r = F.compose(ctx, finder, mode, kfs, h["poses"], h["points"], h["meas"], h["never"], work)
    return dict(h, meas=r["meas_merged"], never=r["never_merged"]), r


def same_refind(got, ref, lists=True):
    for f in F.COUNTS:
        assert got[f] == ref[f], (f, got[f], ref[f])
    for f in LISTS if lists else ():
        assert got[f].dtype == ref[f].dtype and got[f].tobytes() == ref[f].tobytes(), f


def free_pairs(h, n, seed=1):
    """pairs that are in neither table: a second call's work"""
    rng = np.random.default_rng(seed)
    busy = set(zip(h["meas"]["kf"].tolist(), h["meas"]["point"].tolist())) | set(zip(h["never"]["kf"].tolist(), h["never"]["point"].tolist()))
    q = []
    while len(q) < n:
        kp = (int(rng.integers(0, len(h["poses"]))), int(rng.integers(0, len(h["points3"]))))
        if kp not in busy and kp not in q:
            q.append(kp)
    out = np.zeros(n, E.PAIR_DT)
    out["kf"], out["point"] = [k for k, _ in q], [p for _, p in q]
    return out


# ---- 6. the three re-find modes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [KEYFRAME, NEW_POINTS, QUEUE], ids=["keyframe", "new_points", "failure_queue"])
def test_refind_equals_the_composed_path_and_the_finder_state_carries(dev, mode):
    ctx, scene = dev
    points, work = F.make_work(mode, scene)
    h = scene_map(scene, points)
    m = uploaded(ctx, h, scene["kfs"])
    up0, down0 = m.traffic()
    rf, rf_ref = host.ReFinder(ctx), host.ReFinder(ctx)
    want, ref = ref_refind(ctx, rf_ref, h, scene["kfs"], mode, work)
    got = m.refind(rf, mode, work)
    same_refind(got, ref)
    assert ref["n_found"] > 0 and ref["n_never"] > 0 and ref["n_skipped"] > 0
    up, down = m.traffic()
    K, W = len(scene["kfs"]), len(work)
    per_entry_up = {KEYFRAME: 0, NEW_POINTS: 4 + 8, QUEUE: 8}[mode]          # a caller's point list goes up; the pair lists go up
    assert up - up0 <= _abi.RMAP_KF_RECORD_BYTES * K + per_entry_up * W             # the level records; the entries
    assert down - down0 <= 16 + (W if mode == NEW_POINTS else 0) + sum(got[f].nbytes for f in LISTS)
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    # a second call, on the merged tables, with the finder as the first call left it
    again = free_pairs(want, 40)
    want2, ref2 = ref_refind(ctx, rf_ref, want, scene["kfs"], QUEUE, again)
    same_refind(m.refind(rf, QUEUE, again), ref2)
    same_tables(m.tables(), tables_of(want2))
    # without the lists only the counts come down
    before = m.traffic()[1]
    assert m.refind(rf, QUEUE, again, lists=False)["n_skipped"] == len(again)
    assert m.traffic()[1] - before == 16
    for f in (rf, rf_ref):
        f.close()
    m.close()


def test_refind_from_the_resident_queues(dev):
    ctx, scene = dev
    points, new = F.make_work(NEW_POINTS, scene)
    _, fq = F.make_work(QUEUE, scene)
    h = scene_map(scene, points, new_queue=new, failure=fq)
    m = uploaded(ctx, h, scene["kfs"])
    rf, rf_ref = host.ReFinder(ctx), host.ReFinder(ctx)
    # a raised flag: nothing is visited and nothing popped
    s = m.refind(rf, NEW_POINTS, stop=np.ones(1, np.uint8))
    assert s["stopped"] == 1 and s["points_consumed"] == 0 and s["n_pairs"] == 0
    same_tables(m.tables(), tables_of(h))
    # work == NULL: the queue is the work, and points_consumed entries leave it
    want, ref = ref_refind(ctx, rf_ref, h, scene["kfs"], NEW_POINTS, new)
    got = m.refind(rf, NEW_POINTS)
    same_refind(got, ref)
    assert got["points_consumed"] == len(new) and got["n_bad_points"] == 3 and m.counts()["n_new"] == 0
    want = dict(want, new_queue=new[got["points_consumed"]:])
    same_tables(m.tables(), tables_of(want))
    # the failure queue: visited sorted, then cleared (:1080)
    want, ref = ref_refind(ctx, rf_ref, want, scene["kfs"], QUEUE, fq)
    same_refind(m.refind(rf, QUEUE), ref)
    want = dict(want, failure=fq[:0])
    tab = m.tables()
    same_tables(tab, tables_of(want))
    check_invariants(tab)
    assert m.refind(rf, QUEUE)["n_pairs"] == 0                                     # an empty queue
    # a map whose keyframes came without handles cannot re-find
    bare = host.ResidentMap(ctx)
    bare.upload(**{k: h[k] for k in UPLOAD_KEYS})
    assert bare.lib.rmap_refind(bare.h, rf.h, None, NEW_POINTS, 0, None, None, host.C.byref(_abi.MapRefindResult()), None, None, None, 0) == -1
    same_tables(bare.tables(), tables_of(h))
    bare.close()
    for f in (rf, rf_ref):
        f.close()
    m.close()


# ---- 3. the global transform -------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("n,n_kf", [(65, 2), (2000, 6)])
def test_global_transform_matches_reference(dev, n, n_kf):
    ctx, _ = dev
    points, poses, sources, meas, _ = PR.make_map(n, 7, n_kf)
    rng = np.random.default_rng(n)
    se3 = PR._small_pose(rng, 0.4)
    right, down = PR.pixel_vectors(poses, points, sources)
    pts = host.map_refind_points(points, right, down, sources["src_kf"], rng.integers(0, 4, n), rng.integers(0, 400, (n, 2)))
    h = dict(poses=np.array(poses), fixed=np.zeros(n_kf, np.uint8), points3=np.array(points), points=pts, sources=np.array(sources),
             bad=np.zeros(n, np.uint8), meas=np.array(meas), never=np.zeros(0, E.PAIR_DT), new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT),
             outlier_count=np.zeros(n, np.int32), inlier_count=np.zeros(n, np.int32))
    m = host.ResidentMap(ctx)
    m.upload(**{k: h[k] for k in UPLOAD_KEYS})
    up0, down0 = m.traffic()
    rows = m.apply_global_transform(se3)
    up, down_ = m.traffic()
    assert up - up0 <= 256 and down_ - down0 <= 96 * n_kf + rows.nbytes
    tab = m.tables()
    check_invariants(tab)
    # the same kernel as the host-table form: the same bits
    poses_t, points_t, pvs_t = host.map_apply_global_transform(ctx, se3, poses, points, sources)
    assert tab["poses"].tobytes() == poses_t.tobytes() and tab["points3"].tobytes() == points_t.tobytes()
    assert rows.tobytes() == pvs_t.tobytes() and np.ascontiguousarray(tab["points"]["pv"]).tobytes() == pvs_t.tobytes()
    want = dict(h, poses=tab["poses"], points3=tab["points3"], points=tab["points"])
    want["points"] = h["points"].copy()
    want["points"]["pv"] = pvs_t
    same_tables(tab, tables_of(want))                                              # nothing else moved
    # the restatement
    rp, rx, (rr, rd) = PR.apply_global_transform(se3, poses, points, sources)
    figures = dict(poses=_rel(tab["poses"], rp), points=_rel(tab["points3"], rx), right=_rel(rows["pixel_right_w"], rr), down=_rel(rows["pixel_down_w"], rd))
    print(figures)
    assert max(figures.values()) <= TRANSFORM_TOL, figures
    before = m.traffic()[1]
    assert m.apply_global_transform(se3, rows=False) is None                       # the rows come down only when asked for
    assert m.traffic()[1] - before == 96 * n_kf
    assert m.scene_depth().tobytes() == host.map_scene_depth(ctx, m.download("poses"), m.download("points3"), meas).tobytes()   # the mirror moved too
    m.close()


def test_global_transform_on_a_fresh_context_grows_the_scratch_once(hip):
    """a context whose scratch has never been asked for: the aligner's record and the packed rows of the first call are one request.
    2 keyframes x 300 points; bit for bit the host-table form on a second context; the traffic bound of the test above."""
    n, n_kf = 300, 2
    points, poses, sources, meas, _ = PR.make_map(n, 7, n_kf)
    rng = np.random.default_rng(n)
    se3 = PR._small_pose(rng, 0.4)
    right, down = PR.pixel_vectors(poses, points, sources)
    pts = host.map_refind_points(points, right, down, sources["src_kf"], rng.integers(0, 4, n), rng.integers(0, 400, (n, 2)))
    h = dict(poses=np.array(poses), fixed=np.zeros(n_kf, np.uint8), points3=np.array(points), points=pts, sources=np.array(sources),
             bad=np.zeros(n, np.uint8), meas=np.array(meas), never=np.zeros(0, E.PAIR_DT), new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT),
             outlier_count=np.zeros(n, np.int32), inlier_count=np.zeros(n, np.int32))
    fresh, second = host.Context(lib=hip), host.Context(lib=hip)
    m = host.ResidentMap(fresh)
    m.upload(**{k: h[k] for k in UPLOAD_KEYS})
    up0, down0 = m.traffic()
    rows = m.apply_global_transform(se3, rows=True)                                # at once: nothing has grown the scratch for it
    up, down_ = m.traffic()
    assert up - up0 <= 256 and down_ - down0 <= 96 * n_kf + rows.nbytes
    tab = m.tables()
    check_invariants(tab)
    poses_t, points_t, pvs_t = host.map_apply_global_transform(second, se3, poses, points, sources)
    assert tab["poses"].tobytes() == poses_t.tobytes() and tab["points3"].tobytes() == points_t.tobytes()
    assert rows.tobytes() == pvs_t.tobytes() and np.ascontiguousarray(tab["points"]["pv"]).tobytes() == pvs_t.tobytes()
    m.close()
    fresh.close()
    second.close()


# ---- 7. / 8. one whole iteration, the tables never downloaded in between, and what crossed the host link ------------------------------
def test_one_whole_iteration_stays_on_the_device(dev):
    """bundle RECENT, its outliers, re-find the new points, bundle ALL, its outliers, re-find the failure queue, HandleBadPoints, a
    new keyframe, re-find in it, new points, the scene depth: on a resident map of the scene, and composed on the host from the
    reference functions, each step's tables fed to the next.  One download at the end."""
    ctx, scene = dev
    points, new = F.make_work(NEW_POINTS, scene)
    kfs = list(scene["kfs"])
    K, W = len(kfs), _abi.RMAP_WORD_BYTES
    h = scene_map(scene, points, new_queue=new)
    m = uploaded(ctx, h, kfs)
    rf, rf_ref = host.ReFinder(ctx), host.ReFinder(ctx)
    up0, down0 = m.traffic()
    up_bound = down_bound = 0

    def bundle_and_outliers(h, mode):
        nonlocal up_bound, down_bound
        h, ref = ref_bundle(ctx, h, mode, deterministic=1)
        got = m.bundle_adjust(mode, deterministic=1)
        same_bundle(got, ref)
        h, counts = ref_apply_outliers(h, ref["outliers"])
        assert m.apply_outliers(got["outliers"]) == counts
        up_bound += 97 * len(h["poses"]) + got["outliers"].nbytes
        down_bound += 32 + 4 * len(h["poses"]) + 96 * len(h["poses"]) + got["outliers"].nbytes + got["point_ids"].nbytes + W
        return h, got

    def refind(h, mode, work, queue_len):
        nonlocal up_bound, down_bound
        h, ref = ref_refind(ctx, rf_ref, h, kfs, mode, work)
        got = m.refind(rf, mode, None if mode != KEYFRAME else work, lists=False)
        same_refind(got, ref, lists=False)
        up_bound += _abi.RMAP_KF_RECORD_BYTES * len(kfs) + 8 * queue_len                                   # the level records; the pair lists
        down_bound += 16 + {KEYFRAME: 0, NEW_POINTS: 5, QUEUE: 8}[mode] * queue_len   # the counts; the queue itself
        return h, got

    h, b1 = bundle_and_outliers(h, _abi.MAP_BA_RECENT)                               # 1, 2
    h, r3 = refind(h, NEW_POINTS, h["new_queue"], len(h["new_queue"]))             # 3
    h = dict(h, new_queue=h["new_queue"][r3["points_consumed"]:])
    h, b4 = bundle_and_outliers(h, _abi.MAP_BA_ALL)                                  # 4, 5
    h, r6 = refind(h, QUEUE, h["failure"], len(h["failure"]))                      # 6
    h = dict(h, failure=h["failure"][:0])
    h, rb = ref_handle_bad_points(h)                                               # 7
    got = m.handle_bad_points(kept=True)
    E.assert_same(got, rb, E.BAD_COUNTS, ("kept",))
    pose = scene["poses"][3].copy()
    pose[11] += 3e-4 * scene["z"]
    rows = kf_rows(13, rb["n_kept"], 200)
    kfs.append(scene["kfs"][1])
    m.add_keyframe(pose, 0, rows, kf=scene["kfs"][1])                              # 8
    h = ref_add_keyframe(h, pose, 0, rows)
    h, r9 = refind(h, KEYFRAME, np.array([K], np.int32), 0)                        # 9
    made = E.make_made(14, 80)
    made["point"]["world"] = h["points3"][:80] + 1e-3
    m.add_points(K, 5, made)                                                       # 10
    h = ref_add_points(h, K, 5, made)
    depth = m.scene_depth()                                                        # 11
    up, down = m.traffic()
    up_bound += 96 + 1 + rows.nbytes + 4 + made.nbytes                             # the keyframe, its index as KEYFRAME's work, the new points
    down_bound += W + got["kept"].nbytes + depth.nbytes
    assert up - up0 <= up_bound and down - down0 <= down_bound, (up - up0, up_bound, down - down0, down_bound)
    tab = m.tables()
    same_tables(tab, tables_of(h))
    check_invariants(tab)
    assert depth.tobytes() == host.map_scene_depth(ctx, h["poses"], h["points3"], h["meas"]).tobytes()
    assert b1["ran"] == 1 and b4["ran"] == 1 and r3["n_pairs"] > 0 and r9["n_pairs"] == rb["n_kept"] and rb["n_removed"] > 0
    for f in (rf, rf_ref):
        f.close()
    m.close()
