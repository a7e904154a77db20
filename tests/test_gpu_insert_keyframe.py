"""-m gpu: ptam_rmap_insert_keyframe (MapMaker::AddKeyFrameFromTopOfQueue after MakeKeyFrame_Rest as one call on the resident map)
and ptam_rmap_closest_keyframes.  The one call against the sequence of existing resident calls it replaces (the same kernels: every
table, count and result bit for bit) and against the composition of the references on the CPU oracle (tests/insert_keyframe_ref.py,
by the rule and tolerances of tests/test_gpu_mapmaker.py); the closest-keyframe kernel against its numpy restatement.
The scene: three keyframes that are views of the textured plane — a decoy (index 0: the target's image at twice its distance), the
"baseline" target, a third view — whose points were made between the third view and the target at threshold 400; the new keyframe
is the "baseline" source view with a seeded share of those points as its tracker rows."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import insert_keyframe_ref as I
from tests import map_ba_ref as R
from tests import map_refind_ref as F
from tests.test_gpu_mapmaker import _compare
from tests.test_gpu_resident_map import TABLES, UPLOAD_KEYS, check_invariants, same_tables, with_ba_tables

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3
KEYFRAME, QUEUE = _abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_FAILURE_QUEUE
K0 = 3                                                      # keyframes in the map before the call: the new one gets this index
# tests/test_gpu_mapmaker.test_one_call_matches_oracle_composition: the one call against the oracle's per-stage composition
ORACLE_TARGET_ATOL, ORACLE_WORLD_RTOL = 1e-6, 1e-6
# what one call brings down: the closest keyframe (8 + 12), the re-find's counts, the chain's header and four level records
DOWN_BYTES = 20 + 16 + (16 + 4 * host.EPIPOLAR_STATS_DT.itemsize)


def epi_opts(ctx, thr=I.THRESHOLD):
    return host.MapMaker(ctx).opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=thr, **I.DEPTH)


def uploaded(ctx, h, kfs, **reserve):
    m = host.ResidentMap(ctx)
    if reserve:
        m.reserve(**reserve)
    m.upload(kfs=kfs, **{k: h[k] for k in UPLOAD_KEYS})
    return m


@pytest.fixture(scope="module")
def dev(hip):
    """the context, the keyframes and the map's tables before the keyframe arrives, made with the product's own calls; read-only"""
    ctx = host.Context(lib=hip)
    kfs, ka, poses, sp = I.make_keyframes(ctx)
    m = uploaded(ctx, I.empty_tables(poses), kfs)
    made, _ = host.MapMaker(ctx).AddSomeMapPoints(kfs[I.THIRD], poses[I.THIRD], kfs[I.TARGET], poses[I.TARGET], epi_opts(ctx))
    m.add_points(I.THIRD, I.TARGET, made)
    h = m.tables()
    m.close()
    rows = I.tracker_rows(h, sp)
    assert len(h["points3"]) > 300 and 100 < len(rows) < len(h["points3"])
    for a in list(h.values()) + [rows, sp]:
        a.setflags(write=False)
    yield dict(ctx=ctx, kfs=kfs, ka=ka, sp=sp, h=h, rows=rows)
    ctx.close()


def one_call(d, h=None, kfs=None, rows=None, thr=I.THRESHOLD, reserve=None, **opts):
    """-> (the call's result, the tables after it, the traffic it caused, the map, the finder)"""
    ctx = d["ctx"]
    m = uploaded(ctx, d["h"] if h is None else h, d["kfs"] if kfs is None else kfs, **(reserve or {}))
    rf = host.ReFinder(ctx)
    up0, down0 = m.traffic()
    o = m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=thr, **I.DEPTH, **opts)
    res = m.InsertKeyFrame(rf, d["ka"], d["sp"], 0, d["rows"] if rows is None else rows, o)
    up, down = m.traffic()
    return res, m.tables(), (up - up0, down - down0), m, rf


def composed(d, h=None, kfs=None, rows=None, thr=I.THRESHOLD, target_kf=-1, busy_before_refind=False, skip_refind=False, skip_points=False,
             reserve=None):
    """the sequence of existing resident calls the one call replaces -> (dict like the one call's result with the made records,
    the tables, the map, the finder)"""
    ctx = d["ctx"]
    kfs = d["kfs"] if kfs is None else kfs
    rows = d["rows"] if rows is None else rows
    m = uploaded(ctx, d["h"] if h is None else h, kfs, **(reserve or {}))
    rf = host.ReFinder(ctx)
    N = m.counts()["n_points"]
    m.add_keyframe(d["sp"], 0, rows, kf=d["ka"])
    out = dict(kf=K0, target_kf=-1, target_dist=0.0, first_point=N, n_made=0, refind=None, levels=None, made=None)
    before = I.run_busy(m.download("meas"), K0)
    if not skip_refind:
        out["refind"] = m.refind(rf, KEYFRAME, np.array([K0], np.int32), lists=False)
    if not skip_points:
        busy = before if busy_before_refind else I.run_busy(m.download("meas"), K0)
        poses = m.download("poses")
        if target_kf < 0:
            idx, dist = I.closest_keyframes_np(poses, K0, 1)
            target_kf, out["target_dist"] = int(idx[0]), float(dist[0])
        else:
            out["target_dist"] = float(I.linear_dists(poses, K0)[target_kf])
        made, stats = host.MapMaker(ctx).AddSomeMapPoints(d["ka"], d["sp"], kfs[target_kf], poses[target_kf], epi_opts(ctx, thr), busy_level=busy[0],
                                                          busy_root=busy[1])
        m.add_points(K0, target_kf, made)
        out.update(target_kf=target_kf, n_made=len(made), levels=stats, made=made)
    return out, m.tables(), m, rf


def same_result(got, want):
    for f in ("kf", "target_kf", "first_point", "n_made"):
        assert got[f] == want[f], (f, got[f], want[f])
    if want["refind"] is not None:
        for f in F.COUNTS:
            assert got["refind"][f] == want["refind"][f], (f, got["refind"][f], want["refind"][f])
    if want["levels"] is not None:
        assert got["levels"].tobytes() == want["levels"].tobytes(), (got["levels"], want["levels"])


def close_all(*things):
    for t in things:
        t.close()


@pytest.fixture(scope="module")
def pair(dev):
    """the one call and the composed resident sequence on the scene, shared by the tests that only read them"""
    a = one_call(dev)
    b = composed(dev)
    yield a, b
    close_all(a[3], a[4], b[2], b[3])


# ---- 1. one call equals the composed resident sequence --------------------------------------------------------------------------------
def test_one_call_equals_the_composed_resident_sequence(dev, pair):
    (res, tab, _, m, rf), (want, wtab, wm, wrf) = pair
    same_result(res, want)
    same_tables(tab, wtab)
    check_invariants(tab)
    assert m.counts() == wm.counts()
    assert res["target_kf"] == I.TARGET and res["n_made"] > 0 and res["refind"]["n_found"] > 0 and res["refind"]["n_never"] > 0
    assert np.float64(res["target_dist"]).tobytes() == np.float64(want["target_dist"]).tobytes()
    # the new rows are where the result says, and they are the chain's records
    N, A = res["first_point"], res["n_made"]
    assert len(tab["points3"]) == N + A and tab["new_queue"][-A:].tolist() == list(range(N, N + A))
    assert np.ascontiguousarray(m.download("points", N, A)["pv"]).tobytes() == np.ascontiguousarray(want["made"]["point"]).tobytes()
    # the finder's carried state: the same second call on both maps, first on the point the re-find visited last
    last = N - 1
    again = np.zeros(6, host.MAP_PAIR_DT)
    again["kf"], again["point"] = I.DECOY, [last, last - 1, 5, 9, 40, 41]
    r1, r2 = m.refind(rf, QUEUE, again), wm.refind(wrf, QUEUE, again)
    F.assert_same_bits(dict(r1, meas_merged=m.download("meas"), never_merged=m.download("never")),
                       dict(r2, meas_merged=wm.download("meas"), never_merged=wm.download("never")))
    assert r1["n_pairs"] == 6 and r1["n_skipped"] == 0


def test_the_busy_list_is_the_run_after_the_refind(dev, pair):
    """the composed path with the run as it was BEFORE the re-find as its busy list makes other points: the fixture sees the order"""
    (res, tab, _, _, _), _ = pair
    early, etab, em, erf = composed(dev, busy_before_refind=True)
    assert early["levels"].tobytes() != res["levels"].tobytes() and early["n_made"] > res["n_made"]
    assert etab["meas"].tobytes() != tab["meas"].tobytes()
    close_all(em, erf)


# ---- 2. against the CPU oracle composition ----------------------------------------------------------------------------------------------
def test_one_call_matches_the_oracle_composition(dev, pair, oracle):
    (res, tab, _, _, _), (want, _, _, _) = pair
    octx = host.Context(lib=oracle)
    okfs, oka, _, _ = I.make_keyframes(octx)
    ofinder = host.ReFinder(octx)
    ref = I.compose(octx, ofinder, dev["h"], okfs, oka, dev["sp"], 0, dev["rows"])
    # the conditions on the reference: the re-find finds and refuses, points are made, a re-found row thins a candidate
    assert ref["refind"]["n_found"] >= 1 and ref["refind"]["n_never"] >= 1 and len(ref["made"]) >= 1
    assert I.thinned_by_refound_rows(octx, oka, ref) >= 1
    assert ref["target_kf"] == I.TARGET
    # the re-find: the discrete outcome exact, positions by the re-find rule
    for f in F.COUNTS:
        assert res["refind"][f] == ref["refind"][f], (f, res["refind"][f], ref["refind"][f])
    assert np.array_equal(tab["never"], ref["tables"]["never"])
    run = lambda t: t["meas"][(t["meas"]["kf"] == K0) & (t["meas"]["source"] != _abi.SRC_ROOT)]   # the tracker's and the re-found rows
    dr, orr = run(tab), run(ref["tables"])
    assert len(dr) == len(orr) and all(np.array_equal(dr[f], orr[f]) for f in ("point", "source", "level"))
    assert np.abs(dr["root_pos"] - orr["root_pos"]).max() <= ORACLE_TARGET_ATOL
    assert res["target_kf"] == ref["target_kf"] and abs(res["target_dist"] - ref["target_dist"]) <= np.spacing(ref["target_dist"])
    # the new points: the records of the composed resident sequence are the one call's rows (test 1), by _compare's rule
    n = _compare(want["made"], res["levels"], ref["made"], ref["stats"], ref["info"], list(I.KEYFRAME_ORDER), target_atol=ORACLE_TARGET_ATOL,
                 world_rtol=ORACLE_WORLD_RTOL)
    assert n >= 1
    close_all(ofinder, octx)


# ---- 3. ClosestKeyFrames -------------------------------------------------------------------------------------------------------------------
def pose_at(centre, rng=None):
    Rm = synth.so3_exp(rng.uniform(-0.3, 0.3, 3)) if rng is not None else np.eye(3)
    return I.M.camera_pose(np.asarray(centre, np.float64), Rm)


def poses_map(ctx, poses):
    m = host.ResidentMap(ctx)
    m.upload(**{k: v for k, v in I.empty_tables(np.asarray(poses)).items() if k in UPLOAD_KEYS})
    return m


def check_closest(ctx, poses, kf, ns):
    m = poses_map(ctx, poses)
    K = len(poses)
    for n in ns:
        down0 = m.traffic()[1]
        idx, dist = m.ClosestKeyFrames(kf, n)
        widx, wdist = I.closest_keyframes_np(poses, kf, n)
        assert len(idx) == min(n, K - 1) and idx.tolist() == widx.tolist(), (K, kf, n, idx[:8], widx[:8])
        ulps = np.abs(dist - wdist) / np.maximum(np.spacing(wdist), 5e-324)
        print("K", K, "n", n, "max distance error in ulps", ulps.max(initial=0.0))
        assert (ulps <= 1.0).all()                                                  # sqrt of the same fp64 sum: at most its rounding
        assert m.traffic()[1] - down0 == 8 + 12 * len(idx)
    m.close()
    return idx


@pytest.mark.parametrize("K", [2, 5, 64, 65, 1024, 1025])
def test_closest_keyframes_match_numpy(dev, K):
    """n = 1, 4 and n > K - 1 at the sizes of one wave, one stride of the workgroup and one above each; the winner in the last slot"""
    rng = np.random.default_rng(K)
    c = rng.uniform(-5.0, 5.0, (K, 3))
    q = K // 3
    c[K - 1] = c[q] + 1e-3                                                           # nearer than any seeded centre can be
    poses = np.stack([pose_at(c[k], rng) for k in range(K)])
    last = check_closest(dev["ctx"], poses, q, (1, 4, K + 3))
    assert I.closest_keyframes_np(poses, q, 1)[0][0] == K - 1 and len(last) == K - 1 and q not in last.tolist()
    assert sorted(last.tolist()) == [k for k in range(K) if k != q]


def test_closest_keyframes_ties_go_to_the_lower_index(dev):
    """two keyframes at exactly equal distance (a mirrored centre, identity rotations: exact centres), a keyframe at the queried
    one's own pose (distance 0: it is another keyframe and comes first), the queried one never"""
    v = np.array([0.25, -0.5, 0.125])
    centres = [2 * v, -v, np.zeros(3), v, np.zeros(3), 3 * v, -3 * v]                # query = 2; 4 shares its pose; 1 / 3 and 5 / 6 tie
    poses = np.stack([pose_at(c) for c in centres])
    d = I.linear_dists(poses, 2)
    assert d[1] == d[3] and d[5] == d[6] and d[4] == 0.0
    got = check_closest(dev["ctx"], poses, 2, (1, 2, 3, 4, 6, 9))
    assert got.tolist() == [4, 1, 3, 0, 5, 6]
    assert check_closest(dev["ctx"], poses[::-1].copy(), 4, (6,)).tolist() == [2, 3, 5, 6, 0, 1]
    m = poses_map(dev["ctx"], poses)
    for kf, n in ((-1, 1), (7, 1), (0, 0), (0, -2)):
        assert m.ClosestKeyFrames(kf, n, check=False) == E_ARG
    m.close()
    one = poses_map(dev["ctx"], poses[:1])                                           # a map of one keyframe has no other
    assert len(one.ClosestKeyFrames(0, 3)[0]) == 0
    one.close()


def test_closest_keyframes_are_the_recent_bundle_s_choice(dev):
    """ptam_rmap_bundle_adjust(RECENT) adjusts the newest keyframe and those of its four nearest that are not fixed: the same four"""
    K = 12
    h = with_ba_tables(*R.map_from_problem(synth.make_ba_problem(K, 600, 6, window=6), seed=6, extra_fixed=(6, 4)))
    m = host.ResidentMap(dev["ctx"])
    m.upload(**{k: h[k] for k in UPLOAD_KEYS})
    idx, dist = m.ClosestKeyFrames(K - 1, 4)
    assert idx.tolist() == I.closest_keyframes_np(h["poses"], K - 1, 4)[0].tolist() and (np.diff(dist) >= 0).all()
    got = m.bundle_adjust(_abi.MAP_BA_RECENT, deterministic=1)
    assert got["ran"] == 1
    assert got["cam_kf"][:got["n_adjust"]].tolist() == sorted([K - 1] + [int(k) for k in idx if not h["fixed"][k]])
    m.close()


# ---- 4. the busy list's boundaries -------------------------------------------------------------------------------------------------------
def padded(h, n_points):
    """h with copies of its first points appended (measured by no keyframe) up to n_points"""
    N = len(h["points3"])
    take = np.arange(n_points - N) % N
    out = dict(h)
    for k in ("points3", "points", "sources", "bad", "outlier_count", "inlier_count"):
        out[k] = np.concatenate([h[k], h[k][take]])
    return out


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 1025])
def test_busy_list_boundaries(dev, n_rows):
    """skip_refind: the keyframe's run is its n_rows rows.  The thinning, and everything after it, is the host-busy call's."""
    ctx, rng = dev["ctx"], np.random.default_rng(n_rows)
    h = padded(dev["h"], 1100)
    rows = np.zeros(n_rows, host.MAP_KF_ROW_DT)
    rows["point"], rows["level"] = np.arange(n_rows), rng.integers(0, 4, n_rows)
    rows["root_pos"] = rng.uniform((20.0, 20.0), (620.0, 460.0), (n_rows, 2))
    res, tab, _, m, rf = one_call(dev, h=h, rows=rows, skip_refind=True)
    _, stats = host.MapMaker(ctx).AddSomeMapPoints(dev["ka"], dev["sp"], dev["kfs"][I.TARGET], h["poses"][I.TARGET], epi_opts(ctx), busy_level=rows["level"],
                                                   busy_root=rows["root_pos"])
    assert res["levels"].tobytes() == stats.tobytes(), (res["levels"], stats)
    assert res["n_made"] == int(stats["made"].sum()) and res["refind"]["n_pairs"] == 0
    want, wtab, wm, wrf = composed(dev, h=h, rows=rows, skip_refind=True)
    same_result(res, want)
    same_tables(tab, wtab)
    close_all(m, rf, wm, wrf)


# ---- 5. the options ----------------------------------------------------------------------------------------------------------------------------
def test_flat_target_makes_no_point(dev):
    """the target (and the decoy) without a corner: only the keyframe and the re-find show, the new queue stays"""
    kb = host.KeyFrame(dev["ctx"]).MakeKeyFrame_Lite(I.views(True)["ib"])
    kfs = [kb, kb, dev["kfs"][I.THIRD]]
    res, tab, _, m, rf = one_call(dev, kfs=kfs)
    want, wtab, wm, wrf = composed(dev, kfs=kfs, skip_points=True)
    assert res["n_made"] == 0 and res["target_kf"] == I.TARGET and int(res["levels"]["candidates"].sum()) > 0
    assert res["refind"]["n_found"] > 0 and res["refind"] == want["refind"]
    same_tables(tab, wtab)
    assert tab["new_queue"].tobytes() == dev["h"]["new_queue"].tobytes() and len(tab["points3"]) == len(dev["h"]["points3"])
    close_all(m, rf, wm, wrf, kb)


def test_skip_points_is_add_keyframe_and_refind(dev):
    res, tab, traffic, m, rf = one_call(dev, skip_points=True)
    want, wtab, wm, wrf = composed(dev, skip_points=True)
    same_result(res, want)
    same_tables(tab, wtab)
    assert res["target_kf"] == -1 and res["n_made"] == 0 and traffic[1] == 16
    close_all(m, rf, wm, wrf)


def test_explicit_target(dev, pair):
    res, tab, _, m, rf = one_call(dev, target_kf=I.THIRD)
    want, wtab, wm, wrf = composed(dev, target_kf=I.THIRD)
    same_result(res, want)
    same_tables(tab, wtab)
    assert res["target_kf"] == I.THIRD and np.float64(res["target_dist"]).tobytes() == np.float64(want["target_dist"]).tobytes()
    assert tab["meas"].tobytes() != pair[0][1]["meas"].tobytes()
    close_all(m, rf, wm, wrf)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_map_as_it_was(dev):
    ctx, h, rows, ka, sp = dev["ctx"], dev["h"], dev["rows"], dev["ka"], dev["sp"]
    N = len(h["points3"])
    m = uploaded(ctx, h, dev["kfs"])
    rf = host.ReFinder(ctx)
    before, counts = m.tables(), m.counts()

    def refused(status, kf=ka, rows=rows, finder=rf, on=m, was=before, **opts):
        o = on.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH, **opts)
        assert on.InsertKeyFrame(finder, kf, sp, 0, rows, o, check=False) == status, (status, opts)
        same_tables(on.tables(), was)

    swapped = rows.copy()
    swapped[[20, 21]] = swapped[[21, 20]]
    twice, far, level = rows.copy(), rows.copy(), rows.copy()
    twice[8] = twice[7]
    far["point"][-1] = N
    level["level"][3] = 4
    for bad_rows in (swapped, twice, far, level):
        refused(E_ARG, rows=bad_rows)
    for t in (K0, K0 + 1, -2):                                                       # K0 is the new keyframe's own index
        refused(E_ARG, target_kf=t)
    refused(E_ARG, kf=None)
    lite = host.KeyFrame(ctx).MakeKeyFrame_Lite(I.views()["ia"])                     # no MakeKeyFrame_Rest
    refused(E_STATE, kf=lite)
    o = m.insert_opts(levels=(3, 3), **I.DEPTH)
    assert m.InsertKeyFrame(rf, ka, sp, 0, rows, o, check=False) == E_ARG
    assert m.lib.rmap_insert_keyframe(m.h, None, ka.h, host._pd(np.array(sp)), 0, 0, None, host.C.byref(o), host.C.byref(_abi.RmapInsertResult())) == E_ARG
    same_tables(m.tables(), before)
    assert m.counts() == counts
    # a map whose keyframes came without handles; an empty map
    bare = host.ResidentMap(ctx)
    bare.upload(**{k: h[k] for k in UPLOAD_KEYS})
    refused(E_ARG, on=bare, was=before)
    empty = host.ResidentMap(ctx)
    refused(E_STATE, on=empty, was=empty.tables(), rows=rows[:0])
    assert empty.counts()["n_kf"] == 0
    # the same call with valid input is taken
    res = m.InsertKeyFrame(rf, ka, sp, 0, rows, m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH))
    assert res["kf"] == K0 and m.counts()["n_kf"] == K0 + 1
    close_all(m, rf, bare, empty, lite)


# ---- 7. growth ------------------------------------------------------------------------------------------------------------------------------------
def test_growth_gives_the_same_tables(dev, pair):
    h = dev["h"]
    c = dict(n_kf=K0, n_points=len(h["points3"]), n_meas=len(h["meas"]), n_never=len(h["never"]), n_new=len(h["new_queue"]), n_failure=len(h["failure"]))
    tight = one_call(dev, reserve={k: v + 1 for k, v in c.items()})
    roomy = one_call(dev, reserve={k: 8 * v + 4096 for k, v in c.items()})
    same_tables(tight[1], roomy[1])
    same_tables(tight[1], pair[0][1])
    assert tight[0]["levels"].tobytes() == roomy[0]["levels"].tobytes() and tight[0]["n_made"] == pair[0][0]["n_made"]
    check_invariants(tight[1])
    close_all(tight[3], tight[4], roomy[3], roomy[4])


# ---- 8. traffic -----------------------------------------------------------------------------------------------------------------------------------
def test_traffic_is_the_arguments_and_the_count_words(dev, pair):
    (res, _, (up, down), _, _), _ = pair
    rows = dev["rows"]
    # up: the pose and flag, the rows, one level record per keyframe for the re-find; down: the count and stats words
    assert 96 + 1 + rows.nbytes < up <= 96 + 1 + rows.nbytes + _abi.RMAP_KF_RECORD_BYTES * (K0 + 1) + 4, up
    assert down == DOWN_BYTES, down
    # threshold 70 on the same rows: more candidates, more made points, the same bytes
    low = one_call(dev, thr=70.0)
    assert int(low[0]["levels"]["candidates"].sum()) > int(res["levels"]["candidates"].sum()) and low[0]["n_made"] > res["n_made"]
    assert low[2] == (up, down), (low[2], up, down)
    close_all(low[3], low[4])
