"""-m gpu: CalcPlaneAligner, ApplyGlobalTransformationToMap and RefreshSceneDepth on the device (ptam_calc_plane_aligner,
ptam_map_apply_global_transform, ptam_map_align_to_plane, ptam_map_scene_depth) against their numpy restatement
(tests/plane_ref.py).  Every parity fixture is first checked on the restatement alone (guards): no discrete decision — the winning
trial, an inlier flag, the eigenvector taken, the normal's sign, the row-0 test — is near enough to its threshold for rounding to
flip it.  Then the discrete results are compared exactly and the continuous ones under TOL."""
import ctypes as C
import functools

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import plane_ref as PR

pytestmark = pytest.mark.gpu
MAX_DIST = 0.05
# Device against restatement, relative (max |a - b| / max |b| per quantity; the test prints every figure).  The device sums in tree
# order (per thread with stride 256, lanes, waves), the restatement sequentially, and the eigenvector is Jacobi's against LAPACK's.
# Measured on an MI355X over the cases below and the shim's map (docs/LOG_mapmaker.md, "Plane aligner", has every quantity): score
# <= 5.1e-15, mean, normal, eigenvalues, R, t <= 5.9e-16, poses and points <= 1.5e-15, depth mean <= 1.3e-15; the pixel vectors
# <= 9.43e-14 (the largest: pixel_down_w of n10_one_trial) and the depth sigma <= 8.8e-14 are differences of nearly equal numbers
# (two rays 0.002 apart; sum z^2 / n - mean^2), which lose three digits on both sides.  The tolerance is ten times the largest
# figure, the margin the homography test uses for rounding that varies with the fixture.  Far below 1e-6, the project's bundle
# tolerance: nothing to explain.
TOL = 9.5e-13

# name -> (points, map seed, keyframes, outlier fraction, draw seed, trials).  10 with one trial: the smallest map that is scored; 64
# and 65: a wave's edge; 257: one past a workgroup, the stride loop's tail; 2 000: several strides, 30 % outliers, 100 trials.
# skipped_pair and origin_on_mean are built in _case.  The seeds were picked on the CPU so that the guards hold.
CASES = {
    "n10_one_trial": (10, 3, 1, 0.0, 0, 1),
    "n64": (64, 0, 2, 0.25, 1, 100),
    "n65": (65, 1, 2, 0.25, 1, 100),
    "n257": (257, 0, 5, 0.3, 2, 100),
    "n2000": (2000, 0, 2, 0.3, 3, 100),
    "skipped_pair": (70, 2, 2, 0.2, 4, 20),
    "origin_on_mean": (36, 5, 2, 0.0, 0, 1),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(points, poses, sources, meas, sample table, the restatement's results): computed once, shared, never modified"""
    n, seed, n_kf, frac, draw, trials = CASES[name]
    points, poses, sources, meas, _ = PR.make_map(n, seed, n_kf, frac)
    table = PR.samples(draw, n, trials)
    if name == "skipped_pair":
        points[[3, 4, 5]] = points[3]                                    # coincident under distinct indices
        points[[6, 7, 8]] = [[0.5, 0.25, 1.0], [1.0, 0.5, 2.0], [1.5, 0.75, 3.0]]   # collinear: the cross product is exactly 0
        table[2], table[7] = [3, 4, 5], [6, 7, 8]
    if name == "origin_on_mean":    # 0.33333333 * (A + B + C) is exactly (0, 0, 0), and so is the fourth point: dDistSq == 0.0
        rng = np.random.default_rng(seed)
        points[:, :2] = rng.uniform(-1.0, 1.0, (n, 2))
        points[:, 2] = rng.uniform(-0.02, 0.02, n)
        points[30:, 2] = rng.uniform(0.1, 1.0, n - 30)
        points[:4] = [[1.0, 0.0, 0.0], [-0.5, 1.0, 0.0], [-0.5, -1.0, 0.0], [0.0, 0.0, 0.0]]
        table = np.array([[0, 1, 2]], np.int32)
        poses[:, 11] += 2.0                                              # the cameras two units off the plane
    r = PR.calc_plane_aligner(points, table, MAX_DIST)
    moved = PR.apply_global_transform(r["se3"], poses, points, sources)
    depth = PR.scene_depth(moved[0], moved[1], meas)
    for a in (points, poses, sources, meas, table):
        a.setflags(write=False)
    return points, poses, sources, meas, table, (r, moved, depth)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def ctx(hip):
    c = host.Context(lib=hip, size=(160, 128))
    yield c
    c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_guards(name):
    """conditions on the inputs, on the restatement alone"""
    points, _, _, _, table, (r, _, _) = _case(name)
    g = PR.guards(points, table, dict(max_dist=MAX_DIST))
    print(name, r["status"], r["best_trial"], r["n_inliers"], r["trials_skipped"], g)
    assert r["status"] == PR.OK
    assert g["score_gap"] >= 1e-6 and g["threshold_gap"] >= 1e-9 and g["eigen_gap"] >= 1e-3
    assert g["normal_z"] >= 1e-3 and g["one_minus_normal_x"] >= 1e-3
    assert r["trials_skipped"] == (2 if name == "skipped_pair" else 0)
    if name == "origin_on_mean":
        assert np.isnan(r["dists"][3]) and not r["inliers"][3] and r["inliers"][:3].all() and r["n_inliers"] == 29
    if CASES[name][3] > 0:
        assert 0.6 * len(points) <= r["n_inliers"] < len(points)         # the plane is found, the far points are rejected


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_restatement(ctx, name):
    points, poses, sources, meas, table, (r, (poses_r, points_r, (right_r, down_r)), depth_r) = _case(name)
    d = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, samples=table)
    info = d["info"]
    assert info["status"] == r["status"] == _abi.PLANE_OK and info["n_points"] == len(points)
    assert info["best_trial"] == r["best_trial"] and info["trials_skipped"] == r["trials_skipped"]
    assert info["n_inliers"] == r["n_inliers"] and np.array_equal(d["inliers"], r["inliers"])
    depth = host.map_scene_depth(ctx, d["poses"], d["points"], meas)
    assert np.array_equal(depth["n_meas"], depth_r[:, 2])
    figures = dict(score=_rel(info["best_score"], r["best_score"]), mean=_rel(info["mean"], r["mean"]),
                   normal=_rel(info["normal"], r["normal"]), eigenvalues=_rel(info["eigenvalues"], r["eigenvalues"]),
                   R=_rel(d["se3"][:9], r["se3"][:9]), t=_rel(d["se3"][9:], r["se3"][9:]), poses=_rel(d["poses"], poses_r),
                   points=_rel(d["points"], points_r), world=_rel(d["pvs"]["world"], points_r),
                   right=_rel(d["pvs"]["pixel_right_w"], right_r), down=_rel(d["pvs"]["pixel_down_w"], down_r),
                   depth_mean=_rel(depth["depth_mean"], depth_r[:, 0]), depth_sigma=_rel(depth["depth_sigma"], depth_r[:, 1]))
    print(name, {k: "%.2e" % v for k, v in figures.items()})
    assert max(figures.values()) <= TOL, figures                        # TOL: see above
    assert np.array_equal(d["pvs"]["world"], d["points"])


@pytest.mark.parametrize("name", list(CASES))
def test_one_call_equals_the_two_calls(ctx, name):
    points, poses, sources, _, table, _ = _case(name)
    d = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, samples=table)
    se3, info, inl = host.calc_plane_aligner(ctx, points, MAX_DIST, samples=table)
    poses2, points2, pvs2 = host.map_apply_global_transform(ctx, se3, poses, points, sources)
    assert d["se3"].tobytes() == se3.tobytes() and np.array_equal(d["inliers"], inl)
    assert all(np.array_equal(np.asarray(d["info"][k]), np.asarray(info[k])) for k in info)
    assert d["poses"].tobytes() == poses2.tobytes() and d["points"].tobytes() == points2.tobytes() and d["pvs"].tobytes() == pvs2.tobytes()
    poses3, points3, none = host.map_apply_global_transform(ctx, se3, poses, points)    # without a source table
    assert none is None and poses3.tobytes() == poses2.tobytes() and points3.tobytes() == points2.tobytes()


@pytest.mark.parametrize("name", ["n65", "n257", "n2000"])
def test_two_calls_give_the_same_bits(ctx, name):
    points, poses, sources, meas, table, _ = _case(name)
    a = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, samples=table)
    b = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, samples=table)
    for k in ("se3", "inliers", "poses", "points", "pvs"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(np.array_equal(np.asarray(a["info"][k]), np.asarray(b["info"][k])) for k in a["info"])
    da, db = (host.map_scene_depth(ctx, x["poses"], x["points"], meas) for x in (a, b))
    assert da.tobytes() == db.tobytes()


def test_seed_draws_the_exported_table(hip, ctx):
    points = _case("n64")[0]
    a = host.calc_plane_aligner(ctx, points, MAX_DIST, seed=11)
    b = host.calc_plane_aligner(ctx, points, MAX_DIST, samples=host.plane_samples(hip, 11, len(points), 100))
    assert a[1]["status"] == _abi.PLANE_OK and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[2], b[2])
    assert a[1]["best_trial"] == b[1]["best_trial"] and a[1]["best_score"] == b[1]["best_score"]


def test_too_few_points_apply_the_identity(ctx):
    """nine points: the reference returns SE3<>() and applies it; the tables stay, the pixel vectors are still refreshed"""
    points, poses, sources, _, _ = PR.make_map(9, 0, 2, 0.0)
    d = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, seed=1)
    assert d["info"]["status"] == _abi.PLANE_TOO_FEW and d["info"]["n_points"] == 9 and d["info"]["best_trial"] == -1
    assert np.array_equal(d["se3"], PR.IDENTITY) and not d["inliers"].any()
    assert d["poses"].tobytes() == poses.tobytes() and d["points"].tobytes() == points.tobytes()
    right, down = PR.pixel_vectors(poses, points, sources)
    assert np.array_equal(d["pvs"]["world"], points)
    assert _rel(d["pvs"]["pixel_right_w"], right) <= TOL and _rel(d["pvs"]["pixel_down_w"], down) <= TOL
    se3, info, inl = host.calc_plane_aligner(ctx, points, MAX_DIST, seed=1)
    assert info["status"] == _abi.PLANE_TOO_FEW and np.array_equal(se3, PR.IDENTITY) and not inl.any()


def test_all_trials_skipped_leaves_the_tables(ctx):
    points, poses, sources, _, _ = PR.make_map(40, 0, 2)
    points[[3, 4, 5]] = points[3]
    table = np.tile(np.array([3, 4, 5], np.int32), (6, 1))
    assert PR.calc_plane_aligner(points, table, MAX_DIST)["status"] == PR.DEGENERATE
    d = host.map_align_to_plane(ctx, poses, points, sources, MAX_DIST, samples=table)
    assert d["info"]["status"] == _abi.PLANE_DEGENERATE and d["info"]["trials_skipped"] == 6 and d["info"]["best_trial"] == -1
    assert d["info"]["n_inliers"] == 0 and not d["inliers"].any() and np.array_equal(d["se3"], PR.IDENTITY)
    assert d["poses"].tobytes() == poses.tobytes() and d["points"].tobytes() == points.tobytes()
    assert not d["pvs"].tobytes().strip(b"\0")                           # (the wrapper's zeros: nothing was written)


def test_scene_depth_segments(ctx):
    """keyframes with 0, 1, 3, 64, 65 and 300 rows in one table"""
    points, poses, _, _, _ = PR.make_map(300, 7, 6)
    counts = (0, 1, 3, 64, 65, 300)
    rng = np.random.default_rng(0)
    rows = [(k, p) for k, c in enumerate(counts) for p in sorted(rng.permutation(300)[:c].tolist())]
    meas = np.zeros(len(rows), host.MAP_MEAS_DT)
    meas["kf"], meas["point"] = np.array(rows, np.int32).T
    ref = PR.scene_depth(poses, points, meas)
    d = host.map_scene_depth(ctx, poses, points, meas)
    assert d["n_meas"].tolist() == list(counts) and (d["pad_"] == 0).all()
    assert (d["depth_mean"][0], d["depth_sigma"][0]) == (0.0, 0.0) and d["depth_sigma"][1] == 0.0
    figures = dict(mean=_rel(d["depth_mean"], ref[:, 0]), sigma=_rel(d["depth_sigma"], ref[:, 1]))
    print(figures)
    assert max(figures.values()) <= TOL
    none = host.map_scene_depth(ctx, poses, points, meas[:0])
    assert not none.tobytes().strip(b"\0")


def test_refusals(hip, ctx):
    points, poses, sources, meas, table, _ = _case("n64")
    points, poses, table = points.copy(), poses.copy(), table.copy()
    n, K = len(points), len(poses)
    se3, info, inl = np.full(12, 7.0), _abi.PlaneInfo(), np.full(n, 0x5a, np.uint8)
    C.memset(C.byref(info), 0x5a, C.sizeof(info))
    out = np.zeros(n, host.PVS_POINT_DT)
    out.view(np.uint8)[:] = 0x5a
    depth = np.zeros(K, host.SCENE_DEPTH_DT)
    depth.view(np.uint8)[:] = 0x5a
    before = [a.tobytes() for a in (se3, inl, out, depth, points, poses)] + [bytes(info)]

    def untouched():
        return [a.tobytes() for a in (se3, inl, out, depth, points, poses)] + [bytes(info)] == before

    def opts(**kw):
        o = _abi.PlaneOpts()
        hip.plane_opts_default(C.byref(o))
        assert (o.max_dist, o.trials, o.seed, bool(o.samples)) == (0.05, 100, 0, False)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad_tables():
        for kw in (dict(trials=0), dict(trials=-3), dict(max_dist=0.0), dict(max_dist=-1.0)):
            yield opts(**kw)
        for row, col, value in ((0, 0, n), (99, 2, -1), (50, 1, None)):  # an index outside [0, n), one repeated in its triple
            t = table.copy()
            t[row, col] = t[row, 0 if col else 2] if value is None else value
            o = opts(samples=t.ctypes.data_as(C.POINTER(C.c_int32)))
            o._keep = t
            yield o

    p = host._ptr
    calc = [ctx.h, n, p(points), C.byref(opts()), host._pd(se3), C.byref(info), p(inl)]
    for i in (0, 2, 3, 4, 5):                                            # a null pointer
        bad = list(calc)
        bad[i] = None
        assert hip.calc_plane_aligner(*bad) == -1 and untouched(), i
    bad = list(calc)
    bad[1] = -1
    assert hip.calc_plane_aligner(*bad) == -1 and untouched()
    align = [ctx.h, C.byref(opts()), K, p(poses), n, p(points), p(sources), p(out), host._pd(se3), C.byref(info), p(inl)]
    for o in bad_tables():
        bad = list(calc)
        bad[3] = C.byref(o)
        assert hip.calc_plane_aligner(*bad) == -1 and untouched()
        bad = list(align)
        bad[1] = C.byref(o)
        assert hip.map_align_to_plane(*bad) == -1 and untouched()
    apply = [ctx.h, host._pd(PR.IDENTITY.copy()), K, p(poses), n, p(points), p(sources), p(out)]
    src_bad = [sources.copy(), sources.copy()]
    src_bad[0]["src_kf"][n - 1], src_bad[1]["src_kf"][0] = K, -1
    for i, v in [(0, None), (1, None), (3, None), (5, None), (6, None), (7, None), (2, -1), (4, -1)] + [(6, p(s)) for s in src_bad]:
        bad = list(apply)                                                # null tables, one of sources / out alone, src_kf out of range
        bad[i] = v
        assert hip.map_apply_global_transform(*bad) == -1 and untouched(), i
    for i, v in [(0, None), (1, None), (3, None), (5, None), (6, None), (7, None), (8, None), (9, None)] + [(6, p(s)) for s in src_bad]:
        bad = list(align)
        bad[i] = v
        assert hip.map_align_to_plane(*bad) == -1 and untouched(), i
    M = len(meas)
    dep = [ctx.h, K, p(poses), n, p(points), M, p(meas), p(depth)]
    swapped, repeated, far_kf, far_point = (meas.copy() for _ in range(4))
    swapped[[10, 11]] = swapped[[11, 10]]
    repeated[11] = repeated[10]
    far_kf["kf"][M - 1] = K
    far_point["point"][5] = n
    for i, v in [(0, None), (2, None), (4, None), (6, None), (7, None), (1, -1), (3, -1), (5, -1)] + [(6, p(t)) for t in (swapped, repeated, far_kf, far_point)]:
        bad = list(dep)
        bad[i] = v
        assert hip.map_scene_depth(*bad) == -1 and untouched(), i
    assert hip.map_align_to_plane(*align) == 0 and info.status == _abi.PLANE_OK and not untouched()   # the context still works
    assert hip.map_scene_depth(*dep) == 0 and (depth["n_meas"] > 0).all()
