"""-m gpu: the resident TrackMap chain (ptam_track_map, src/Tracker.cc:442-696) against the same frame composed stage by
stage through the CPU oracle (tests/trackmap_ref.py): pose, mbDidCoarse, per-level attempted / found counts, the sets'
sizes, every entry of vIterationSet (point, level, found, sub-pixel flag, v2Found, outlier flag) and the scene-depth sums."""
import numpy as np
import pytest

from ptam_cg_amd import host, synth
from tests import trackmap_ref

pytestmark = pytest.mark.gpu


def _setup(lib, counts, **case_kw):
    ctx = host.Context(lib=lib)
    a, b = synth.make_frame_pair()
    kfa = host.KeyFrame(ctx).MakeKeyFrame_Lite(a)
    kfb = host.KeyFrame(ctx).MakeKeyFrame_Lite(b)
    case = synth.make_trackmap_case([kfa.level(l) for l in range(4)], counts=counts, **case_kw)
    return ctx, kfa, kfb, case


def _run_hip(hip, counts, opts_kw, **case_kw):
    ctx, kfa, kfb, case = _setup(hip, counts, **case_kw)
    tr = host.Tracker(ctx, len(case["world"]) + 7)
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
    res = tr.TrackMap(kfb, case["pose_in"], tr.opts(**opts_kw))
    it = tr.iteration_set()
    res2 = tr.TrackMap(kfb, case["pose_in"], tr.opts(**opts_kw))     # the resident state must not leak into the next frame
    assert np.array_equal(res["pose"], res2["pose"]) and res["n_meas"] == res2["n_meas"]
    tr.close()
    return res, it, case


def _run_ref(oracle, counts, opts_kw, pvs_lib=None, **case_kw):
    ctx, kfa, kfb, case = _setup(oracle, counts, **case_kw)
    pvs_ctx = host.Context(lib=pvs_lib) if pvs_lib is not None else None
    return trackmap_ref.track_map(ctx, kfb, kfa, case, case["pose_in"], case["shuffle_levels"], case["shuffle_fine"], pvs_ctx=pvs_ctx, **opts_kw)


CASES = {
    # coarse stage counts (60 coarse points, > 20 found), fine set chopped to MaxPatchesPerFrame
    "coarse_and_chop": (dict(counts=(800, 300, 80, 40)), dict()),
    # few top-level points: level 3 alone does not fill CoarseMax -> the :538 assignment path (level-2 list replaces it)
    "coarse_from_level2": (dict(counts=(300, 120, 30, 25)), dict()),
    # level 2 larger than the remainder: level-3 picks + part of level 2
    "coarse_mixed": (dict(counts=(200, 100, 90, 25)), dict()),
    # coarse stage disabled by the caller's heuristics: fine range 10, no re-projection
    "no_coarse": (dict(counts=(400, 200, 60, 30)), dict(try_coarse=0)),
    # too few coarse points in the PVS (<= CoarseMin): no coarse search at all
    "too_few_coarse": (dict(counts=(300, 100, 10, 6)), dict()),
    # coarse search runs but finds fewer than CoarseMin (prediction far off): mbDidCoarse stays false
    "coarse_fails": (dict(counts=(300, 100, 40, 30), pose_noise=(0.08, 0.05)), dict()),
    # more top-level points than the coarse set takes: the remainder is searched with sub-pixel refinement in the fine stage
    "top_level_remainder": (dict(counts=(300, 100, 30, 40)), dict(coarse_max=20, coarse_min=10)),
    # smaller patch budget than the sets: the fine set is chopped to zero
    "tiny_budget": (dict(counts=(200, 100, 50, 30)), dict(max_patches=40)),
}


def _check(res, it, ref, strict):
    assert bool(res["did_coarse"]) == ref["did_coarse"]
    assert list(res["n_pvs"]) == ref["n_pvs"]
    assert (res["n_coarse"], res["n_top"], res["n_fine"]) == (ref["n_coarse"], ref["n_top"], ref["n_fine"])
    assert list(res["attempted"]) == ref["attempted"] and list(res["found"]) == ref["found"]
    assert res["n_meas"] == ref["n_meas"]
    rit = ref["iteration_set"]
    assert len(it) == len(rit)
    for k in ("point", "level", "found", "did_subpix", "outlier"):
        assert np.array_equal(it[k], rit[k]), k
    f = it["found"] == 1
    dv = np.abs(it["v2_found"][f] - rit["v2_found"][f]).max(1) if f.any() else np.zeros(0)
    sub = it["did_subpix"][f] == 1
    assert (dv[~sub] <= 1e-9).all()                     # coarse positions: corner coordinates, exact
    if strict:
        # product vs product: to the bit.  Oracle stages on the device's warp matrices: 1e-6 px / 1e-9 — seven of the eight
        # cases agree to 6e-14 px; in "coarse_fails" (prediction far off, ten marginal matches) one sub-pixel iteration that
        # barely converges ends 2.6e-7 px apart
        assert (dv <= (1e-9 if strict is True else 1e-6)).all()
        assert np.allclose(res["pose"], ref["pose"], rtol=0, atol=1e-10 if strict is True else 1e-9)
        if strict == "oracle":
            print("chain vs oracle stages on the device's warp matrices: max |dv| %.2e px over %d found patches, max |dpose| %.2e"
                  % (dv.max() if dv.size else 0.0, dv.size, np.abs(res["pose"] - ref["pose"]).max()))
    else:
        # CVD::transform truncates the interpolated value to a byte (src/PatchFinder.cc:116): a last-bit difference of the PVS warp
        # matrix can flip one grey level of a warped template, which moves that patch's sub-pixel fit by up to ~0.1 px (found /
        # not found, levels, outlier flags are unaffected).  Rounds 2-3: ~1 % of the templates (the device's PVS had its a * b +
        # c * d fused into FMAs, the oracle's compiler emits none), 5 % of the positions allowed here and 2e-5 on the pose.  Round
        # 4: pvs_device.h computes uncontracted — what is left is the device's atan against glibc's: ONE template in the
        # eight scenarios (0.026 px, pose 2.6e-6), every other position within 3e-7 px
        assert (dv <= 0.3).all() and (dv > 1e-6).sum() <= max(2, int(0.005 * dv.size))
        assert np.allclose(res["pose"], ref["pose"], rtol=0, atol=5e-6)
    assert res["depth_n"] == ref["depth"][2]
    tol = 1e-12 if strict is True else (1e-9 if strict else 1e-5)
    assert np.isclose(res["depth_sum"], ref["depth"][0], rtol=tol) and np.isclose(res["depth_sum_sq"], ref["depth"][1], rtol=tol)


@pytest.mark.parametrize("name", list(CASES))
def test_track_map_matches_composed_oracle(hip, oracle, name):
    case_kw, opts_kw = dict(CASES[name][0]), CASES[name][1]
    counts = case_kw.pop("counts")
    res, it, case = _run_hip(hip, counts, opts_kw, **case_kw)
    _check(res, it, _run_ref(oracle, counts, opts_kw, **case_kw), strict=False)
    # the allowance above exists only because the two libraries' warp matrices differ in the last bit
    # (device atan / FMA vs glibc) and CVD::transform truncates to bytes.  With the PVS pass of the device handed to the oracle
    # composition — every other stage the oracle's — the chain must match EXACTLY: every sub-pixel position, the pose to 1e-10
    _check(res, it, _run_ref(oracle, counts, opts_kw, pvs_lib=hip, **case_kw), strict="oracle")
    # the same composition through the product's own per-stage entry points: identical arithmetic, so the chain's control
    # flow, list order and TrackerData hand-over between the stages must reproduce it to the last bit of the pose
    _check(res, it, _run_ref(hip, counts, opts_kw, **case_kw), strict=True)
    # the frame did something: most searched patches were found, and the pose moved towards the truth
    if name not in ("coarse_fails", "tiny_budget"):
        assert res["n_meas"] > 0.5 * len(it)
        err_in = np.abs(case["pose_in"] - case["cur_pose"]).max()
        err_out = np.abs(res["pose"] - case["cur_pose"]).max()
        assert err_out < err_in


def test_track_map_degenerate_maps(hip):
    """an empty map, a map none of whose points is visible, and a map of two points: the chain must return the prediction
    unchanged (CalcPoseUpdate of an empty set is a zero update, src/Tracker.cc:955-956) and empty sets, not hang or fault"""
    ctx, kfa, kfb, case = _setup(hip, (40, 20, 10, 5))
    tr = host.Tracker(ctx, 64)
    pose = case["pose_in"]
    # empty
    tr.set_map(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), kfa, np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    r = tr.TrackMap(kfb, pose)
    assert np.array_equal(r["pose"], pose) and r["n_meas"] == 0 and list(r["n_pvs"]) == [0, 0, 0, 0] and len(tr.iteration_set()) == 0
    # nothing visible: every point behind the camera
    w = case["world"][:30].copy()
    w[:, 2] += 50.0
    tr.set_map(w, case["pixel_right_w"][:30], case["pixel_down_w"][:30], kfa, case["src_level"][:30], case["center"][:30])
    r = tr.TrackMap(kfb, pose)
    assert np.array_equal(r["pose"], pose) and r["n_meas"] == 0 and sum(r["n_pvs"]) == 0
    # two points
    tr.set_map(case["world"][:2], case["pixel_right_w"][:2], case["pixel_down_w"][:2], kfa, case["src_level"][:2], case["center"][:2])
    tr.set_shuffle(np.array([1, 0], np.int32), np.array([0, 1], np.int32))
    r = tr.TrackMap(kfb, pose)
    assert np.isfinite(r["pose"]).all() and r["n_meas"] <= 2 and len(tr.iteration_set()) == sum(r["n_pvs"])
    tr.close()


def test_track_frame_equals_keyframe_then_track_map(hip):
    """ptam_track_map_frame (keyframe of the new image + TrackMap, one call) == MakeKeyFrame_Lite followed by
    ptam_track_map, bit for bit — also when the keyframe object is re-used frame after frame with different images"""
    ctx, kfa, kfb, case = _setup(hip, (800, 300, 80, 40))
    a, b = synth.make_frame_pair()
    frames = [b, a, b, np.roll(b, 2, axis=1), b]
    tr = host.Tracker(ctx, len(case["world"]))
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    want = []
    for im in frames:
        kf = host.KeyFrame(ctx).MakeKeyFrame_Lite(im)
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        r = tr.TrackMap(kf, case["pose_in"])
        want.append((r.copy(), tr.iteration_set().copy(), [kf.level(l)["corners"].copy() for l in range(4)]))
    kfc = host.KeyFrame(ctx)
    bufs = [host.DevBuf(ctx, im) for im in frames]
    got = []
    # (the same history on both sides: set_map starts every point's PatchFinder afresh)
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    for d in bufs:                                  # back to back, no synchronisation of the caller's in between
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        r = tr.TrackFrame(kfc, d, case["pose_in"])
        got.append((r.copy(), tr.iteration_set().copy(), [kfc.level(l)["corners"].copy() for l in range(4)]))
    for (r0, it0, c0), (r1, it1, c1) in zip(want, got):
        assert r0.tobytes() == r1.tobytes()
        assert it0.tobytes() == it1.tobytes()
        for x, y in zip(c0, c1):
            assert np.array_equal(x, y)
    assert want[0][0]["n_meas"] != want[1][0]["n_meas"] or not np.array_equal(want[0][0]["pose"], want[1][0]["pose"])
    tr.close()


def test_native_replicas_track_the_same_frame(hip):
    """ptam_bench_track_frames: k contexts driven by k host threads inside the library (per frame set_shuffle +
    ptam_track_map_frame) leave every tracker with the pose a single ptam_track_map_frame call gives — the permutations
    travel through host-mapped memory on this path (maps of at most 8192 points), so a non-trivial shuffle is part of it."""
    import ctypes as C
    ctx0 = host.Context(lib=hip)
    a, b = synth.make_frame_pair()
    kfa0 = host.KeyFrame(ctx0).MakeKeyFrame_Lite(a)
    case = synth.make_trackmap_case([kfa0.level(l) for l in range(4)], counts=(400, 200, 60, 30))
    ws = []
    for _ in range(3):
        cx = host.Context(lib=hip)
        ka = host.KeyFrame(cx).MakeKeyFrame_Lite(a)
        tr = host.Tracker(cx, len(case["world"]))
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], ka, case["src_level"], case["center"])
        ws.append((cx, ka, host.KeyFrame(cx), tr, host.DevBuf(cx, b)))
    cx, ka, kb, tr, di = ws[0]
    opts = tr.opts()
    tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
    want = tr.TrackFrame(kb, di, case["pose_in"], opts)
    # the same frame with the identity shuffle picks other sets: the permutations do arrive
    ident = np.arange(len(case["world"]), dtype=np.int32)
    tr.set_shuffle(ident, ident)
    other = tr.TrackFrame(kb, di, case["pose_in"], opts)
    assert not np.array_equal(other["pose"], want["pose"]) or other["n_meas"] != want["n_meas"]
    raw = lambda h: h.value if hasattr(h, "value") else int(h)
    k = len(ws)
    trs = (C.c_void_p * k)(*[raw(w[3].h) for w in ws])
    kfs = (C.c_void_p * k)(*[raw(w[2].h) for w in ws])
    dis = (C.c_void_p * k)(*[raw(w[4].p) for w in ws])
    sl = np.ascontiguousarray(case["shuffle_levels"], dtype=np.int32)
    sf = np.ascontiguousarray(case["shuffle_fine"], dtype=np.int32)
    pose = np.ascontiguousarray(case["pose_in"], dtype=np.float64)
    secs = C.c_double()
    ctx0._check(hip.bench_track_frames(k, trs, kfs, dis, pose.ctypes.data_as(C.POINTER(C.c_double)), opts.ctypes.data_as(C.c_void_p),
                                       sl.ctypes.data_as(C.c_void_p), sf.ctypes.data_as(C.c_void_p), 5, C.byref(secs)), "bench_track_frames")
    assert secs.value > 0
    for cx, ka, kb, tr, di in ws:
        # the trackers' last frame == the single call (the resident state does not leak from frame to frame)
        again = tr.TrackFrame(kb, di, case["pose_in"], opts)   # (shuffle as the native driver left it)
        assert np.array_equal(again["pose"], want["pose"]) and again["n_meas"] == want["n_meas"]
        tr.close()


def test_batch_of_frames_equals_single_calls(hip):
    """ptam_track_map_frames_batch: nb trackers with DIFFERENT maps, frames and predictions in one chain of launches give, frame
    by frame, exactly what ptam_track_map_frame gives (same kernel bodies; maps of equal size pick the same pose-kernel
    instantiations) — pose, counts, depth sums and the iteration sets."""
    import ctypes as C
    a, b = synth.make_frame_pair()
    ctx0 = host.Context(lib=hip)
    kfa0 = host.KeyFrame(ctx0).MakeKeyFrame_Lite(a)
    ws = []
    for i in range(4):
        case = synth.make_trackmap_case([kfa0.level(l) for l in range(4)], counts=(400, 200, 60, 30), seed=100 + i)
        cx = host.Context(lib=hip)
        ka = host.KeyFrame(cx).MakeKeyFrame_Lite(a)
        tr = host.Tracker(cx, len(case["world"]))
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], ka, case["src_level"], case["center"])
        frame = b if i % 2 == 0 else np.ascontiguousarray(b[::-1, ::-1])   # two of the frames show another image
        ws.append((cx, ka, host.KeyFrame(cx), tr, host.DevBuf(cx, frame), case))
    opts = ws[0][3].opts()
    single, sets = [], []
    for cx, ka, kb, tr, di, case in ws:
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        single.append(tr.TrackFrame(kb, di, case["pose_in"], opts).copy())
        sets.append(tr.iteration_set())
    raw = lambda h: h.value if hasattr(h, "value") else int(h)
    k = len(ws)
    trs = (C.c_void_p * k)(*[raw(w[3].h) for w in ws])
    kfs = (C.c_void_p * k)(*[raw(w[2].h) for w in ws])
    dis = (C.c_void_p * k)(*[raw(w[4].p) for w in ws])
    poses = np.ascontiguousarray(np.stack([np.asarray(w[5]["pose_in"], dtype=np.float64).reshape(12) for w in ws]))
    res = np.zeros(k, dtype=host.TRACKMAP_RESULT_DT)
    for rep in range(2):   # (twice: what the trackers keep between frames — the PatchFinders' templates: same prediction, so every
                           #  one of them is kept — must not change the outcome)
        for cx, ka, kb, tr, di, case in ws:
            tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        ctx0._check(hip.track_map_frames_batch(k, trs, kfs, dis, poses.ctypes.data_as(C.POINTER(C.c_double)), opts.ctypes.data_as(C.c_void_p),
                                               res.ctypes.data_as(C.c_void_p)), "track_map_frames_batch")
        for i, (cx, ka, kb, tr, di, case) in enumerate(ws):
            for f in res.dtype.names:
                if f == "templates_reused":
                    assert res[i][f] == sum(res[i]["attempted"]) + (res[i]["n_coarse"] + res[i]["n_top"] + res[i]["n_fine"] - sum(res[i]["attempted"]))
                    continue
                assert np.array_equal(res[i][f], single[i][f]), (rep, i, f, res[i][f], single[i][f])
            it = tr.iteration_set()
            assert it.tobytes() == sets[i].tobytes(), (rep, i)
    assert single[0]["n_meas"] > 100 and not np.array_equal(single[0]["pose"], single[1]["pose"])
    for cx, ka, kb, tr, di, case in ws:
        tr.close()


@pytest.mark.parametrize("size", [(640, 480), (322, 243), (163, 121)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_keyframes_and_degenerate_maps(hip, size):
    """the batch's keyframe kernels (tall-tile FAST detection: aligned-word staging at widths that are multiples of four, the
    byte path otherwise) leave every keyframe exactly as MakeKeyFrame_Lite does — images, corners, row LUTs of all four
    levels — and frames whose map is empty or invisible come back with the prediction, beside a frame that tracks"""
    w, h = size
    a, b = synth.make_frame_pair()
    rng = np.random.default_rng(7)
    ims = [np.ascontiguousarray(a[:h, :w]), np.ascontiguousarray(b[:h, :w]), rng.integers(0, 256, (h, w)).astype(np.uint8)]
    ws = []
    for im in ims:
        cx = host.Context(lib=hip, size=size)
        tr = host.Tracker(cx, 32)
        ka = host.KeyFrame(cx).MakeKeyFrame_Lite(ims[0])
        tr.set_map(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), ka, np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
        ws.append((cx, ka, host.KeyFrame(cx), tr, host.DevBuf(cx, im)))
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    res = host.Tracker.TrackFramesBatch([x[3] for x in ws], [x[2] for x in ws], [x[4] for x in ws], [pose] * len(ws), ws[0][3].opts())
    for (cx, ka, kb, tr, di), im, r in zip(ws, ims, res):
        assert np.array_equal(r["pose"], pose) and r["n_meas"] == 0
        want = host.KeyFrame(cx).MakeKeyFrame_Lite(im)
        for l in range(4):
            g, q = kb.level(l), want.level(l)
            assert np.array_equal(g["im"], q["im"]) and np.array_equal(g["corners"], q["corners"]) and np.array_equal(g["rowlut"], q["rowlut"]), (size, l)
        assert len(kb.level(0)["corners"]) > 0
        tr.close()


def test_stage_profiling_counts_frames_and_leaves_the_result_alone(hip):
    """ptam_tracker_set_profiling / ptam_tracker_stage_time: the events of a profiled frame change nothing in its result — the same
    frame from the same pose with profiling off, on, off again, bit for bit — and the stage times cover exactly the frames profiled
    since the last switch.  163x121 with the empty map of test_batch_keyframes_and_degenerate_maps: the suite's smallest frame chain."""
    import ctypes as C
    from ptam_cg_amd import _abi
    size = (163, 121)
    a, _ = synth.make_frame_pair()
    im = np.ascontiguousarray(a[:size[1], :size[0]])
    cx = host.Context(lib=hip, size=size)
    tr = host.Tracker(cx, 32)
    ka = host.KeyFrame(cx).MakeKeyFrame_Lite(im)
    tr.set_map(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), ka, np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    kb, di = host.KeyFrame(cx), host.DevBuf(cx, im)
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    opts = tr.opts()

    def frames_profiled():
        got = set()
        for i in range(len(_abi.TRACK_STAGE_NAMES)):
            ms, n = C.c_double(), C.c_int()
            cx._check(hip.tracker_stage_time(tr.h, i, C.byref(ms), C.byref(n)), "tracker_stage_time")
            got.add(n.value)
        assert len(got) == 1   # every stage reports the same count
        return got.pop()

    off = tr.TrackFrame(kb, di, pose, opts).copy()
    assert frames_profiled() == 0
    tr.set_profiling(True)
    on = tr.TrackFrame(kb, di, pose, opts).copy()
    assert frames_profiled() == 1
    times = tr.stage_times()
    tr.set_profiling(False)   # (every switch starts the sums again)
    off_again = tr.TrackFrame(kb, di, pose, opts).copy()
    assert frames_profiled() == 0
    assert off.tobytes() == on.tobytes() == off_again.tobytes()
    assert np.array_equal(off["pose"], pose) and off["n_meas"] == 0
    assert list(times) == list(_abi.TRACK_STAGE_NAMES)
    vals = np.array(list(times.values()))
    assert np.isfinite(vals).all() and (vals >= 0).all() and vals.sum() > 0
    tr.close()


@pytest.mark.parametrize("variant", ["R", "T"])
@pytest.mark.parametrize("size", [(640, 480), (608, 407), (322, 243), (163, 121), (96, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_track_frame_keyframe_is_make_keyframe_lite(hip, size, variant):
    """the tracked frame's own keyframe launch (pyramid pixels computed inside the FAST tiles: one word per thread at widths that
    are multiples of 32, pixel by pixel otherwise) leaves the keyframe exactly as MakeKeyFrame_Lite does — images, corners, row
    LUTs of all four levels, in both halfSample roundings"""
    from ptam_cg_amd import _abi
    w, h = size
    a, b = synth.make_frame_pair()
    rng = np.random.default_rng(11)
    ims = [np.ascontiguousarray(b[:h, :w]), rng.integers(0, 256, (h, w)).astype(np.uint8), np.ascontiguousarray(a[h // 7:h // 7 + h, 5:5 + w]) if h * 8 // 7 <= a.shape[0] and w + 5 <= a.shape[1] else np.ascontiguousarray(a[:h, :w])]
    cx = host.Context(lib=hip, size=size, halfsample=_abi.HALFSAMPLE_R if variant == "R" else _abi.HALFSAMPLE_T)
    tr = host.Tracker(cx, 32)
    ka = host.KeyFrame(cx).MakeKeyFrame_Lite(ims[0])
    tr.set_map(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), ka, np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    kb = host.KeyFrame(cx)
    for im in ims:
        r = tr.TrackFrame(kb, host.DevBuf(cx, im), pose)
        assert np.array_equal(r["pose"], pose) and r["n_meas"] == 0
        want = host.KeyFrame(cx).MakeKeyFrame_Lite(im)
        for l in range(4):
            g, q = kb.level(l), want.level(l)
            assert np.array_equal(g["im"], q["im"]) and np.array_equal(g["corners"], q["corners"]) and np.array_equal(g["rowlut"], q["rowlut"]), (size, l)
    assert len(kb.level(0)["corners"]) > 0
    tr.close()


def test_batch_with_maps_of_different_sizes(hip):
    """a batch whose maps differ in size: grids are sized for the largest, every frame works on its own counts; the pose
    kernels run in the instantiation the LARGEST list capacity selects, so a small map's sums are taken in another order
    than in its single call — same sets, counts and flags, poses equal to rounding"""
    a, b = synth.make_frame_pair()
    ctx0 = host.Context(lib=hip)
    kfa0 = host.KeyFrame(ctx0).MakeKeyFrame_Lite(a)
    ws = []
    for i, counts in enumerate([(800, 300, 80, 40), (80, 40, 20, 10), (300, 120, 30, 25)]):
        case = synth.make_trackmap_case([kfa0.level(l) for l in range(4)], counts=counts, seed=200 + i)
        cx = host.Context(lib=hip)
        ka = host.KeyFrame(cx).MakeKeyFrame_Lite(a)
        tr = host.Tracker(cx, len(case["world"]) + 3 * i)
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], ka, case["src_level"], case["center"])
        ws.append((cx, ka, host.KeyFrame(cx), tr, host.DevBuf(cx, b), case))
    opts = ws[0][3].opts()
    single, sets = [], []
    for cx, ka, kb, tr, di, case in ws:
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        single.append(tr.TrackFrame(kb, di, case["pose_in"], opts).copy())
        sets.append(tr.iteration_set())
    for cx, ka, kb, tr, di, case in ws:
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
    res = host.Tracker.TrackFramesBatch([w[3] for w in ws], [w[2] for w in ws], [w[4] for w in ws], [w[5]["pose_in"] for w in ws], opts)
    assert len({len(w[5]["world"]) for w in ws}) == 3
    for i, (cx, ka, kb, tr, di, case) in enumerate(ws):
        for f in res.dtype.names:
            if f in ("pose", "depth_sum", "depth_sum_sq"):
                assert np.allclose(res[i][f], single[i][f], rtol=1e-9, atol=1e-9), (i, f)
            elif f == "templates_reused":     # (the single calls above made the templates, the batch keeps every one of them)
                assert single[i][f] == 0 and res[i][f] == len(sets[i])
            else:
                assert np.array_equal(res[i][f], single[i][f]), (i, f, res[i][f], single[i][f])
        it = tr.iteration_set()
        for f in ("point", "level", "found", "did_subpix", "outlier"):
            assert np.array_equal(it[f], sets[i][f]), (i, f)
        assert np.allclose(it["v2_found"], sets[i]["v2_found"], rtol=0, atol=1e-9)
        assert single[i]["n_meas"] > 20
        tr.close()


@pytest.mark.parametrize("counts", [(900, 500, 300, 200), (1000, 900, 700, 500)], ids=lambda c: f"{sum(c)}pts")
def test_batch_equals_single_call_on_maps_of_two_thousand_points(hip, counts):
    """maps beyond the fused pose kernels' 1 024 slots take the gather pass and the small / general pose kernel pair in a batch:
    the searches must give the single call's positions to the bit, the pose its pose to rounding.  (The PVS body inlined into
    the batch's kernel and into the single frame's had fused different products of the warp matrix: last-bit differences, one
    grey level in 3-6 of ~1 000 warped templates, sub-pixel fits 0.01 px and one corner apart — pvs_device.h now computes
    uncontracted.)  Also with a patch budget above the kernels' limit (the general pose kernel on both sides)."""
    a, b = synth.make_frame_pair()
    ctx = host.Context(lib=hip)
    ka = host.KeyFrame(ctx).MakeKeyFrame_Lite(a)
    case = synth.make_trackmap_case([ka.level(l) for l in range(4)], counts=counts, seed=300)
    tr = host.Tracker(ctx, len(case["world"]))
    kb, di = host.KeyFrame(ctx), host.DevBuf(ctx, b)

    def fresh():   # (the same history on both sides: set_map starts every point's PatchFinder afresh)
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], ka, case["src_level"], case["center"])
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])

    for budget in (1000, 2000):
        opts = tr.opts(max_patches=budget)
        fresh()
        single = tr.TrackFrame(kb, di, case["pose_in"], opts).copy()
        its = tr.iteration_set().copy()
        fresh()
        res = host.Tracker.TrackFramesBatch([tr], [kb], [di], [case["pose_in"]], opts)[0]
        itb = tr.iteration_set()
        for f in its.dtype.names:
            assert np.array_equal(its[f], itb[f]), (budget, f)
        for f in res.dtype.names:
            if f in ("pose", "depth_sum", "depth_sum_sq"):
                assert np.allclose(res[f], single[f], rtol=1e-12, atol=1e-12), (budget, f)
            else:
                assert np.array_equal(res[f], single[f]), (budget, f)
        assert single["n_meas"] > (900 if budget == 1000 else 1024)
    tr.close()


@pytest.mark.parametrize("tile", [1, 4], ids=["2561pts_lds_lists", "10244pts_global_lists"])
def test_track_map_large_maps(hip, tile):
    """maps beyond the one- and two-entries-per-thread runs of the set choice: 2 561 points (LDS level lists, three entries per
    thread, host-mapped permutations) and the same map four times over = 10 244 points (more than the LDS lists hold: global
    lists, device permutations, runs reloaded inside the loops) against the composition through the product's own stage calls —
    the chain's control flow, list order and hand-over must reproduce it to the last bit"""
    ctx, kfa, kfb, case = _setup(hip, (1000, 900, 700, 500))
    if tile > 1:
        rng = np.random.default_rng(5)
        for k in ("world", "pixel_right_w", "pixel_down_w", "src_level", "center"):
            case[k] = np.concatenate([case[k]] * tile)
        n = len(case["world"])
        case["shuffle_levels"] = rng.permutation(n).astype(np.int32)
        case["shuffle_fine"] = rng.permutation(n).astype(np.int32)
    n = len(case["world"])
    assert (n > 8192) == (tile > 1) and n > 2048
    tr = host.Tracker(ctx, n)
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
    res = tr.TrackMap(kfb, case["pose_in"], tr.opts())
    it = tr.iteration_set()
    tr.close()
    ref = trackmap_ref.track_map(ctx, kfb, kfa, case, case["pose_in"], case["shuffle_levels"], case["shuffle_fine"])
    _check(res, it, ref, strict=True)
    assert res["n_meas"] > 500 and sum(res["n_pvs"]) > 2400 * tile


def test_tracker_and_mapmaker_threads_run_side_by_side(hip):
    """the reference's two-thread loop: a tracker thread tracking frames while the mapmaker thread runs a bundle adjustment, each in
    its own context on the same device — both get exactly what they get when run one after the other"""
    import threading
    from tests import util
    ctx_t, kfa, kfb, case = _setup(hip, (800, 300, 80, 40))
    a, b = synth.make_frame_pair()
    tr = host.Tracker(ctx_t, len(case["world"]))
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    d_im = host.DevBuf(ctx_t, b)
    kf_cur = host.KeyFrame(ctx_t)
    opts = tr.opts()

    def track(n):
        out = []
        for _ in range(n):
            tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
            out.append(tr.TrackFrame(kf_cur, d_im, case["pose_in"], opts).copy())
        return out

    prob = synth.make_ba_problem(20, 3000, 5)
    want_track = track(3)
    want_ba = util.run_ba(hip, prob)
    got = {}
    th = [threading.Thread(target=lambda: got.__setitem__("track", track(60))),
          threading.Thread(target=lambda: got.__setitem__("ba", [util.run_ba(hip, prob) for _ in range(3)]))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert len(got["track"]) == 60 and len(got["ba"]) == 3
    for r in got["track"]:
        assert np.array_equal(r["pose"], want_track[0]["pose"]) and r["n_meas"] == want_track[0]["n_meas"]
    for r in got["ba"]:
        util.assert_ba_equal(r, want_ba, rel=1e-9)
        assert np.array_equal(r["outliers"], want_ba["outliers"])
    tr.close()


def test_trackmap_options_out_of_range_are_refused(hip):
    """coarse_max is an unsigned option that becomes an int on the device; 2^31 made the set sizes negative and the
    set choice write outside its lists.  Every out-of-range option must come back as an argument error, nothing enqueued."""
    ctx, kfa, kfb, case = _setup(hip, (60, 30, 20, 10))
    tr = host.Tracker(ctx, len(case["world"]))
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    good = tr.TrackMap(kfb, case["pose_in"], tr.opts())
    for bad in (dict(coarse_max=2 ** 31), dict(coarse_max=2 ** 32 - 1), dict(coarse_min=2 ** 31 + 5), dict(coarse_range=10 ** 6),
                dict(estimator=7), dict(estimator=-1), dict(max_patches=-1), dict(coarse_subpix_its=65)):
        with pytest.raises(RuntimeError, match="bad argument"):
            tr.TrackMap(kfb, case["pose_in"], tr.opts(**bad))
    again = tr.TrackMap(kfb, case["pose_in"], tr.opts())      # and the tracker is still usable
    assert np.array_equal(good["pose"], again["pose"])
    tr.close()


def _moved(pose, rot_z=0.0, dz=0.0, dx=0.0):
    """pose (R row-major | t) left-multiplied by a small motion: rotation about the optical axis, translation along x / z"""
    R, t = np.asarray(pose[:9], dtype=np.float64).reshape(3, 3), np.asarray(pose[9:], dtype=np.float64)
    c, s = np.cos(rot_z), np.sin(rot_z)
    M = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([(M @ R).ravel(), M @ t + np.array([dx, 0.0, dz])])


def test_track_map_keeps_patchfinder_state_between_frames(hip, oracle):
    """ADVICE r2 (medium) / src/PatchFinder.cc:98-127: a point's PatchFinder keeps its search template — and mbTemplateBad —
    while neither column of the warp moves by more than 0.07, and a warp rejected by CalcSearchLevelAndWarpMatrix leaves
    mbTemplateBad up until the next re-make (:78-81).  One tracker follows five predictions on the same image: the
    prediction, nearly the same one (templates kept), a camera pushed towards the scene (many warps rejected, many re-made),
    back again (kept templates with a stale mbTemplateBad), and far off.  Frame by frame the chain must equal the composed
    oracle that carries the same per-point state."""
    ctx, kfa, kfb, case = _setup(hip, (400, 200, 70, 40))
    octx, okfa, okfb, _ = _setup(oracle, (400, 200, 70, 40))
    tr = host.Tracker(ctx, len(case["world"]))
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    p0 = case["pose_in"]
    z = float(np.median(case["world"] @ p0[6:9] + p0[11]))     # a typical depth
    poses = [p0, _moved(p0, rot_z=2e-4, dx=1e-4 * z), _moved(p0, dz=-0.45 * z), _moved(p0, rot_z=2e-4, dx=1e-4 * z), _moved(p0, rot_z=0.12)]
    finders = {}
    reused, stale = [], []
    for k, pose in enumerate(poses):
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        res = tr.TrackMap(kfb, pose, tr.opts())
        it = tr.iteration_set()
        ref = trackmap_ref.track_map(octx, okfb, okfa, case, pose, case["shuffle_levels"], case["shuffle_fine"], finders=finders)
        _check(res, it, ref, strict=False)
        assert res["templates_reused"] == ref["templates_reused"], (k, res["templates_reused"], ref["templates_reused"])
        reused.append(int(res["templates_reused"]))
        stale.append(ref["stale_bad"])
    searched = len(it)
    print("templates reused per frame", reused, "of", searched, "| kept with a stale mbTemplateBad", stale)
    assert reused[0] == 0                       # a fresh tracker warps every template
    assert reused[1] > 0.8 * searched           # nearly the same prediction: nearly every finder keeps its template
    assert reused[2] < reused[1]                # the pushed-in camera changes the warps
    assert reused[3] > 0 and reused[4] < reused[1]
    # a new map starts every finder afresh
    tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
    tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
    assert tr.TrackMap(kfb, p0, tr.opts())["templates_reused"] == 0
    tr.close()


def test_track_map_chain_against_oracle_twin_over_frames(hip, oracle):
    """the chain (ptam_track_map_frame: keyframe of the new image + TrackMap) against the oracle's twin of the same entry point
    (ptamo_track_map_frame, C++), six frames of one tracker each: alternating images, predictions that wander, the
    PatchFinders' state carried along on both sides"""
    a, b = synth.make_frame_pair()
    frames = [b, b, np.roll(b, 1, axis=1), b, a, b]
    runs = {}
    for name, lib in (("hip", hip), ("oracle", oracle)):
        ctx = host.Context(lib=lib)
        kfa = host.KeyFrame(ctx).MakeKeyFrame_Lite(a)
        case = synth.make_trackmap_case([kfa.level(l) for l in range(4)], counts=(500, 250, 80, 40))
        tr = host.Tracker(ctx, len(case["world"]))
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
        kf = host.KeyFrame(ctx)
        out = []
        pose = np.array(case["pose_in"], dtype=np.float64)
        for k, im in enumerate(frames):
            tr.set_shuffle(np.roll(case["shuffle_levels"], 7 * k), np.roll(case["shuffle_fine"], 3 * k))
            fr = host.DevBuf(ctx, im) if name == "hip" else None
            res = tr.TrackFrame(kf, fr if fr is not None else np.ascontiguousarray(im).ctypes.data, pose, tr.opts())
            out.append((res, tr.iteration_set()))
            if fr is not None:
                fr.free()
            pose = _moved(case["pose_in"], rot_z=1e-4 * (k + 1), dx=2e-5 * (k + 1))   # (the same predictions on both sides)
        runs[name] = out
        tr.close()
    for k, ((rh, ih), (ro, io)) in enumerate(zip(runs["hip"], runs["oracle"])):
        ref = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": io}
        _check(rh, ih, ref, strict=False)
        assert rh["templates_reused"] == ro["templates_reused"], k
    assert runs["oracle"][1][0]["templates_reused"] > 0 and runs["oracle"][0][0]["n_meas"] > 300


def _copy_model(m):
    from ptam_cg_amd import _abi
    import ctypes as C
    c = _abi.MotionModel()
    C.memmove(C.byref(c), C.byref(m), C.sizeof(m))
    return c


def test_moving_camera_sequence_against_oracle_twin(hip, oracle):
    """a camera that MOVES (synth.make_tracking_frames: 48 distinct rendered frames of a trajectory that
    translates, rises, rolls and tilts) tracked as Tracker::TrackFrame does it — keyframe of the new image, motion-model
    prediction, bTryCoarse from the velocity, TrackMap, motion-model update (src/Tracker.cc:94,134-137,1013-1056).
    (i) frame by frame, product and oracle twin start from the SAME model state (the oracle's closed-loop one) and must agree
    like every other chain test: discrete outcome exactly, poses / sub-pixel positions within the documented allowance, the
    number of kept templates exactly; (ii) the product's own closed loop stays on the true trajectory and beside the oracle's;
    (iii) the native driver (ptam_bench_track_sequence) reproduces the closed loop bit for bit."""
    frames, poses, kim, kpose = synth.make_tracking_frames(48)
    sides = {}
    for name, lib in (("hip", hip), ("oracle", oracle)):
        ctx = host.Context(lib=lib)
        kf0 = host.KeyFrame(ctx).MakeKeyFrame_Lite(kim)
        m = synth.make_sequence_map([kf0.level(l) for l in range(4)], kpose)
        tr = host.Tracker(ctx, len(m["world"]))
        tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], kf0, m["src_level"], m["center"])
        sides[name] = (ctx, kf0, m, tr, host.KeyFrame(ctx))
    ctx_h, _, m, tr_h, kf_h = sides["hip"]
    _, _, mo, tr_o, kf_o = sides["oracle"]
    for k in ("world", "src_level", "center"):
        assert np.array_equal(m[k], mo[k])                       # bit-exact keyframes -> the same map on both sides
    d_frames = [host.DevBuf(ctx_h, f) for f in frames]
    opts = tr_h.opts()
    mm_o = tr_o.motion_model(poses[0])
    reused = searched = coarse = 0
    closed_o = []
    for k in range(len(frames)):
        mm_h = _copy_model(mm_o)                                  # the same prediction and heuristics on both sides
        tr_o.set_shuffle(np.roll(m["shuffle_levels"], 5 * k), np.roll(m["shuffle_fine"], 11 * k))
        tr_h.set_shuffle(np.roll(m["shuffle_levels"], 5 * k), np.roll(m["shuffle_fine"], 11 * k))
        ro = tr_o.TrackFrameMoving(kf_o, frames[k].ctypes.data, mm_o, tr_o.opts())
        io = tr_o.iteration_set()
        rh = tr_h.TrackFrameMoving(kf_h, d_frames[k], mm_h, opts)
        ih = tr_h.iteration_set()
        ref = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": io}
        _check(rh, ih, ref, strict=False)
        assert rh["templates_reused"] == ro["templates_reused"], k
        # the models after the frame: same start pose, velocity = ln of poses that agree to 2e-5
        assert np.array_equal(np.array(mm_h.start_pose), np.array(mm_o.start_pose))
        assert np.allclose(np.array(mm_h.velocity), np.array(mm_o.velocity), rtol=0, atol=5e-5)
        assert np.isclose(mm_h.scene_depth_mean, mm_o.scene_depth_mean, rtol=1e-5)
        assert np.abs(ro["pose"] - poses[k]).max() < 3e-3, k
        n = int(ro["n_coarse"] + ro["n_top"] + ro["n_fine"])
        if k:
            reused, searched, coarse = reused + int(ro["templates_reused"]), searched + n, coarse + int(ro["did_coarse"])
        closed_o.append(ro["pose"].copy())
    print("moving camera: %d of %d searched templates kept (%.0f %%), coarse stage on %d of %d frames"
          % (reused, searched, 100.0 * reused / searched, coarse, len(frames) - 1))
    assert 0.3 * searched < reused < 0.95 * searched and coarse >= len(frames) - 3
    # (ii) the product's own closed loop
    tr_h.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], sides["hip"][1], m["src_level"], m["center"])
    mm = tr_h.motion_model(poses[0])
    closed_h = []
    for k in range(len(frames)):
        tr_h.set_shuffle(m["shuffle_levels"], m["shuffle_fine"])
        r = tr_h.TrackFrameMoving(kf_h, d_frames[k], mm, opts)
        assert np.abs(r["pose"] - poses[k]).max() < 3e-3 and r["n_meas"] > 600, k
        closed_h.append(r["pose"].copy())
    # (the two loops use different shuffles and round differently: they meet within the tracking noise, not to the bit)
    assert np.abs(np.array(closed_h) - np.array(closed_o)).max() < 2e-3
    # (iii) the native driver: the same closed loop from one C++ host thread
    tr_h.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], sides["hip"][1], m["src_level"], m["center"])
    mm2 = tr_h.motion_model(poses[0])
    secs, st = tr_h.track_sequence_native(kf_h, d_frames, mm2, opts, m["shuffle_levels"], m["shuffle_fine"], passes=1, poses_true=poses)
    assert secs > 0 and st["frames"] == len(frames) and st["frames_below_50_measurements"] == 0
    assert np.array_equal(np.array(mm2.pose), closed_h[-1]) and np.array_equal(np.array(mm2.velocity), np.array(mm.velocity))
    assert 0 < st["templates_reused"] < st["searched"] and st["max_position_error_m"] < 5e-3
    for d in d_frames:
        d.free()
    tr_h.close()
    tr_o.close()


def test_update_map_keeps_the_finders_of_persisting_points(hip, oracle):
    """ptam_tracker_set_map starts every PatchFinder afresh, but the reference's TrackerData lives as long as its
    MapPoint while the mapmaker adds and removes other points.  ptam_tracker_update_map carries the finders of the points that
    persist (re-ordered) and gives new points fresh ones: product against the oracle's twin, two frames before and one after
    the change; and set_map on the same tracker still resets them all."""
    runs = {}
    for name, lib in (("hip", hip), ("oracle", oracle)):
        ctx, kfa, kfb, case = _setup(lib, (300, 150, 60, 30))
        n = len(case["world"])
        tr = host.Tracker(ctx, n + 5)
        tr.set_map(case["world"], case["pixel_right_w"], case["pixel_down_w"], kfa, case["src_level"], case["center"])
        out = []
        tr.set_shuffle(case["shuffle_levels"], case["shuffle_fine"])
        out.append((tr.TrackMap(kfb, case["pose_in"], tr.opts()).copy(), tr.iteration_set()))
        rng = np.random.default_rng(3)
        perm = rng.permutation(n)
        keep, fresh = perm[: 2 * n // 3], perm[2 * n // 3:]
        order = np.concatenate([keep, fresh])
        prev = np.concatenate([keep, np.full(len(fresh), -1)]).astype(np.int32)
        c2 = {k: case[k][order] for k in ("world", "pixel_right_w", "pixel_down_w", "src_level", "center")}
        sl, sf = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
        tr.update_map(c2["world"], c2["pixel_right_w"], c2["pixel_down_w"], kfa, c2["src_level"], c2["center"], prev)
        p1 = _moved(case["pose_in"], rot_z=2e-4, dx=1e-4)
        tr.set_shuffle(sl, sf)
        out.append((tr.TrackMap(kfb, p1, tr.opts()).copy(), tr.iteration_set()))
        with pytest.raises(RuntimeError):        # an old index used twice is refused, the tracker keeps its map
            tr.update_map(c2["world"], c2["pixel_right_w"], c2["pixel_down_w"], kfa, c2["src_level"], c2["center"], np.zeros(n, np.int32))
        tr.set_map(c2["world"], c2["pixel_right_w"], c2["pixel_down_w"], kfa, c2["src_level"], c2["center"])
        tr.set_shuffle(sl, sf)
        out.append((tr.TrackMap(kfb, p1, tr.opts()).copy(), tr.iteration_set()))
        runs[name] = out
        tr.close()
    for k, ((rh, ih), (ro, io)) in enumerate(zip(runs["hip"], runs["oracle"])):
        ref = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": io}
        _check(rh, ih, ref, strict=False)
        assert rh["templates_reused"] == ro["templates_reused"], k
    searched = len(runs["hip"][1][1])
    assert runs["hip"][0][0]["templates_reused"] == 0 and runs["hip"][2][0]["templates_reused"] == 0
    assert 0.3 * searched < runs["hip"][1][0]["templates_reused"] < 0.9 * searched
