"""-m gpu: ptam_track_frames_batch — Tracker::TrackFrame's tracking branch for a batch of cameras in one chain of launches, with the
motion model, the bTryCoarse heuristics per camera and the SmallBlurryImage rotation estimator on the device — against single-call
twins built from the public pieces.  The alignment is the single call's body (exact); the predicted pose is made by the device's
twin of ptam_motion_predict_sbi (tolerance-class: TOL_PREDICT) and handed back in info.pose_in, which makes everything behind it
exact again: the result is ptam_track_map_frame from info.pose_in, byte for byte."""
import ctypes as C

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import sbi_cases as SC
from tests import sbi_ref as S
from tests.test_gpu_sbi import TOL_ALIGN
from tests.test_gpu_trackmap import _check, _copy_model

pytestmark = pytest.mark.gpu

# The device's prediction against the host's ptam_motion_predict_sbi, max |delta| / max(1, |t|) over the 64-row table of
# test_device_prediction_against_the_host_function, measured on an MI355X: 5.13e-16 (docs/LOG_sbi.md, "Batch").  Ten times that, the
# margin the other tolerances of that log use.  The work is a handful of ulps (asin or acos, a square root, sin and cos of the
# exponential, a 3x4 product): a figure above 1e-13 would be a bug of the twin, not rounding.
TOL_PREDICT = 5.13e-15


def _predict_error(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(want, np.float64).reshape(-1, 12)
    return np.abs(got - want).max(1) / np.maximum(1.0, np.linalg.norm(want[:, 9:], axis=1))


def _prediction_table():
    """-> (models, rotations (n, 9), labels): rotations exp(w) over every range of SO3::ln — identity, tiny, the estimator's 0.1 rad,
    either side of pi/4 and 3 pi/4, and pi - 1e-3 / pi - 1e-7 with the axis led by x, y and z, each with both signs (the three axis
    choices and both outcomes of the r2 . w test)"""
    rng = np.random.default_rng(20)
    unit = lambda v: np.asarray(v, np.float64) / np.linalg.norm(v)
    ws, labels = [], []
    mags = [1e-9, 1e-3, 0.1, np.pi / 4 - 1e-6, np.pi / 4 + 1e-6, 3 * np.pi / 4 - 1e-6, 3 * np.pi / 4 + 1e-6]
    for mag in mags:
        for _ in range(7):
            ws.append(mag * unit(rng.normal(size=3)))
            labels.append("%.7g" % mag)
    for mag in (np.pi - 1e-3, np.pi - 1e-7):
        for axis in ((0.8, 0.5, 0.33), (0.4, 0.85, 0.3), (0.3, 0.4, 0.86)):
            for sign in (1.0, -1.0):
                ws.append(mag * sign * unit(axis))
                labels.append("pi-%.0e axis %d sign %+d" % (np.pi - mag, int(np.argmax(axis)), int(sign)))
    for _ in range(3):
        ws.append(np.zeros(3))
        labels.append("identity")
    rots = np.stack([np.eye(3).reshape(9) if not w.any() else S.so3_exp(w).reshape(9) for w in ws])
    models = (_abi.MotionModel * len(ws))()
    for m in models:
        m.velocity[:] = (1e-2 * rng.normal(size=6)).tolist()
        R = S.so3_exp(rng.normal(size=3))
        t = rng.uniform(-10, 10, 3) / np.sqrt(3.0)
        m.pose[:] = np.concatenate([R.reshape(9), t]).tolist()
        m.start_pose[:] = m.pose[:]
    return models, np.ascontiguousarray(rots), labels


def test_device_prediction_against_the_host_function(hip):
    """ptam_motion_predict_sbi_dev (the align workgroup's prediction, one thread per row) against ptam_motion_predict_sbi"""
    ctx = host.Context(lib=hip)
    models, rots, labels = _prediction_table()
    n = len(labels)
    assert 60 <= n <= 70
    before = bytes(models)
    got = np.zeros((n, 12))
    ctx._check(hip.motion_predict_sbi_dev(ctx.h, n, models, host._pd(rots), host._pd(got)), "motion_predict_sbi_dev")
    assert bytes(models) == before
    want = np.zeros((n, 12))
    for i in range(n):
        m = _copy_model(models[i])
        hip.motion_predict_sbi(C.byref(m), host._pd(np.ascontiguousarray(rots[i])))
        want[i] = np.array(m.pose)
    err = _predict_error(got, want)
    worst = {}
    for lab, e in zip(labels, err):
        worst[lab] = max(worst.get(lab, 0.0), e)
    print("device prediction against ptam_motion_predict_sbi, max |delta| / max(1, |t|): %.2e over %d rows" % (err.max(), n))
    for lab, e in worst.items():
        print("   |w| = %-28s %.2e" % (lab, e))
    assert np.isfinite(got).all()
    assert err.max() <= 1e-13, "the device twin of the prediction is wrong, not rounded"
    assert err.max() <= TOL_PREDICT
    # the identity: ln is exactly zero, so the step is exp((0, 0, v2, 0, 0, 0)) — its rotation part is exactly the identity, and
    # the pose's rotation comes through to the bit
    for i in [i for i, lab in enumerate(labels) if lab == "identity"]:
        step = np.zeros(12)
        hip.se3_exp(host._ptr(np.array([0, 0, models[i].velocity[2], 0, 0, 0.0])), host._ptr(step))
        assert _predict_error(got[i], synth.se3_mul(step, np.array(models[i].pose)))[0] <= TOL_PREDICT
        assert np.array_equal(got[i][:9], np.array(models[i].pose)[:9])
    ctx.close()


# ---- cameras and their single-call twins ----------------------------------------------------------------------------------------
class Camera:
    """one camera of a batch: its own context with the map's source keyframe, a tracker on the sequence's map (or a subset of it),
    the frames on the device, its keyframe, motion model and rotation estimator — and a twin tracker in the same context that is fed
    the same frames through the single-camera entry points"""

    def __init__(self, hip, estimator=True, subset=None, frames=None, size=(640, 480), empty=False, mapping=None):
        self.lib = hip
        seq_frames, self.poses, kim, kpose = SC.tracking_sequence()
        self.frames = seq_frames if frames is None else frames
        self.ctx = host.Context(lib=hip, size=size)
        w, h = size
        self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(np.ascontiguousarray(kim[:h, :w]))
        if empty:
            z3, zi = np.zeros((0, 3)), np.zeros(0, np.int32)
            self.map = {"world": z3, "pixel_right_w": z3, "pixel_down_w": z3, "src_level": zi, "center": np.zeros((0, 2), np.int32)}
        else:
            m = mapping if mapping is not None else synth.make_sequence_map([self.kf0.level(l) for l in range(4)], kpose)
            self.map = m if subset is None else {k: v[subset(m)] for k, v in m.items() if k not in ("shuffle_levels", "shuffle_fine")}
        self.d_frames = [host.DevBuf(self.ctx, np.ascontiguousarray(f)) for f in self.frames]
        self.tr, self.twin = self._tracker(), self._tracker()
        self.kf, self.kf_twin = host.KeyFrame(self.ctx), host.KeyFrame(self.ctx)
        self.est = host.RotationEstimator(self.ctx, size=size) if estimator else None
        self.sbi = [host.SmallBlurryImage(self.ctx, size=size), host.SmallBlurryImage(self.ctx, size=size)] if estimator else []
        self.last = None
        self.model = self.tr.motion_model(self.poses[0])

    def _tracker(self):
        m = self.map
        tr = host.Tracker(self.ctx, max(len(m["world"]), 32))
        tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], self.kf0, m["src_level"], m["center"])
        return tr

    def reset_estimator(self):
        self.est.reset()
        self.last = None

    def twin_frame(self, k, before, info):
        """frame k through the single-camera pieces, from the model `before` -> (result, alignment or None, opts, model after,
        the host's prediction or None)"""
        lib, ctx = self.lib, self.ctx
        m = _copy_model(before)
        if self.est is None:
            r = self.twin.TrackFrameMoving(self.kf_twin, self.d_frames[k], m, self.twin.opts())   # ptam_track_frame
            return r, None, SC.coarse_opts(self.twin, before), m, None
        o = SC.coarse_opts(self.twin, before)
        ctx._check(lib.make_keyframe_lite_dev(ctx.h, self.kf_twin.h, self.d_frames[k].p), "make_keyframe_lite_dev")
        this = 0 if self.last is None else 1 - self.last
        self.sbi[this].MakeFromKF(self.kf_twin, 0.75)
        al = self.sbi[this].CalcSBIRotation(self.sbi[this if self.last is None else self.last], 6)
        self.last = this
        hostm = _copy_model(before)
        lib.motion_predict_sbi(C.byref(hostm), host._pd(np.ascontiguousarray(al["rotation"].reshape(9))))
        r = self.twin.TrackFrame(self.kf_twin, self.d_frames[k], info["pose_in"], o)              # ptam_track_map_frame
        m.just_recovered = 0
        m.start_pose[:] = m.pose[:]
        m.pose[:] = np.asarray(info["pose_in"]).tolist()
        lib.motion_update(C.byref(m), host._ptr(np.array([r])))
        return r, al, o, m, np.array(hostm.pose)

    def close(self):
        for o in [self.tr, self.twin, self.kf, self.kf_twin, self.kf0] + self.sbi + ([self.est] if self.est else []):
            o.close()
        for d in self.d_frames:
            d.free()
        self.ctx.close()


def _batch(cams, ks, opts=None):
    """one ptam_track_frames_batch over the cameras, camera i on its frame ks[i] -> (results, infos, the models before)"""
    before = [_copy_model(c.model) for c in cams]
    models = [c.model for c in cams]
    res, infos = host.Tracker.track_frames_batch([c.tr for c in cams], [c.kf for c in cams], [c.d_frames[k] for c, k in zip(cams, ks)],
                                                 models, [c.est for c in cams], opts)
    return res, infos, before


def _check_against_twin(cam, k, r, info, before, tag):
    """camera `cam`'s frame k of a batch against its single-call twin: alignment exact, pose_in within TOL_PREDICT of the host's
    prediction, result and model byte for byte, the heuristics as sbi_cases.coarse_opts has them"""
    r2, al2, o, m2, host_pose = cam.twin_frame(k, before, info)
    assert (info["try_coarse"], info["coarse_max"], info["coarse_range"]) == (o["try_coarse"][0], o["coarse_max"][0], o["coarse_range"][0]), tag
    if cam.est is not None:
        al = info["align"]
        assert all(np.array_equal(np.asarray(al[f]), np.asarray(al2[f])) for f in al2), tag
        e = _predict_error(info["pose_in"], host_pose)[0]
        print(tag, "pose_in against the host's prediction: %.2e" % e)
        assert e <= TOL_PREDICT, tag
    else:
        assert not np.asarray(info["align"]["rotation"]).any() and info["align"]["n_used"] == 0, tag
        hostm = _copy_model(before)
        hostm.just_recovered = 0
        cam.lib.motion_predict(C.byref(hostm))
        assert np.array_equal(info["pose_in"], np.array(hostm.pose)), tag
    assert r.tobytes() == r2.tobytes(), (tag, r, r2)
    assert bytes(cam.model) == bytes(m2), tag
    assert cam.tr.iteration_set().tobytes() == cam.twin.iteration_set().tobytes(), tag
    return r2, al2


def test_one_camera_with_estimator_equals_the_single_call_pieces(hip):
    """nb = 1, frames 0-3"""
    cam = Camera(hip)
    for k in range(4):
        res, infos, before = _batch([cam], [k])
        r2, al2 = _check_against_twin(cam, k, res[0], infos[0], before[0], "frame %d" % k)
        assert (k == 0) == np.array_equal(al2["rotation"], np.eye(3))
        assert np.abs(res[0]["pose"] - cam.poses[k]).max() < 3e-3 and res[0]["n_meas"] >= 50, k
    cam.close()


def _subset_300(m):
    """300 points of the map with every point of levels 2 and 3 among them (more than CoarseMax = 60 coarse candidates)"""
    top = np.flatnonzero(m["src_level"] >= 2)
    rest = np.flatnonzero(m["src_level"] < 2)
    return np.sort(np.concatenate([top, rest[:300 - len(top)]]))


@pytest.fixture(scope="module")
def four(hip):
    """A: on frames k.  B: on frames k + 2, its estimator reset before round 0.  C: no estimator (the host predicts).  D: a standing
    model after ptam_motion_recover, on a 300-point subset of the map."""
    cams = [Camera(hip), Camera(hip), Camera(hip, estimator=False), Camera(hip, subset=_subset_300)]
    yield cams
    for c in cams:
        c.close()


def test_mixed_batch_of_four_cameras_over_three_rounds(four):
    A, B, Cc, D = four
    lib = A.lib
    assert len(D.map["world"]) == 300 and len(A.map["world"]) > 1024
    # A and B have moved before (a frame each, tracked alone), so that their models have a velocity; C stands at frame 0's pose
    for cam, k in ((A, 0), (B, 2)):
        cam.model = cam.tr.motion_model(cam.poses[k])
        res, infos, before = _batch([cam], [k])
        _check_against_twin(cam, k, res[0], infos[0], before[0], "warm-up")
    B.reset_estimator()
    Cc.model = Cc.tr.motion_model(Cc.poses[0])
    D.model = D.tr.motion_model(D.poses[3])
    D.model.velocity[:] = [0.1] * 6
    lib.motion_recover(C.byref(D.model), host._pd(np.ascontiguousarray(D.poses[1])))
    assert D.model.just_recovered == 1
    for rnd in range(3):
        ks = [1 + rnd, 3 + rnd, rnd, 1 + rnd]
        res, infos, before = _batch(four, ks)
        for name, cam, k, r, info, b in zip("ABCD", four, ks, res, infos, before):
            _check_against_twin(cam, k, r, info, b, "round %d camera %s" % (rnd, name))
            assert r["n_meas"] >= 50, (rnd, name)
        if rnd == 0:
            assert np.array_equal(infos[1]["align"]["rotation"], np.eye(3)) and infos[1]["align"]["score"] == 0.0     # B: freshly reset
            assert not np.array_equal(infos[0]["align"]["rotation"], np.eye(3))
            # two different coarse decisions in ONE batch: D just recovered (doubled CoarseMax, coarse although it stands), C stands
            assert res[3]["did_coarse"] == 1 and res[3]["n_coarse"] > 60 and infos[3]["coarse_max"] == 120 and infos[3]["coarse_range"] == 60
            assert res[2]["did_coarse"] == 0 and infos[2]["try_coarse"] == 0 and infos[2]["coarse_max"] == 60
            assert D.model.just_recovered == 0


def test_refusals_leave_models_and_estimators_as_they_were(four, hip):
    A, B, Cc, D = four
    ref = Camera(hip)            # runs the same good calls as A, without the refused ones
    for cam in (A, ref):
        cam.model = cam.tr.motion_model(cam.poses[0])
        cam.reset_estimator()
        # (a new history for both: the trackers' finders keep templates from frame to frame)
        for tr in (cam.tr, cam.twin):
            m = cam.map
            tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], cam.kf0, m["src_level"], m["center"])
    B.model = B.tr.motion_model(B.poses[0])
    for k in range(3):
        both = [A, B]
        before = [bytes(c.model) for c in both]
        # options that TrackMap refuses, on ANOTHER frame
        with pytest.raises(host.PtamError):
            _batch(both, [(k + 3) % 8, (k + 4) % 8], A.tr.opts(estimator=7))
        assert [bytes(c.model) for c in both] == before
        # an estimator of another tracker's context; the same estimator twice
        for ests in ([B.est, A.est], [A.est, A.est]):
            res = np.zeros(2, host.TRACKMAP_RESULT_DT)
            raw = lambda h: h.value if hasattr(h, "value") else int(h)
            arr = lambda xs: (C.c_void_p * 2)(*[raw(x) for x in xs])
            mm = (_abi.MotionModel * 2)(A.model, B.model)
            rc = hip.track_frames_batch(2, arr([A.tr.h, B.tr.h]), arr([A.kf.h, B.kf.h]), arr([A.d_frames[k].p, B.d_frames[k].p]), mm,
                                        arr([e.h for e in ests]), None, host._ptr(res), None)
            assert rc == -1 and bytes(mm) == b"".join(before)
        assert [bytes(c.model) for c in both] == before
        ra, ia, _ = _batch([A], [k])
        rr, ir, _ = _batch([ref], [k])
        assert ra.tobytes() == rr.tobytes() and bytes(A.model) == bytes(ref.model), k
        assert all(np.array_equal(np.asarray(ia[0]["align"][f]), np.asarray(ir[0]["align"][f])) for f in ia[0]["align"]), k
        assert np.array_equal(ia[0]["pose_in"], ir[0]["pose_in"])
        assert (k == 0) == np.array_equal(ia[0]["align"]["rotation"], np.eye(3))
    ref.close()


def test_the_smallest_chain(hip):
    """nb = 2 on 163x121 frames with empty maps (a SmallBlurryImage of 10x7), blank frames in slot 1"""
    size = (163, 121)
    seq = SC.tracking_sequence()[0]
    f0 = [np.ascontiguousarray(f[:size[1], :size[0]]) for f in seq[:3]]
    blank = np.full((size[1], size[0]), 128, np.uint8)
    f1 = [blank, blank, f0[0]]      # (blank against itself after the reset, then blank against blank: no gradient on either side)
    cams = [Camera(hip, size=size, empty=True, frames=f0), Camera(hip, size=size, empty=True, frames=f1)]
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    for c in cams:
        c.model = c.tr.motion_model(pose)
        c.model.velocity[:] = [0.002, -0.001, 0.003, 0.001, 0.002, -0.003]
    for k in range(3):
        res, infos, before = _batch(cams, [k, k])
        for i, c in enumerate(cams):
            _check_against_twin(c, k, res[i], infos[i], before[i], "frame %d camera %d" % (k, i))
            assert np.array_equal(res[i]["pose"], infos[i]["pose_in"]) and res[i]["n_meas"] == 0      # an empty map: the prediction
        al = infos[1]["align"]
        assert al["degenerate"] == (1 if k < 2 else 0), k
        assert np.isfinite(al["rotation"]).all() and np.isfinite(infos[1]["pose_in"]).all()
        assert infos[0]["align"]["degenerate"] == 0
    for c in cams:
        c.close()


def test_maps_beyond_the_fused_pose_kernels(hip):
    """nb = 2 on maps of about 2 000 points, one camera just recovered, the other not; also with a patch budget above the fused
    kernels' 1 024 slots — the frame is then finished by the gather pass and the small / general pose kernel pair, as in the
    single call"""
    seq = SC.tracking_sequence()
    ctx0 = host.Context(lib=hip)
    kf0 = host.KeyFrame(ctx0).MakeKeyFrame_Lite(seq[2])
    big = synth.make_sequence_map([kf0.level(l) for l in range(4)], seq[3], counts=(900, 500, 300, 200))
    assert len(big["world"]) > 1900
    cams = [Camera(hip, mapping=big), Camera(hip, mapping=big)]
    for budget in (1000, 2000):
        for c in cams:
            for tr in (c.tr, c.twin):      # (the same history on both sides)
                tr.set_map(big["world"], big["pixel_right_w"], big["pixel_down_w"], c.kf0, big["src_level"], big["center"])
            c.reset_estimator()
        cams[0].model = cams[0].tr.motion_model(cams[0].poses[0])
        cams[1].model = cams[1].tr.motion_model(cams[1].poses[5])
        hip.motion_recover(C.byref(cams[1].model), host._pd(np.ascontiguousarray(cams[1].poses[1])))
        opts = cams[0].tr.opts(max_patches=budget)
        # (the twin's per-frame options carry the budget too)
        orig = [c.twin.opts for c in cams]
        for c in cams:
            c.twin.opts = (lambda tw: (lambda **kw: host.Tracker.opts(tw, max_patches=budget, **kw)))(c.twin)
        for k in range(2):
            res, infos, before = _batch(cams, [k, 1 + k], opts)
            for i, c in enumerate(cams):
                _check_against_twin(c, [k, 1 + k][i], res[i], infos[i], before[i], "budget %d frame %d camera %d" % (budget, k, i))
            if k == 0:
                assert infos[1]["coarse_max"] == 120 and infos[0]["coarse_max"] == 60 and res[1]["did_coarse"] == 1
                assert res[0]["n_meas"] > (900 if budget == 1000 else 1024)
        for c, f in zip(cams, orig):
            c.twin.opts = f
    for c in cams:
        c.close()
    kf0.close()
    ctx0.close()


def test_a_refused_plain_batch_leaves_the_trackers_usable(hip):
    """ptam_track_map_frames_batch, nb = 2 on the rig of test_the_smallest_chain: a call refused for its second slot (a keyframe of
    another size) and one refused for its options, each followed by a good call — whose results must be those of the same good
    calls on twin trackers that never saw a refusal"""
    size = (163, 121)
    seq = SC.tracking_sequence()[0]
    f0 = [np.ascontiguousarray(f[:size[1], :size[0]]) for f in seq[:2]]
    cams = [Camera(hip, size=size, empty=True, frames=f0, estimator=False), Camera(hip, size=size, empty=True, frames=f0[::-1], estimator=False)]
    big_ctx = host.Context(lib=hip)
    big_kf = host.KeyFrame(big_ctx)
    poses = np.stack([np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]]), np.concatenate([np.eye(3).reshape(9), [0.01, -0.02, 1.4]])])
    trs, kfs = [c.tr for c in cams], [c.kf for c in cams]
    twins, kf_twins = [c.twin for c in cams], [c.kf_twin for c in cams]
    for k in range(2):
        d = [c.d_frames[k] for c in cams]
        with pytest.raises(host.PtamError):
            host.Tracker.TrackFramesBatch(trs, [kfs[0], big_kf], d, poses)
        with pytest.raises(host.PtamError):
            host.Tracker.TrackFramesBatch(trs, kfs, d, poses, trs[0].opts(coarse_range=5000))
        got = host.Tracker.TrackFramesBatch(trs, kfs, d, poses)
        want = host.Tracker.TrackFramesBatch(twins, kf_twins, d, poses)
        for f in got.dtype.names:
            assert np.array_equal(got[f], want[f]), (k, f)
        assert np.array_equal(got["pose"], poses) and (got["n_meas"] == 0).all()      # an empty map: the pose that went in
        for c in cams:
            assert c.tr.iteration_set().tobytes() == c.twin.iteration_set().tobytes()
    big_kf.close()
    big_ctx.close()
    for c in cams:
        c.close()


def test_coarse_lists_beyond_the_fused_kernels_equal_the_plain_batch(hip):
    """ptam_track_frames_batch with CoarseMax = 1100 on maps of about 2 000 points, no estimators, both models fast enough for the
    coarse stage: every coarse list outgrows the fused pose kernels, so both stages go through the gather pass and the small / general
    kernel pair — the launches of ptam_track_map_frames_batch from the same poses with the same options.  Every result field equal."""
    seq = SC.tracking_sequence()
    ctx0 = host.Context(lib=hip)
    kf0 = host.KeyFrame(ctx0).MakeKeyFrame_Lite(seq[2])
    big = synth.make_sequence_map([kf0.level(l) for l in range(4)], seq[3], counts=(900, 500, 300, 200))
    assert len(big["world"]) > 1900
    cams = [Camera(hip, mapping=big, estimator=False), Camera(hip, mapping=big, estimator=False)]
    ks = [0, 1]
    for c, k in zip(cams, ks):
        c.model = c.tr.motion_model(c.poses[k])
        c.model.msd_scaled_velocity = 0.05      # (above coarse_min_velocity = 0.006; the velocity itself stays zero)
    opts = cams[0].tr.opts(coarse_max=1100)
    res, infos, _ = _batch(cams, ks, opts)
    print("points", len(big["world"]), "n_coarse", res["n_coarse"], "n_meas", res["n_meas"])
    for i in range(2):
        assert (infos[i]["try_coarse"], infos[i]["coarse_max"]) == (1, 1100) and res[i]["did_coarse"] == 1 and res[i]["n_meas"] >= 50, i
    opts["try_coarse"] = 1
    plain = host.Tracker.TrackFramesBatch([c.twin for c in cams], [c.kf_twin for c in cams], [c.d_frames[k] for c, k in zip(cams, ks)],
                                          np.stack([infos[i]["pose_in"] for i in range(2)]), opts)
    for f in res.dtype.names:
        assert np.array_equal(res[f], plain[f]), f
    for c in cams:
        assert c.tr.iteration_set().tobytes() == c.twin.iteration_set().tobytes()
        c.close()
    kf0.close()
    ctx0.close()


def test_closed_loop_against_the_cpu_composition(hip, oracle):
    """a batch of two cameras on the same sequence: frame by frame both start from the CPU loop's model state and must agree with it
    as ptam_track_frame_sbi does (test_gpu_sbi_track.py); and a free-running batch loop against a free-running ptam_track_frame_sbi"""
    loop = SC.closed_loop_on_oracle(oracle)
    rots = SC.sequence_rotations()
    cams = [Camera(hip), Camera(hip)]
    for k, f in enumerate(loop):
        for c in cams:
            c.model = _abi.MotionModel.from_buffer_copy(f["model_before"])
        res, infos, _ = _batch(cams, [k, k])
        ro = f["result"]
        ref = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": f["iteration_set"]}
        for i, c in enumerate(cams):
            print(k, i, "rotation %.2e pose %.2e" % (np.abs(infos[i]["align"]["rotation"] - rots[k]).max(), np.abs(res[i]["pose"] - ro["pose"]).max()))
            _check(res[i], c.tr.iteration_set(), ref, strict=False)
            assert np.abs(infos[i]["align"]["rotation"] - rots[k]).max() <= TOL_ALIGN
        assert res[0].tobytes() == res[1].tobytes()
    # free-running: the batch (nb = 1) against ptam_track_frame_sbi on the twin tracker
    cam = cams[0]
    for tr in (cam.tr, cam.twin):
        m = cam.map
        tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], cam.kf0, m["src_level"], m["center"])
    cam.reset_estimator()
    est2 = host.RotationEstimator(cam.ctx)
    cam.model = cam.tr.motion_model(cam.poses[0])
    m2 = cam.twin.motion_model(cam.poses[0])
    for k in range(SC.TRACK_FRAMES):
        res, infos, _ = _batch([cam], [k])
        r2, al2 = cam.twin.track_frame_sbi(cam.kf_twin, cam.d_frames[k], m2, est2, cam.twin.opts())
        r = res[0]
        print(k, "free-running: pose against ptam_track_frame_sbi %.2e, against the truth %.2e" % (np.abs(r["pose"] - r2["pose"]).max(), np.abs(r["pose"] - cam.poses[k]).max()))
        assert np.abs(infos[0]["align"]["rotation"] - al2["rotation"]).max() <= TOL_ALIGN
        ref = {"pose": r2["pose"], "did_coarse": bool(r2["did_coarse"]), "n_pvs": list(r2["n_pvs"]), "attempted": list(r2["attempted"]),
               "found": list(r2["found"]), "n_coarse": r2["n_coarse"], "n_top": r2["n_top"], "n_fine": r2["n_fine"], "n_meas": r2["n_meas"],
               "depth": (r2["depth_sum"], r2["depth_sum_sq"], r2["depth_n"]), "iteration_set": cam.twin.iteration_set()}
        _check(r, cam.tr.iteration_set(), ref, strict=False)
        assert r["n_meas"] >= 50 and np.abs(r["pose"] - cam.poses[k]).max() < 3e-3, k
    est2.close()
    for c in cams:
        c.close()
