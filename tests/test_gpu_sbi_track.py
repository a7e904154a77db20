"""-m gpu: ptam_track_frame_sbi — the tracked frame with the SmallBlurryImage rotation estimator on (src/Tracker.cc:94-108,
:1016-1028) — against the same frame composed from the public pieces (bit for bit), against the CPU composition of the restatement
and the checker's TrackMap (tests/sbi_cases.closed_loop_on_oracle; the tolerances of test_gpu_trackmap's closed-loop parity test),
and the recovery path ptam_relocalise -> ptam_motion_recover -> ptam_track_frame_sbi.  The rotation's own correctness is
tests/test_gpu_sbi.py's job."""
import ctypes as C

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import sbi_cases as SC
from tests.test_gpu_sbi import TOL_ALIGN
from tests.test_gpu_trackmap import _check, _copy_model

pytestmark = pytest.mark.gpu
IDENTITY3 = np.eye(3)


class Rig:
    """one context on the sequence: the map's source keyframe, the uploaded frames, and trackers made on demand"""

    def __init__(self, hip):
        self.lib = hip
        self.frames, self.poses, kim, self.kpose = SC.tracking_sequence()
        self.ctx = host.Context(lib=hip)
        self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(kim)
        self.map = synth.make_sequence_map([self.kf0.level(l) for l in range(4)], self.kpose)
        self.d_frames = [host.DevBuf(self.ctx, f) for f in self.frames]
        self.made = []

    def tracker(self):
        m = self.map
        tr = host.Tracker(self.ctx, len(m["world"]))
        tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], self.kf0, m["src_level"], m["center"])
        self.made.append(tr)
        return tr

    def close(self):
        for o in self.made + self.d_frames + [self.kf0]:
            (o.free if isinstance(o, host.DevBuf) else o.close)()
        self.ctx.close()


@pytest.fixture(scope="module")
def rig(hip):
    r = Rig(hip)
    yield r
    r.close()


class Pieces:
    """the frame as a caller composes it from the public entry points: ptam_make_keyframe_lite_dev, ptam_sbi_make (this frame's; the
    first frame's serves as last frame's too), ptam_sbi_calc_rotation, ptam_motion_predict_sbi, ptam_track_map, ptam_motion_update"""

    def __init__(self, rig, blur=0.75):
        self.rig, self.blur = rig, blur
        self.tr, self.kf = rig.tracker(), host.KeyFrame(rig.ctx)
        self.sbi = [host.SmallBlurryImage(rig.ctx), host.SmallBlurryImage(rig.ctx)]
        self.last = None

    def frame(self, d_frame, model):
        lib, ctx = self.rig.lib, self.rig.ctx
        o = SC.coarse_opts(self.tr, model)
        model.just_recovered = 0
        ctx._check(lib.make_keyframe_lite_dev(ctx.h, self.kf.h, d_frame.p), "make_keyframe_lite_dev")
        this = 0 if self.last is None else 1 - self.last
        self.sbi[this].MakeFromKF(self.kf, self.blur)
        al = self.sbi[this].CalcSBIRotation(self.sbi[this if self.last is None else self.last], 6)
        lib.motion_predict_sbi(C.byref(model), host._pd(np.ascontiguousarray(al["rotation"].reshape(9))))
        r = self.tr.TrackMap(self.kf, np.array(model.pose), o)
        lib.motion_update(C.byref(model), host._ptr(np.array([r])))
        self.last = this
        return r, al, o

    def close(self):
        for o in self.sbi + [self.kf]:
            o.close()


def test_first_frame_has_the_identity_rotation(rig):
    """after a reset the frame is both "this" and "last": the rotation is the identity to the bit, and of the velocity only v[2] moves
    the prediction — the frame is ptam_make_keyframe_lite_dev + ptam_track_map from exp((0, 0, v2, 0, 0, 0)) * pose"""
    ctx, lib = rig.ctx, rig.lib
    tr, kf, est = rig.tracker(), host.KeyFrame(ctx), host.RotationEstimator(ctx)
    m = tr.motion_model(rig.poses[0])
    m.velocity[:] = [0.01, -0.02, 0.003, 0.01, 0.02, -0.03]
    m.msd_scaled_velocity = 1.0                                       # (the heuristics then try the coarse stage, as the defaults do)
    m2 = _copy_model(m)
    r, al = tr.track_frame_sbi(kf, rig.d_frames[0], m, est)
    assert np.array_equal(al["rotation"], IDENTITY3) and np.array_equal(al["R"], np.eye(2)) and not al["t"].any() and al["score"] == 0.0
    step = np.zeros(12)
    lib.se3_exp(host._ptr(np.array([0, 0, m2.velocity[2], 0, 0, 0.0])), host._ptr(step))
    want = synth.se3_mul(step, np.array(m2.pose))
    lib.motion_predict_sbi(C.byref(m2), host._pd(np.eye(3).reshape(9).copy()))
    assert np.abs(np.array(m2.pose) - want).max() <= 2e-15 and np.array_equal(np.array(m2.start_pose), rig.poses[0])
    kf2, fresh = host.KeyFrame(ctx), rig.tracker()
    ctx._check(lib.make_keyframe_lite_dev(ctx.h, kf2.h, rig.d_frames[0].p), "make_keyframe_lite_dev")
    r2 = fresh.TrackMap(kf2, np.array(m2.pose), fresh.opts())
    assert r.tobytes() == r2.tobytes() and r["did_coarse"] == 1 and r["n_meas"] >= 50
    # a later frame turns against its predecessor; after a reset the next one is its own predecessor again
    _, al = tr.track_frame_sbi(kf, rig.d_frames[1], m, est)
    assert not np.array_equal(al["rotation"], IDENTITY3) and al["score"] > 0
    est.reset()
    _, al = tr.track_frame_sbi(kf, rig.d_frames[2], m, est)
    assert np.array_equal(al["rotation"], IDENTITY3) and al["score"] == 0.0
    for o in (est, kf, kf2):
        o.close()


def test_frames_equal_the_composition_of_the_public_pieces(rig):
    """frames 0-7, bit for bit; refused calls in the middle — a null frame, refused at once, and options that TrackMap refuses after the
    estimator has stepped — change nothing that follows"""
    tr, kf, est = rig.tracker(), host.KeyFrame(rig.ctx), host.RotationEstimator(rig.ctx)
    twin = Pieces(rig)
    m, m2 = tr.motion_model(rig.poses[0]), tr.motion_model(rig.poses[0])
    for k in range(SC.TRACK_FRAMES):
        if k in (0, 4):
            before, res, al = bytes(m), np.zeros(1, host.TRACKMAP_RESULT_DT), _abi.SbiAlignment()
            rc = rig.lib.track_frame_sbi(tr.h, kf.h, None, C.byref(m), est.h, None, host._ptr(res), C.byref(al))
            assert rc == -1 and bytes(m) == before and not res.tobytes().strip(b"\0")
        if k in (1, 5):
            # a refusal AFTER the estimator's step: TrackMap refuses the options (estimator 7) when ANOTHER frame's keyframe and
            # SmallBlurryImage have been made — the free slot is overwritten, the last / this pair and the model must not move
            before = bytes(m)
            with pytest.raises(host.PtamError):
                tr.track_frame_sbi(kf, rig.d_frames[(k + 3) % SC.TRACK_FRAMES], m, est, tr.opts(estimator=7))
            assert bytes(m) == before
        r, al = tr.track_frame_sbi(kf, rig.d_frames[k], m, est, tr.opts())
        r2, al2, _ = twin.frame(rig.d_frames[k], m2)
        assert r.tobytes() == r2.tobytes() and bytes(m) == bytes(m2), k
        assert all(np.array_equal(np.asarray(al[f]), np.asarray(al2[f])) for f in al), k
        assert np.abs(r["pose"] - rig.poses[k]).max() < 3e-3 and r["n_meas"] >= 50, k
        assert (k == 0) == np.array_equal(al["rotation"], IDENTITY3)
    est.close()
    kf.close()
    twin.close()


def test_closed_loop_against_the_cpu_composition(rig, oracle):
    """as test_gpu_trackmap's closed-loop parity: frame by frame the product starts from the CPU loop's model state and must agree
    with it — discrete outcome exactly, poses and positions within that test's allowance.  The estimator's own state (last frame's
    image) is the product's; the rotation it finds differs from the restatement's by test_gpu_sbi's tolerance."""
    loop = SC.closed_loop_on_oracle(oracle)
    tr, kf, est = rig.tracker(), host.KeyFrame(rig.ctx), host.RotationEstimator(rig.ctx)
    rots = SC.sequence_rotations()
    for k, f in enumerate(loop):
        m = _abi.MotionModel.from_buffer_copy(f["model_before"])
        r, al = tr.track_frame_sbi(kf, rig.d_frames[k], m, est, tr.opts())
        ro = f["result"]
        ref = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": f["iteration_set"]}
        print(k, "rotation %.2e pose %.2e" % (np.abs(al["rotation"] - rots[k]).max(), np.abs(r["pose"] - ro["pose"]).max()))
        _check(r, tr.iteration_set(), ref, strict=False)
        assert np.abs(al["rotation"] - rots[k]).max() <= TOL_ALIGN
    est.close()
    kf.close()


def test_recovery_path(rig):
    """ptam_relocalise on frame 0 against the map's source keyframe, ptam_motion_recover, and the next ptam_track_frame_sbi: the flag
    is consumed and the coarse stage runs with doubled CoarseMax / CoarseRange although the model stands still (src/Tracker.cc:508-513)"""
    ctx, lib = rig.ctx, rig.lib
    rel = host.Relocaliser(ctx, capacity=1)
    assert rel.add(rig.kf0, rig.kpose) == 0
    kf, est, tr = host.KeyFrame(ctx), host.RotationEstimator(ctx), rig.tracker()
    ctx._check(lib.make_keyframe_lite_dev(ctx.h, kf.h, rig.d_frames[0].p), "make_keyframe_lite_dev")
    rec = rel.AttemptRecovery(kf)
    assert rec["best"] == 0 and rec["good"] and np.isfinite(rec["pose"]).all()
    m = tr.motion_model(rig.poses[3])
    m.velocity[:] = [0.1] * 6
    lib.motion_recover(C.byref(m), host._pd(rec["pose"]))
    assert m.just_recovered == 1 and not np.array(m.velocity).any()
    assert np.array_equal(np.array(m.pose), rec["pose"]) and np.array_equal(np.array(m.start_pose), rec["pose"])
    twin, m2 = Pieces(rig), _copy_model(m)
    r, _ = tr.track_frame_sbi(kf, rig.d_frames[0], m, est)
    r2, _, o = twin.frame(rig.d_frames[0], m2)
    assert (o["try_coarse"][0], o["coarse_max"][0], o["coarse_range"][0]) == (1, 120, 60)
    assert r.tobytes() == r2.tobytes() and bytes(m) == bytes(m2) and m.just_recovered == 0
    print("recovered: pose off by %.2e before, %.2e after; n_coarse %d, n_meas %d"
          % (np.abs(rec["pose"] - rig.poses[0]).max(), np.abs(r["pose"] - rig.poses[0]).max(), r["n_coarse"], r["n_meas"]))
    assert r["did_coarse"] == 1 and r["n_coarse"] > 60 and r["n_meas"] >= 50          # more than CoarseMax = 60: the doubled set
    # the control: the same standing model without the flag does not try the coarse stage
    m3 = tr.motion_model(rec["pose"])
    est.reset()
    r3, _ = rig.tracker().track_frame_sbi(kf, rig.d_frames[0], m3, est)
    assert r3["did_coarse"] == 0
    for o_ in (rel, kf, est, twin):
        o_.close()
