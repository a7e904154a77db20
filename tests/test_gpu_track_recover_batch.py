"""-m gpu: ptam_track_frames_recover_batch — Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) for a batch of cameras in one
chain: a camera that is lost runs the relocaliser inside the chain and is tracked from its pose in the same call.  Every frame is
compared with the composition of the existing entries on twin trackers (ptam_track_frames_batch's pieces for a tracking frame;
ptam_relocalise + ptam_track_map_frame with the doubled coarse options for a recovered one), byte for byte, and the state with
tests/track_state_ref.py.  The fixture's own condition is checked on the CPU in tests/test_track_state_ref.py."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import sbi_cases as SC
from tests import sbi_ref as S
from tests import track_state_ref as T
from tests.test_gpu_sbi import TOL_ALIGN, TOL_SSD, _rel
from tests.test_gpu_track_frames_batch import Camera, _check_against_twin
from tests.test_gpu_trackmap import _check, _copy_model
from tests.test_track_state_ref import BLANK_VALUE, recovery_bank

pytestmark = pytest.mark.gpu

# KeyFrameLinearDist on the host against numpy's: a 3x3 product, a difference, a square root on distances of order 1 — a few ulps
TOL_DIST = 1e-14


def _copy_state(s):
    return _abi.TrackState.from_buffer_copy(bytes(s))


def _ref_state(s):
    """a ptam_track_state as tests/track_state_ref.py's dict"""
    m = s.model
    model = dict(pose=np.array(m.pose), start_pose=np.array(m.start_pose), velocity=np.array(m.velocity), msd_scaled_velocity=m.msd_scaled_velocity,
                 scene_depth_mean=m.scene_depth_mean, scene_depth_sigma=m.scene_depth_sigma, just_recovered=m.just_recovered)
    return dict(model=model, lost_frames=s.lost_frames, quality=s.quality, frame=s.frame, last_keyframe_dropped=s.last_keyframe_dropped)


def _scalars(s):
    return (s.lost_frames, s.quality, s.frame, s.last_keyframe_dropped) if hasattr(s, "model") else \
        (s["lost_frames"], s["quality"], s["frame"], s["last_keyframe_dropped"])


class RecCamera(Camera):
    """a camera of tests/test_gpu_track_frames_batch.py with its ptam_track_state, its relocaliser (bank, poses, scratch image) and a
    second relocaliser for the twin's ptam_relocalise"""

    def __init__(self, hip, size=(640, 480), **kw):
        super().__init__(hip, size=size, **kw)
        self.size = size
        self.state = self.tr.track_state(self.poses[0])
        self.rel = self.rel_twin = None
        self.bank_kfs, self.kf_poses = [], np.zeros((0, 12))

    def make_bank(self, images, poses, capacity=None):
        w, h = self.size
        self.bank_kfs = [host.KeyFrame(self.ctx).MakeKeyFrame_Lite(np.ascontiguousarray(im[:h, :w])) for im in images]
        self.kf_poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
        self.rel, self.rel_twin = (host.Relocaliser(self.ctx, capacity or len(images), size=self.size) for _ in range(2))
        for rel in (self.rel, self.rel_twin):
            rel.add_batch(self.bank_kfs, self.kf_poses)
        self.ctx.sync()
        return self

    def lose(self):
        self.state.lost_frames, self.state.quality = 3, T.BAD

    def restart(self, pose):
        """a new history on both sides: the trackers' finders keep templates from frame to frame"""
        m = self.map
        for tr in (self.tr, self.twin):
            tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], self.kf0, m["src_level"], m["center"])
        if self.est is not None:
            self.reset_estimator()
        self.state = self.tr.track_state(pose)

    def close(self):
        for o in [self.rel, self.rel_twin] + self.bank_kfs:
            if o is not None:
                o.close()
        super().close()


def _sequence_bank(cam):
    ims, poses = recovery_bank()
    return cam.make_bank(ims, poses)


def _batch(cams, ks, state_opts=None, opts=None, rels=None):
    """one ptam_track_frames_recover_batch, camera i on its frame ks[i] -> (results, infos, the states before)"""
    before = [_copy_state(c.state) for c in cams]
    res, infos = host.Tracker.track_frames_recover_batch([c.tr for c in cams], [c.kf for c in cams], [c.d_frames[k] for c, k in zip(cams, ks)],
                                                         [c.state for c in cams], [c.est for c in cams],
                                                         [c.rel for c in cams] if rels is None else rels, opts, state_opts)
    for c in cams:
        c.model = _copy_model(c.state.model)
    return res, infos, before


def _check_tracked(cam, k, r, info, before, tag, opts=T.DEFAULTS):
    """a tracking frame: ptam_track_frames_batch's twin for result, model, info; tests/track_state_ref.py for the state"""
    assert info["branch"] == T.TRACKED and not info["reloc"]["good"] and not info["reloc"]["pose"].any(), tag
    _check_against_twin(cam, k, r, info, before.model, tag)
    ref = _ref_state(before)
    ref["model"] = _ref_state(cam.state)["model"]      # (the model is the twin's, checked above; the decision reads its depth mean)
    want = T.after_tracked_frame(ref, r, cam.kf_poses, opts)
    assert _scalars(cam.state) == _scalars(ref), (tag, _scalars(cam.state), _scalars(ref))
    assert (info["closest_kf"], bool(info["need_new_keyframe"]), bool(info["want_keyframe"])) == \
        (want["closest_kf"], want["need_new_keyframe"], want["want_keyframe"]), (tag, info, want)
    assert abs(info["closest_kf_dist"] - want["closest_kf_dist"]) <= TOL_DIST, tag


def _twin_recovery_frame(cam, k, max_score):
    """the recovery frame's keyframe, the estimator's image (no alignment) and ptam_relocalise on the twin side"""
    cam.ctx._check(cam.lib.make_keyframe_lite_dev(cam.ctx.h, cam.kf_twin.h, cam.d_frames[k].p), "make_keyframe_lite_dev")
    if cam.est is not None:
        this = 0 if cam.last is None else 1 - cam.last
        cam.sbi[this].MakeFromKF(cam.kf_twin, 0.75)
        cam.last = this
    return cam.rel_twin.AttemptRecovery(cam.kf_twin, 2.5, max_score)


def _check_reloc(info, rl, tag):
    got = info["reloc"]
    assert (got["best"], got["good"], got["best_ssd"]) == (rl["best"], rl["good"], rl["best_ssd"]), (tag, got, rl)
    assert got["pose"].tobytes() == rl["pose"].tobytes(), tag
    assert all(np.array_equal(np.asarray(got["align"][f]), np.asarray(rl["align"][f])) for f in rl["align"]), tag
    assert not np.asarray(info["align"]["rotation"]).any() and info["align"]["n_used"] == 0, tag      # nothing was aligned for the estimator


def _check_recovered(cam, k, r, info, before, tag, max_score=9e6, opts=T.DEFAULTS):
    """a recovery frame: ptam_relocalise + ptam_track_map_frame from its pose with the doubled options on the twin"""
    rl = _twin_recovery_frame(cam, k, max_score)
    _check_reloc(info, rl, tag)
    o = cam.twin.opts()
    assert (info["try_coarse"], info["coarse_max"], info["coarse_range"]) == T.recovery_opts(int(o["coarse_max"][0]), int(o["coarse_range"][0])), tag
    if not rl["good"]:
        assert info["branch"] == T.RECOVERY_FAILED, tag
        assert r.tobytes() == bytes(r.nbytes) and not info["pose_in"].any(), tag
        ref = _ref_state(before)
        T.after_failed_recovery(ref)
        want = _copy_state(before)
        want.frame = ref["frame"]
        assert bytes(cam.state) == bytes(want), tag                    # the state differs in `frame` only
        assert (info["closest_kf"], info["need_new_keyframe"], info["want_keyframe"]) == (-1, 0, 0), tag
        return None
    assert info["branch"] == T.RECOVERED and np.array_equal(info["pose_in"], rl["pose"]), tag
    o["try_coarse"], o["coarse_max"], o["coarse_range"] = T.recovery_opts(int(o["coarse_max"][0]), int(o["coarse_range"][0]))
    r2 = cam.twin.TrackFrame(cam.kf_twin, cam.d_frames[k], rl["pose"], o)
    assert r.tobytes() == r2.tobytes(), (tag, r, r2)
    assert cam.tr.iteration_set().tobytes() == cam.twin.iteration_set().tobytes(), tag
    ref = _ref_state(before)
    at, dist = T.after_recovered_frame(ref, rl["pose"], r2, cam.kf_poses, opts)
    got = _ref_state(cam.state)
    assert _scalars(got) == _scalars(ref), (tag, _scalars(got), _scalars(ref))
    for f, v in ref["model"].items():
        assert np.array_equal(np.asarray(got["model"][f]), np.asarray(v)), (tag, f)
    m, b = cam.state.model, before.model
    assert (m.coarse_min_velocity, m.use_constant_velocity, m.disable_coarse) == (b.coarse_min_velocity, b.use_constant_velocity, b.disable_coarse)
    assert info["closest_kf"] == at and abs(info["closest_kf_dist"] - dist) <= TOL_DIST and (info["need_new_keyframe"], info["want_keyframe"]) == (0, 0), tag
    return r2


# ---- 1. four cameras over seven rounds ---------------------------------------------------------------------------------------------
def _blank():
    return np.full((480, 640), BLANK_VALUE, np.uint8)


@pytest.fixture(scope="module")
def four(hip):
    """0: tracks throughout.  1: frame 0, three blank frames, then frames 4, 5, 6.  2: no estimator.  3: lost, a group of its own with
    reloc_max_score = 1."""
    seq = SC.tracking_sequence()[0]
    f1 = [seq[0], _blank(), _blank(), _blank(), seq[4], seq[5], seq[6]]
    cams = [RecCamera(hip), RecCamera(hip, frames=f1), RecCamera(hip, estimator=False), RecCamera(hip)]
    for c in cams:
        _sequence_bank(c)
    yield cams
    for c in cams:
        c.close()


def test_four_cameras_over_seven_rounds(four):
    A, B, Cc, D = four
    for c in four:
        c.restart(c.poses[0])
    D.lose()
    never = D.tr.state_opts(reloc_max_score=1.0)
    want_lost = [0, 1, 2, 3, 0, 0, 0]
    branches = []
    for rnd in range(7):
        was_lost = B.state.lost_frames >= 3
        res, infos, before = _batch([A, B, Cc], [rnd, rnd, rnd])
        _check_tracked(A, rnd, res[0], infos[0], before[0], "round %d camera 0" % rnd)
        _check_tracked(Cc, rnd, res[2], infos[2], before[2], "round %d camera 2" % rnd)
        if was_lost:
            r2 = _check_recovered(B, rnd, res[1], infos[1], before[1], "round %d camera 1" % rnd)
            assert r2 is not None and infos[1]["reloc"]["best"] == 2 and infos[1]["reloc"]["align"]["score"] < 9e3
            assert np.abs(res[1]["pose"] - B.poses[4]).max() < 1e-3 and infos[1]["coarse_max"] == 120 and infos[1]["coarse_range"] == 60
            assert sum(res[1]["found"]) > 0.8 * sum(res[1]["attempted"]) and B.state.quality == T.GOOD
            # the carried model: zero velocity, the velocity magnitude of the frame before the loss, no doubled range for the next frame
            m = B.state.model
            assert not any(m.velocity) and m.msd_scaled_velocity == before[1].model.msd_scaled_velocity and m.just_recovered == 0
        else:
            _check_tracked(B, rnd, res[1], infos[1], before[1], "round %d camera 1" % rnd)
            if 1 <= rnd <= 3:
                assert sum(res[1]["attempted"]) > 100 and sum(res[1]["found"]) == 0 and B.state.quality == T.BAD
            if rnd == 5:      # the frame after the recovery: predicted from a standing model, with the estimator's pair carried through it
                assert infos[1]["coarse_max"] == 60 and np.abs(res[1]["pose"] - B.poses[5]).max() < 3e-3
        branches.append(infos[1]["branch"])
        assert B.state.lost_frames == want_lost[rnd] and A.state.lost_frames == 0 and Cc.state.lost_frames == 0, rnd
        assert A.state.quality == T.GOOD and np.abs(res[0]["pose"] - A.poses[rnd]).max() < 3e-3
        assert infos[0]["want_keyframe"] == 1 and A.state.frame == rnd + 1      # frame - (-20) > 20 from the first frame on
        # camera 3: lost, and no alignment scores below 1
        k3 = 1 + rnd % 6      # (frames 0 and 7 are in the bank: they score 0)
        res3, infos3, before3 = _batch([D], [k3], never)
        assert _check_recovered(D, k3, res3[0], infos3[0], before3[0], "round %d camera 3" % rnd, max_score=1.0) is None
        assert (D.state.lost_frames, D.state.frame) == (3, rnd + 1)
    assert branches == [T.TRACKED] * 4 + [T.RECOVERED] + [T.TRACKED] * 2


# ---- 2. a failed recovery leaves no trace --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", [False, True])
def test_failed_recovery_leaves_no_trace(four, hip, estimator):
    """camera X sees a failed recovery frame between frames 1 and 2, in one batch with a tracking camera; its twin Y never sees it.
    With an estimator the failed frame is frame 1 again: the estimator's pair advances over it, onto the image it already held."""
    cams = [four[0], four[3]] if estimator else [four[2], RecCamera(hip, estimator=False)]
    X, Y = cams
    if Y.rel is None:
        _sequence_bank(Y)
    for c in cams:
        c.restart(c.poses[0])
    other = four[1]
    other.restart(other.poses[0])
    never = X.tr.state_opts(reloc_max_score=1.0)
    for k in range(4):
        if k == 2:
            it_before, st_before = X.tr.iteration_set().tobytes(), _copy_state(X.state)
            X.lose()
            lost = _copy_state(X.state)
            res, infos, before = _batch([other, X], [0, 1], never)
            assert infos[0]["branch"] == T.TRACKED and infos[1]["branch"] == T.RECOVERY_FAILED
            assert _check_recovered(X, 1, res[1], infos[1], before[1], "the failed frame", max_score=1.0) is None
            lost.frame += 1
            assert bytes(X.state) == bytes(lost) and X.tr.iteration_set().tobytes() == it_before
            X.state = st_before                                     # (the host's own bookkeeping put back: Y's frame counter and quality)
        res, infos, before = _batch([X], [k])
        res2, infos2, _ = _batch([Y], [k])
        _check_tracked(X, k, res[0], infos[0], before[0], "frame %d" % k)
        assert res[0].tobytes() == res2[0].tobytes() and bytes(X.state) == bytes(Y.state), k
        assert X.tr.iteration_set().tobytes() == Y.tr.iteration_set().tobytes(), k
        assert np.array_equal(infos[0]["pose_in"], infos2[0]["pose_in"]), k
        assert all(np.array_equal(np.asarray(infos[0]["align"][f]), np.asarray(infos2[0]["align"][f])) for f in infos[0]["align"]), k
    if not estimator:
        Y.close()


# ---- 3. the smallest chain -----------------------------------------------------------------------------------------------------------
def test_the_smallest_chain(hip):
    """nb = 2 on 163x121 frames with empty maps and 10x7 SmallBlurryImages: one camera tracks, one recovers against a bank of one
    entry, then of two"""
    size = (163, 121)
    seq = SC.tracking_sequence()[0]
    fr = [np.ascontiguousarray(f[:size[1], :size[0]]) for f in seq[:3]]
    pose = np.concatenate([np.eye(3).reshape(9), [0.0, 0.0, 1.5]])
    for n_bank in (1, 2):
        cams = [RecCamera(hip, size=size, empty=True, frames=fr), RecCamera(hip, size=size, empty=True, frames=fr)]
        kf_poses = np.stack([synth.se3_mul(np.concatenate([np.eye(3).reshape(9), [0.01 * i, 0.0, 0.0]]), pose) for i in range(n_bank)])
        for c in cams:
            c.make_bank([seq[2], seq[1]][:n_bank], kf_poses)
            c.state = c.tr.track_state(pose)
        cams[1].lose()
        res, infos, before = _batch(cams, [0, 1])
        _check_tracked(cams[0], 0, res[0], infos[0], before[0], "bank of %d, the tracking camera" % n_bank)
        r2 = _check_recovered(cams[1], 1, res[1], infos[1], before[1], "bank of %d, the recovering camera" % n_bank)
        assert r2 is not None and infos[1]["reloc"]["best"] == n_bank - 1                  # (frame 1 itself is the second entry)
        assert res[1]["n_meas"] == 0 and sum(res[1]["attempted"]) == 0 and np.array_equal(res[1]["pose"], infos[1]["reloc"]["pose"])
        assert (cams[1].state.quality, cams[1].state.lost_frames) == (T.BAD, 4)            # nothing attempted
        assert np.array_equal(cams[0].tr.reloc_ssd(0, n_bank), cams[1].rel_twin.AttemptRecovery(cams[1].kf_twin)["ssd"])
        for c in cams:
            c.close()


# ---- 4. the arg-min beyond one workgroup's stride --------------------------------------------------------------------------------------
def test_argmin_over_a_bank_of_300(hip):
    """160x128 frames; a bank of 300 entries from 3 distinct keyframes, the current view's one first at entry 260 (each thread of the
    arg-min scans every 256th entry: entry 260 is thread 4's second): equal SSDs go to the lowest index.  Two recovering cameras
    share that bank in one call, a third has a bank of its own in which the same keyframe comes first at entry 1."""
    size = (160, 128)
    seq, poses = SC.tracking_sequence()[:2]
    fr = [np.ascontiguousarray(f[:size[1], :size[0]]) for f in seq]
    cams = [RecCamera(hip, size=size, empty=True, frames=fr) for _ in range(3)]
    late = [0, 7] * 130 + [3] * 40
    early = [0, 3, 7] * 100
    for cam, order in ((cams[0], late), (cams[2], early)):
        cam.make_bank([fr[i] for i in (0, 3, 7)], poses[[0, 3, 7]], capacity=300)
        kf_of = dict(zip((0, 3, 7), cam.bank_kfs))
        for rel in (cam.rel, cam.rel_twin):
            rel.close()
        cam.rel, cam.rel_twin = (host.Relocaliser(cam.ctx, 300, size=size) for _ in range(2))
        for rel in (cam.rel, cam.rel_twin):
            rel.add_batch([kf_of[i] for i in order], poses[order])
        cam.kf_poses = np.ascontiguousarray(poses[order])
        cam.ctx.sync()
    cams[1].make_bank([fr[0]], poses[[0]])                   # (its own relocaliser serves the twin's scratch only)
    cams[1].kf_poses = cams[0].kf_poses
    for c in cams:
        c.lose()
    rels = [cams[0].rel, cams[0].rel, cams[2].rel]
    scratch_of_1 = host.SmallBlurryImage(cams[1].ctx, size)

    class Shared:            # camera 1: camera 0's bank, a scratch image of its own
        h, scratch = cams[0].rel.h, scratch_of_1
    rels[1] = Shared
    ks = [3, 3, 3]
    res, infos, before = _batch(cams, ks, rels=rels)
    for i, (cam, want_best) in enumerate(zip(cams, (260, 260, 1))):
        cam.ctx._check(cam.lib.make_keyframe_lite_dev(cam.ctx.h, cam.kf_twin.h, cam.d_frames[ks[i]].p), "make_keyframe_lite_dev")
        cam.ctx.sync()
        twin_rel = cams[0].rel_twin if i < 2 else cam.rel_twin
        if i == 1:            # (ptam_relocalise wants bank and scratch in one context: camera 1's keyframe, made again there)
            kf = host.KeyFrame(cams[0].ctx).MakeKeyFrame_Lite(fr[ks[i]])
            rl = twin_rel.AttemptRecovery(kf)
            kf.close()
        else:
            rl = twin_rel.AttemptRecovery(cam.kf_twin)
        assert rl["best"] == want_best and (rl["ssd"] == rl["best_ssd"]).sum() >= 40
        _check_reloc(infos[i], rl, "camera %d" % i)
        assert infos[i]["branch"] == T.RECOVERED
        assert np.array_equal(cams[0].tr.reloc_ssd(i, 300), rl["ssd"]), i
    scratch_of_1.close()
    for c in cams:
        c.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(four, hip):
    A, B = four[0], four[1]
    ref = RecCamera(hip)
    _sequence_bank(ref)
    for c in (A, B, ref):
        c.restart(c.poses[0])
    small = host.Context(lib=hip, size=(320, 240))
    other_size = host.Relocaliser(small, 2, size=(320, 240))
    kf_small = host.KeyFrame(small).MakeKeyFrame_Lite(np.ascontiguousarray(SC.tracking_sequence()[0][0][:240, :320]))
    other_size.add(kf_small, A.poses[0])
    empty = host.Relocaliser(A.ctx, 2)
    unset = host.Relocaliser(A.ctx, 2)
    A.ctx._check(hip.sbi_bank_add(unset.h, A.bank_kfs[0].h, 2.5, None), "sbi_bank_add")        # an entry, and no pose for it
    A.ctx.sync()
    est_small = host.RotationEstimator(A.ctx, size=(320, 240))

    class Rel:
        def __init__(self, h, scratch):
            self.h, self.scratch = h, scratch

    class Est:
        def __init__(self, h):
            self.h = h
    for k in range(3):
        both = [A, B]
        for c in both:
            c.lose()
        before = [bytes(c.state) for c in both]
        banks_before = [(c.rel.count(), c.rel.bank_poses().tobytes()) for c in both]
        cases = {
            "no bank": ([None, B.rel], None, -1),
            "no scratch": ([Rel(A.rel.h, None), B.rel], None, -1),
            "an empty bank": ([empty, B.rel], None, -3),
            "poses never set": ([unset, B.rel], None, -3),
            "a bank of another image size": ([Rel(other_size.h, A.rel.scratch), B.rel], None, -1),
            "a scratch of another image size": ([Rel(A.rel.h, other_size.scratch), B.rel], None, -1),
            "an estimator of another image size": ([A.rel, B.rel], [Est(est_small.h), B.est], -1),
            "a scratch named twice": ([A.rel, Rel(B.rel.h, A.rel.scratch)], None, -1),
        }
        for name, (rels, ests, want_rc) in cases.items():
            states = [c.state for c in both]
            rc = host.Tracker.track_frames_recover_batch([c.tr for c in both], [c.kf for c in both], [c.d_frames[(k + 3) % 8] for c in both], states,
                                                         ests or [c.est for c in both], rels, None, None, check=False)
            assert rc == want_rc, (name, rc)
            assert [bytes(c.state) for c in both] == before, name
            assert [(c.rel.count(), c.rel.bank_poses().tobytes()) for c in both] == banks_before, name
        # options that TrackMap refuses: nothing moves either
        with pytest.raises(host.PtamError):
            _batch(both, [(k + 3) % 8, (k + 4) % 8], opts=A.tr.opts(estimator=7))
        assert [bytes(c.state) for c in both] == before
        assert empty.count() == 0 and unset.count() == 1
        # estimators and trackers are where they were: the next good call equals that of a camera that saw no refused call
        for c in (A, ref):
            c.state.lost_frames, c.state.quality = 0, T.GOOD
        ra, ia, _ = _batch([A], [k])
        rr, ir, _ = _batch([ref], [k])
        assert ra.tobytes() == rr.tobytes() and bytes(A.state) == bytes(ref.state), k
        assert all(np.array_equal(np.asarray(ia[0]["align"][f]), np.asarray(ir[0]["align"][f])) for f in ia[0]["align"]), k
        assert (k == 0) == np.array_equal(ia[0]["align"]["rotation"], np.eye(3))
    for o in (ref, other_size, kf_small, empty, unset, est_small):
        o.close()
    small.close()


# ---- 6. against the CPU ----------------------------------------------------------------------------------------------------------------
def test_loss_and_recovery_against_the_cpu_composition(hip, oracle):
    """scenario 1's camera 1 (frame 0, three blank frames, frames 4 and 5), the host predicting: on the CPU the oracle's ptam_track_frame
    for the tracked frames, sbi_ref.relocalise + the oracle's TrackMap from its pose for the recovery frame and track_state_ref for
    the state; the device starts every frame from the CPU loop's state, as the closed-loop test of test_gpu_track_frames_batch.py does,
    and must agree within that test's allowances (test_gpu_trackmap._check, strict=False) and test_gpu_sbi.py's TOL_ALIGN / TOL_SSD"""
    frames, poses, kim, kpose = SC.tracking_sequence()
    ims, kf_poses = recovery_bank()
    bank = [S.make_sbi_from_frame(f, 2.5) for f in ims]
    seq = [frames[0], _blank(), _blank(), _blank(), frames[4], frames[5]]
    cam = _sequence_bank(RecCamera(hip, estimator=False, frames=seq))
    ctx = host.Context(lib=oracle)
    kf0 = host.KeyFrame(ctx).MakeKeyFrame_Lite(kim)
    m = synth.make_sequence_map([kf0.level(l) for l in range(4)], kpose)
    tr = host.Tracker(ctx, len(m["world"]))
    tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], kf0, m["src_level"], m["center"])
    kf = host.KeyFrame(ctx)
    ref = T.reset(poses[0])
    mm = tr.motion_model(poses[0])
    branches = []
    for k, frame in enumerate(seq):
        cam.state = _abi.TrackState(_copy_model(mm), ref["lost_frames"], ref["quality"], ref["frame"], ref["last_keyframe_dropped"])
        res, infos, _ = _batch([cam], [k])
        r, info = res[0], infos[0]
        if not T.branch(ref):
            ro = tr.TrackFrameMoving(kf, np.ascontiguousarray(frame).ctypes.data, mm, tr.opts())
            ref["model"]["scene_depth_mean"] = mm.scene_depth_mean
            want = T.after_tracked_frame(ref, ro, kf_poses)
            assert (info["branch"], info["closest_kf"], bool(info["want_keyframe"])) == (T.TRACKED, want["closest_kf"], want["want_keyframe"])
        else:
            rl = S.relocalise(bank, kf_poses, S.make_sbi_from_frame(frame, 2.5))
            got = info["reloc"]
            figures = dict(best_ssd=_rel(got["best_ssd"], rl["ssd"][rl["best"]]), ssd=_rel(cam.tr.reloc_ssd(0, 3), rl["ssd"]), pose=_rel(got["pose"], rl["pose"]),
                           score=_rel(got["align"]["score"], rl["align"]["score"]), rotation=_rel(got["align"]["rotation"], rl["align"]["rotation"]))
            print("recovery frame:", got["best"], {f: "%.2e" % v for f, v in figures.items()})
            assert rl["good"] and (info["branch"], got["best"], got["good"]) == (T.RECOVERED, rl["best"], True)
            assert max(figures["ssd"], figures["best_ssd"]) <= TOL_SSD and max(figures["pose"], figures["score"], figures["rotation"]) <= TOL_ALIGN
            o = tr.opts()
            o["try_coarse"], o["coarse_max"], o["coarse_range"] = T.recovery_opts(int(o["coarse_max"][0]), int(o["coarse_range"][0]))
            ro = tr.TrackMap(kf.MakeKeyFrame_Lite(frame), rl["pose"], o)
            msd = mm.msd_scaled_velocity
            ref["model"] = _ref_state(_abi.TrackState(_copy_model(mm), 0, 0, 0, 0))["model"]
            T.after_recovered_frame(ref, rl["pose"], ro, kf_poses)
            rm = ref["model"]
            mm.pose[:], mm.start_pose[:], mm.velocity[:] = rm["pose"].tolist(), rm["start_pose"].tolist(), [0.0] * 6
            mm.scene_depth_mean, mm.scene_depth_sigma, mm.just_recovered = rm["scene_depth_mean"], rm["scene_depth_sigma"], 0
            assert mm.msd_scaled_velocity == msd == cam.state.model.msd_scaled_velocity and not any(cam.state.model.velocity)
            assert np.abs(np.array(cam.state.model.start_pose) - rl["pose"]).max() <= TOL_ALIGN * max(1.0, np.abs(rl["pose"]).max())
        branches.append(info["branch"])
        print(k, "pose against the CPU's %.2e, found %s" % (np.abs(r["pose"] - ro["pose"]).max(), list(r["found"])))
        cpu = {"pose": ro["pose"], "did_coarse": bool(ro["did_coarse"]), "n_pvs": list(ro["n_pvs"]), "attempted": list(ro["attempted"]),
               "found": list(ro["found"]), "n_coarse": ro["n_coarse"], "n_top": ro["n_top"], "n_fine": ro["n_fine"], "n_meas": ro["n_meas"],
               "depth": (ro["depth_sum"], ro["depth_sum_sq"], ro["depth_n"]), "iteration_set": tr.iteration_set()}
        _check(r, cam.tr.iteration_set(), cpu, strict=False)
        assert _scalars(cam.state) == _scalars(ref), k
        assert np.allclose(np.array(cam.state.model.pose), np.array(mm.pose), rtol=0, atol=5e-6)
    assert branches == [T.TRACKED] * 4 + [T.RECOVERED, T.TRACKED] and ref["lost_frames"] == 0 and ref["quality"] == T.GOOD
    for o in (tr, kf, kf0):
        o.close()
    ctx.close()
    cam.close()
