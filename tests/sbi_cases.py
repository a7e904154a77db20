"""The fixtures the SmallBlurryImage tests share (tests/test_sbi_ref.py on the CPU, tests/test_gpu_sbi*.py on the device): rendered
views of the sequence's textured plane and the restatement's results on them, computed once, shared and never modified."""
import functools

import numpy as np

from ptam_cg_amd import synth
from tests import sbi_ref as S

BLURS = (0.75, 2.5)          # Tracker.RotationEstimatorBlur; the keyframes' and the relocaliser's default
VARIANTS = ("R", "T")

# name -> (frame size, rotation of the current view against the target's (rotation vector, rad), noise seed).  The SBI is
# (size / 8) / 2: tiny 10x8 — at sigma 2.5 the 17-tap kernel is wider than the image on both axes, 80 pixels < one workgroup; odd 21x17
# — odd sizes, the centre by integer division, 357 = 256 + 101 pixels (the stride loop's tail); work 40x30 — 1 200 = 4 * 256 + 176;
# blank — constant frames: all gradients zero, degenerate; far — a roll of 0.12 rad with tilt: warped samples leave the image.
# The seeds and rotations were picked on the CPU so that the guards of test_sbi_ref.py hold.
CASES = {
    "tiny": ((160, 128), (0.004, -0.003, 0.02), 11),
    "odd": ((336, 272), (0.01, 0.008, -0.03), 12),
    "work": ((640, 480), (0.02, -0.015, 0.04), 13),
    "blank": ((160, 128), None, 0),
    "far": ((640, 480), (0.03, -0.02, 0.12), 14),
}


def rotated(pose, w):
    """the pose of a camera at pose's centre turned by the rotation vector w: exp(w) * pose"""
    R = S.so3_exp(np.asarray(w, np.float64))
    return np.concatenate([(R @ pose[:9].reshape(3, 3)).reshape(9), R @ pose[9:]])


@functools.lru_cache(maxsize=None)
def texture():
    t = synth.make_plane_texture()
    t.setflags(write=False)
    return t


def render(size, pose, seed):
    im = synth.render_plane_view(synth.AtanCam(synth.DEFAULT_CAMERA, size), pose, texture(), np.random.default_rng(seed))
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def views(name):
    """-> (current frame, target frame)"""
    size, w, seed = CASES[name]
    if w is None:
        f = np.full((size[1], size[0]), 128, np.uint8)
        f.setflags(write=False)
        return f, f
    pose = synth.sequence_pose(3, 64)
    return render(size, rotated(pose, w), seed), render(size, pose, seed + 100)


@functools.lru_cache(maxsize=None)
def reference(name, blur, variant):
    """-> dict(cur, tgt: make_sbi of the two views; align: calc_rotation(cur, tgt))"""
    cur, tgt = (S.make_sbi_from_frame(f, blur, variant) for f in views(name))
    return dict(cur=cur, tgt=tgt, align=S.calc_rotation(cur, tgt, 6))


# ---- the relocaliser's bank: 16 keyframes along the sequence and a current view near keyframe 5 -------------------------------------
BANK_SIZE, BANK_NEAREST, BANK_CURRENT_FRAME = 16, 5, 21


@functools.lru_cache(maxsize=None)
def bank_views():
    """-> (keyframe images (16), their poses (16, 12), the current view): keyframe k is frame 4 k of the 64-frame sequence, the
    current view frame 21 — one frame past keyframe 5"""
    poses = np.stack([synth.sequence_pose(4 * k, 64) for k in range(BANK_SIZE)])
    poses.setflags(write=False)
    kfs = tuple(render((640, 480), poses[k], 200 + k) for k in range(BANK_SIZE))
    return kfs, poses, render((640, 480), synth.sequence_pose(BANK_CURRENT_FRAME, 64), 300)


@functools.lru_cache(maxsize=None)
def bank_reference(variant="R", n=BANK_SIZE, first=0):
    """the restatement's AttemptRecovery on keyframes first .. first + n - 1"""
    kfs, poses, cur = bank_views()
    bank = [S.make_sbi_from_frame(f, 2.5, variant) for f in kfs[first:first + n]]
    return S.relocalise(bank, poses[first:first + n], S.make_sbi_from_frame(cur, 2.5, variant))


# ---- the tracked sequence with the rotation estimator on: the expectation, composed on the CPU ----------------------------------------
TRACK_FRAMES = 8


@functools.lru_cache(maxsize=None)
def tracking_sequence():
    """frames 0-7 of synth.make_tracking_frames, their true poses, the map's source keyframe image and pose"""
    return synth.make_tracking_frames(TRACK_FRAMES)


@functools.lru_cache(maxsize=None)
def sequence_rotations():
    """the restatement's rotation of every frame against the one before it (sigma 0.75, 6 iterations); frame 0 against itself"""
    frames = tracking_sequence()[0]
    sbis = [S.make_sbi_from_frame(f, 0.75) for f in frames]
    return [S.calc_rotation(sbis[k], sbis[max(k - 1, 0)], 6)["rotation"] for k in range(len(frames))]


def coarse_opts(tracker, model):
    """the bTryCoarse heuristics of src/Tracker.cc:505-516 as ptam_track_frame has them -> the frame's opts"""
    o = tracker.opts()
    o["try_coarse"] = 0 if (model.disable_coarse or model.msd_scaled_velocity < model.coarse_min_velocity or o["coarse_max"][0] == 0) else 1
    if model.just_recovered:
        o["try_coarse"], o["coarse_max"], o["coarse_range"] = 1, 2 * o["coarse_max"], 2 * o["coarse_range"]
    return o


def closed_loop_on_oracle(oracle):
    """Tracker::TrackFrame's tracking branch with the estimator on, over the 8 frames, composed from the restatement's rotation, the
    prediction of src/Tracker.cc:1013-1029 in numpy and the oracle's TrackMap / UpdateMotionModel
    -> per frame dict(model_before (bytes), pose_in, result, iteration_set)"""
    import ctypes as C

    from ptam_cg_amd import host
    frames, poses, kim, kpose = tracking_sequence()
    ctx = host.Context(lib=oracle)
    kf0 = host.KeyFrame(ctx).MakeKeyFrame_Lite(kim)
    m = synth.make_sequence_map([kf0.level(l) for l in range(4)], kpose)
    tr = host.Tracker(ctx, len(m["world"]))
    tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], kf0, m["src_level"], m["center"])
    kf = host.KeyFrame(ctx)
    mm = tr.motion_model(poses[0])
    out = []
    for k, rot in enumerate(sequence_rotations()):
        before = bytes(mm)
        o = coarse_opts(tr, mm)
        mm.just_recovered = 0
        pred = S.predict_sbi(np.array(mm.pose), np.array(mm.velocity), rot)
        mm.start_pose[:] = mm.pose[:]
        mm.pose[:] = pred.tolist()
        r = tr.TrackMap(kf.MakeKeyFrame_Lite(frames[k]), pred, o)
        oracle.motion_update(C.byref(mm), host._ptr(np.array([r])))
        out.append(dict(model_before=before, pose_in=pred, result=r.copy(), iteration_set=tr.iteration_set()))
    tr.close()
    return out
