"""Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) around TrackMap, restated in plain Python from the reference's lines:
AssessTrackingQuality (:1062-1107), the branch choice (:129, :168), the model a recovery frame leaves (:171-175, :196-207, :508-513,
:692-696), ClosestKeyFrame / KeyFrameLinearDist / IsNeedNewKeyFrame (src/MapMaker.cc:696-703, :736-763) and the keyframe decision
(:146-166).  The state is a dict: lost_frames, quality, frame, last_keyframe_dropped and `model`, itself a dict with the fields of
ptam_motion_model that move here."""
import math

import numpy as np

BAD, GOOD = 0, 1
TRACKED, RECOVERED, RECOVERY_FAILED = 0, 1, 2

DEFAULTS = dict(quality_good=0.3, quality_lost=0.13, wiggle_scale=0.1, wiggle_scale_depth_normalized=0.1, max_kf_dist_wiggle_mult=0.05,
                reloc_blur=2.5, reloc_max_score=9e6)


def reset(pose):
    """Tracker::Reset :52-62"""
    pose = np.asarray(pose, np.float64).reshape(12).copy()
    model = dict(pose=pose, start_pose=pose.copy(), velocity=np.zeros(6), msd_scaled_velocity=0.0, scene_depth_mean=1.0,
                 scene_depth_sigma=0.0, just_recovered=0)
    return dict(model=model, lost_frames=0, quality=GOOD, frame=0, last_keyframe_dropped=-20)


def assess(state, attempted, found, closest_kf_dist, opts=DEFAULTS):
    """AssessTrackingQuality :1062-1107, in place"""
    total_attempted, total_found = int(sum(attempted)), int(sum(found))
    large_attempted, large_found = int(sum(attempted[2:])), int(sum(found[2:]))
    if total_found == 0 or total_attempted == 0:
        state["quality"] = BAD
    else:
        total_frac = total_found / total_attempted
        large_frac = large_found / large_attempted if large_attempted > 10 else total_frac
        if total_frac > opts["quality_good"]:
            state["quality"] = GOOD
        elif large_frac < opts["quality_lost"]:
            state["quality"] = BAD
        elif closest_kf_dist > opts["wiggle_scale"] * 10.0:      # (otherwise the quality stays what it was)
            state["quality"] = BAD
    if state["quality"] == BAD:
        state["lost_frames"] += 1
    else:
        state["lost_frames"] = 0
    return state


def branch(state):
    """:129 / :168 -> True: the camera attempts recovery"""
    return state["lost_frames"] >= 3


def camera_position(pose):
    pose = np.asarray(pose, np.float64).reshape(12)
    return -pose[:9].reshape(3, 3).T @ pose[9:]


def linear_dist(pose_a, pose_b):
    """KeyFrameLinearDist, src/MapMaker.cc:696-703"""
    d = camera_position(pose_b) - camera_position(pose_a)
    return math.sqrt(float(d @ d))


def closest_keyframe(pose, kf_poses):
    """ClosestKeyFrame :736-752 -> (index, distance): the first strictly lowest distance; (-1, 0.0) without keyframes"""
    best, at = 9999999999.9, -1
    for i, kp in enumerate(np.asarray(kf_poses, np.float64).reshape(-1, 12)):
        d = linear_dist(pose, kp)
        if d < best:
            best, at = d, i
    return (at, best) if at >= 0 else (-1, 0.0)


def need_new_keyframe(dist, scene_depth_mean, opts=DEFAULTS):
    """IsNeedNewKeyFrame :754-763"""
    return dist * (1.0 / scene_depth_mean) > opts["max_kf_dist_wiggle_mult"] * opts["wiggle_scale_depth_normalized"]


def scene_depth(model, result):
    """:692-696"""
    if result["depth_n"] > 20:
        mean = result["depth_sum"] / result["depth_n"]
        model["scene_depth_mean"] = mean
        model["scene_depth_sigma"] = math.sqrt(result["depth_sum_sq"] / result["depth_n"] - mean * mean)


def recovery_opts(coarse_max, coarse_range):
    """:508-513 on the frame that AttemptRecovery is followed by -> (try_coarse, coarse_max, coarse_range)"""
    return 1, 2 * coarse_max, 2 * coarse_range


def after_recovered_frame(state, reloc_pose, result, kf_poses, opts=DEFAULTS):
    """a good AttemptRecovery (:196-207), TrackMap from its pose, AssessTrackingQuality (:171-175): no prediction, no UpdateMotionModel
    -> (closest keyframe, its distance)"""
    m = state["model"]
    m["start_pose"] = np.asarray(reloc_pose, np.float64).reshape(12).copy()
    m["pose"] = np.asarray(result["pose"], np.float64).reshape(12).copy()
    m["velocity"] = np.zeros(6)
    m["just_recovered"] = 0
    scene_depth(m, result)
    state["frame"] += 1
    at, dist = closest_keyframe(m["pose"], kf_poses)
    assess(state, result["attempted"], result["found"], dist, opts)
    return at, dist


def after_failed_recovery(state):
    """:168-176 with AttemptRecovery false: only mnFrame (:111) has moved"""
    state["frame"] += 1


def after_tracked_frame(state, result, kf_poses, opts=DEFAULTS):
    """the assessment and the keyframe decision of :135-166 behind a tracked frame whose model the caller has updated
    -> dict(closest_kf, closest_kf_dist, need_new_keyframe, want_keyframe)"""
    state["frame"] += 1
    at, dist = closest_keyframe(result["pose"], kf_poses)
    assess(state, result["attempted"], result["found"], dist, opts)
    need = bool(at >= 0 and need_new_keyframe(dist, state["model"]["scene_depth_mean"], opts))
    want = state["quality"] == GOOD and state["frame"] - state["last_keyframe_dropped"] > 20
    return dict(closest_kf=at, closest_kf_dist=dist, need_new_keyframe=need, want_keyframe=bool(want))
