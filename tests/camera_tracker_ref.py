"""The frame of ptam_camera_tracker_track_frames composed in Python from the calls it is made of — MapMaker.released, Tracker.take_map,
Relocaliser.take_keyframes, shuffle_order + set_shuffle, track_frames_recover_batch, report_frame, the decision of
src/Tracker.cc:146-166 in plain Python, KeyFrame.clone, MapMaker.AddKeyFrame / NoteFrame — and the scene both sides of
tests/test_gpu_camera_tracker.py stand on: the tracking sequence's map (1 244 points) in a resident map whose keyframes are the
recovery bank's three images, with its snapshot, finder and host.MapMaker."""
import numpy as np

from ptam_cg_amd import _abi, host
from tests import sbi_cases as SC
from tests.test_gpu_map_publish import synthetic, uploaded
from tests.test_track_state_ref import recovery_bank

TRACKED, RECOVERED, FAILED = 0, 1, 2
GOOD = 1
CAP, MAX_KF = 8192, 16


def decide(branch, quality, frame, last, gap, queue, max_queue, records):
    """-> "add" | "note" | None"""
    if branch == FAILED or records == 0:
        return None
    if branch == TRACKED and quality == GOOD and frame - last > gap and queue < max_queue:
        return "add"
    return "note"


class Scene:
    """one side: the map's context with the resident map, its snapshot (keyframe section enabled), finder and MapMaker; the tracker's
    context with the frames on the device"""

    def __init__(self, lib, mm_opts=None):
        from ptam_cg_amd import synth
        frames, self.poses, kim, kpose = SC.tracking_sequence()
        ims, kf_poses = recovery_bank()
        self.ctx_m, self.ctx_t = host.Context(lib=lib), host.Context(lib=lib)
        self.kfs = [host.KeyFrame(self.ctx_m).MakeKeyFrame_Lite(np.ascontiguousarray(im)) for im in ims]
        m = synth.make_sequence_map([self.kfs[0].level(l) for l in range(4)], kpose)
        n = len(m["world"])
        h = synthetic(n, K=len(ims))
        p = h["points"]
        p["pv"]["world"], p["pv"]["pixel_right_w"], p["pv"]["pixel_down_w"] = m["world"], m["pixel_right_w"], m["pixel_down_w"]
        p["src_kf"], p["src_level"] = 0, m["src_level"]
        c = np.asarray(m["center"], np.int32).reshape(n, 2)
        p["center_x"], p["center_y"] = c[:, 0], c[:, 1]
        h["sources"]["src_kf"] = 0
        h["points3"] = np.ascontiguousarray(p["pv"]["world"])
        h["poses"] = np.ascontiguousarray(kf_poses)
        self.n0 = n
        self.rmap = uploaded(self.ctx_m, h, list(self.kfs))
        self.snap = host.MapSnapshot(self.ctx_m, CAP)
        self.snap.enable_keyframes(MAX_KF)
        self.finder = host.ReFinder(self.ctx_m)
        self.mm = host.MapMaker(self.ctx_m, self.rmap, self.finder, self.snap, mm_opts(self.ctx_m) if mm_opts else None)
        self.rmap.publish(self.snap)
        blank = np.full(frames[0].shape, 128, np.uint8)
        self.d_frames = [host.DevBuf(self.ctx_t, np.ascontiguousarray(f)) for f in frames]
        self.d_blank = host.DevBuf(self.ctx_t, blank)
        self.tracker = None

    def close(self):
        if self.tracker is not None:
            self.tracker.close()
        self.mm.close()
        for d in self.d_frames + [self.d_blank]:
            d.free()
        for x in [self.finder, self.snap, self.rmap] + self.kfs:
            x.close()
        self.ctx_t.close()
        self.ctx_m.close()


class RefCameraTracker:
    """host.CameraTracker's frame from the existing calls; the same keyword options"""

    def __init__(self, ctx, snapshot, mapmaker, keyframe_gap=20, max_queue=3, shuffle_seed=0, tag_base=0, reports=8, keyframes=32,
                 use_rotation_estimator=1, state=None, max_points=CAP, max_keyframes=MAX_KF):
        self.ctx, self.lib, self.snapshot, self.mm = ctx, ctx.lib, snapshot, mapmaker
        self.gap, self.max_queue, self.seed, self.tag_base = keyframe_gap, max_queue, shuffle_seed, tag_base
        self.tr = host.Tracker(ctx, max_points)
        self.kf = host.KeyFrame(ctx)
        self.est = host.RotationEstimator(ctx) if use_rotation_estimator else None
        self.rel = host.Relocaliser(ctx, max_keyframes)
        self.state_opts = self.tr.state_opts(**(state or {}))
        self._state = self.tr.track_state(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
        self.free_reports = [host.FrameReport(ctx, max_points) for _ in range(reports)]
        self.out, self.n_keyframes, self.clones = {}, keyframes, []
        self.last_report = None

    def reset(self, pose):
        self._state = self.tr.track_state(pose)
        if self.est is not None:
            self.est.reset()
        self.rel.clear()
        self.free_reports += list(self.out.values())
        self.out, self.clones = {}, []

    def state(self):
        return self._state

    def pool(self):
        return len(self.free_reports), self.n_keyframes - len(self.clones)

    def TrackFrame(self, d_frame):
        for tag in self.mm.released():
            if tag in self.out:
                self.free_reports.append(self.out.pop(tag))
        take = self.tr.take_map(self.snapshot)
        kf_take = self.rel.take_keyframes(self.snapshot)
        n, s = self.tr.n, self._state
        tag = self.tag_base + s.frame
        self.tr.set_shuffle(*[host.shuffle_order(self.lib, self.seed, s.frame, w, n) for w in (0, 1)])
        res, infos = host.Tracker.track_frames_recover_batch([self.tr], [self.kf], [d_frame], [s], [self.est], [self.rel], None, self.state_opts)
        f = infos[0]
        rep = self.free_reports[0]
        empty = dict(map_id=0, tag=0, n_records=0, n_entries=0, n_outliers=0)
        info = empty if f["branch"] == FAILED else self.tr.report_frame(rep, tag)
        queue = self.mm.QueueSize()
        what = decide(f["branch"], s.quality, s.frame, s.last_keyframe_dropped, self.gap, queue, self.max_queue, info["n_records"])
        if what == "add":
            clone = self.kf.clone()
            self.ctx.sync()
            self.clones.append(clone)
            self.mm.AddKeyFrame(clone, res[0]["pose"], 0, rep, s.model.scene_depth_mean, s.model.scene_depth_sigma, tag)
            s.last_keyframe_dropped = s.frame
        elif what == "note":
            self.mm.NoteFrame(rep, tag)
        if what:
            self.out[tag] = self.free_reports.pop(0)
        self.last_report = rep
        return dict(track=res[0], branch=f["branch"], quality=s.quality, lost_frames=s.lost_frames, frame=s.frame, report=info, map_take=take,
                    keyframes_take=kf_take, added_keyframe=int(what == "add"), noted_frame=int(what == "note"), queue_size=queue, tag=tag,
                    info=f)

    def close(self):
        for r in self.free_reports + list(self.out.values()):
            r.close()
        for x in [self.rel, self.kf, self.tr] + ([self.est] if self.est else []):
            x.close()
