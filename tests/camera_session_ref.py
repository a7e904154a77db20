"""The session of ptam_camera_tracker_session_frames composed from the calls it is made of, and the scene both sides of
tests/test_gpu_camera_session.py stand on: an EMPTY resident map with its snapshot (keyframe section enabled), finder and host.MapMaker
in the map's context, and the init_map_ref sequence, extended along view_pose, on the device in the tracker's context.  The composed
twin: init_map_ref.run_trails, ResidentMap.InitFromStereo(matches), a publish, and camera_tracker_ref.RefCameraTracker (imported, not
changed) whose state is reset at the tracker's pose with the handle's frame count.  No test lives here."""
import numpy as np

from ptam_cg_amd import host
from tests import init_map_ref as IR
from tests.camera_tracker_ref import CAP, MAX_KF, RefCameraTracker

N_FRAMES = 10                 # the six frames of the stereo sequence and four more along view_pose
INIT = dict(max_bundles=20, homography=dict(seed=3), ba=dict(deterministic=1), plane=dict(seed=5))
THRESHOLD, MAX_TRAILS, MIN_GOOD = 70.0, 1000, 10


def frames():
    return IR.stereo_sequence(n_frames=N_FRAMES)[0]


class Scene:
    def __init__(self, lib, mm_opts=None):
        self.ctx_m, self.ctx_t = host.Context(lib=lib, size=IR.SIZE), host.Context(lib=lib, size=IR.SIZE)
        self.rmap = host.ResidentMap(self.ctx_m)
        self.snap = host.MapSnapshot(self.ctx_m, CAP)
        self.snap.enable_keyframes(MAX_KF)
        self.finder = host.ReFinder(self.ctx_m)
        self.mm = host.MapMaker(self.ctx_m, self.rmap, self.finder, self.snap, mm_opts(self.ctx_m) if mm_opts else None)
        self.frames = frames()
        self.d_frames = [host.DevBuf(self.ctx_t, np.ascontiguousarray(f)) for f in self.frames]
        self.d_blank = host.DevBuf(self.ctx_t, np.full(self.frames[0].shape, 128, np.uint8))
        self.tracker, self.extra = None, []

    def init_opts(self):
        return self.rmap.init_opts(**INIT)

    def close(self):
        for x in [self.tracker] + self.extra:
            if x is not None:
                x.close()
        self.mm.close()
        for d in self.d_frames + [self.d_blank]:
            d.free()
        for x in (self.finder, self.snap, self.rmap):
            x.close()
        self.ctx_t.close()
        self.ctx_m.close()


class RefSession:
    """the twin of a handle with a session, on its own Scene: the trails by the per-camera calls, then the map by the one call"""

    def __init__(self, scene, **opts):
        self.s, self.opts = scene, opts
        self.kf, self.first = host.KeyFrame(scene.ctx_t), host.KeyFrame(scene.ctx_t)
        self.tr = host.Trails(scene.ctx_t, MAX_TRAILS)
        self.frame = 0

    def idle(self):
        self.frame += 1

    def start(self, im):
        self.frame += 1
        self.kf.MakeKeyFrame_Lite(im)
        self.kf.MakeKeyFrame_Rest()
        self.first.copy_from(self.kf)
        return self.tr.start(self.kf, THRESHOLD, MAX_TRAILS)

    def advance(self, im):
        self.frame += 1
        return self.tr.advance(self.kf.MakeKeyFrame_Lite(im))

    def make_map(self):
        """what the mapmaker's step does with the request, then the tracker at the tracker's pose -> the init result"""
        s = self.s
        self.clones = [self.first.clone(), self.kf.clone()]
        s.ctx_t.sync()
        res = s.rmap.InitFromStereo(self.clones[0], self.clones[1], matches=self.tr.read(), opts=s.init_opts())
        s.rmap.publish(s.snap)
        s.tracker = RefCameraTracker(s.ctx_t, s.snap, s.mm, **self.opts)
        return res

    def begin(self, res, frame, last_keyframe_dropped):
        t = self.s.tracker
        t.reset(res["tracker_pose"])
        t.state().frame, t.state().last_keyframe_dropped = frame, last_keyframe_dropped

    def close(self):
        for x in [self.tr, self.kf, self.first] + getattr(self, "clones", []):
            x.close()
