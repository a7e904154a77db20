"""Times a trail-stage frame of a session — MakeKeyFrame_Lite of a device-resident frame and TrailTracking_Advance — for 1 and 16
cameras (each in its own context) at 640x480 on synth.make_tracking_frames, and prints one JSON line:
  batch_us      ptam_trails_advance_batch: one chain for all cameras, per frame of the call (all cameras together)
  baseline_us   ptam_make_keyframe_lite_dev + ptam_trails_advance camera by camera, per frame (all cameras together)
Order batch, baseline, baseline, batch; each figure the median of --passes passes over the sequence with min and max; a pass starts
the trails again on frame 0, so every pass sees the same live counts (printed).  Host clock around the calls.
  poke_to_tracked_us   a whole session at 640x480 on the rendered stereo sequence of tests/init_map_ref.py at half its step (the
                       pixel motion of the 320x240 sequence: at the full step the trails die), pokes at frames 0 and 10:
                       from the call with the second poke to the end of the first tracked frame, one thread — the frame that leaves
                       the request (ptam_trails_read, two keyframe copies, ptam_mapmaker_request_init), the mapmaker's step
                       (InitFromStereo and the publish) and the first tracked frame (the poll, the takes, the chain) — each also
                       on its own; the median of --sessions sessions after one warm-up session, min and max"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import host, synth  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402
from tests import init_map_ref as IR  # noqa: E402


class Camera:
    def __init__(self, lib, frames, threshold):
        self.lib, self.thr, self.first = lib, threshold, frames[0]
        self.ctx = host.Context(lib=lib)
        self.kf = host.KeyFrame(self.ctx)
        self.tr = host.Trails(self.ctx, 1000)
        self.dev = [host.DevBuf(self.ctx, f) for f in frames]

    def start(self):
        self.kf.MakeKeyFrame_Lite(self.first)
        self.kf.MakeKeyFrame_Rest()
        n = self.tr.start(self.kf, self.thr, 1000)
        self.ctx.sync()
        return n


def one_pass(cams, n_frames, batch):
    """-> (us per frame, the first camera's live counts)"""
    for c in cams:
        c.start()
    alive, t = [], 0.0
    for k in range(1, n_frames):
        t0 = time.perf_counter()
        if batch:
            got = host.Trails.advance_batch([c.tr for c in cams], [c.kf for c in cams], [c.dev[k] for c in cams])
        else:
            got = []
            for c in cams:
                c.ctx._check(c.lib.make_keyframe_lite_dev(c.ctx.h, c.kf.h, c.dev[k].p), "make_keyframe_lite_dev")
                got.append(c.tr.advance(c.kf))
        t += time.perf_counter() - t0
        alive.append(got[0][1])
    return t * 1e6 / (n_frames - 1), alive


def poke_to_tracked(lib, sessions):
    size = (640, 480)
    frames = IR.stereo_sequence(size=size, n_frames=12, step=IR.STEP / 2)[0]
    ctx_m, ctx_t = host.Context(lib=lib, size=size), host.Context(lib=lib, size=size)
    rmap, finder, snap = host.ResidentMap(ctx_m), host.ReFinder(ctx_m), host.MapSnapshot(ctx_m, 16384)
    snap.enable_keyframes(16)
    mm = host.MapMaker(ctx_m, rmap, finder, snap, host.MapMaker.mapmaker_opts(ctx_m))
    h = host.CameraTracker(ctx_t, snap, mm, max_points=16384, max_keyframes=16, keyframes=8)
    h.EnableSession(init=rmap.init_opts(max_bundles=20))
    dev = [host.DevBuf(ctx_t, np.ascontiguousarray(f)) for f in frames]
    rows, info = [], {}
    for n in range(sessions + 1):
        h.SessionFrame(dev[0], poke=True)
        for k in range(1, 10):
            h.SessionFrame(dev[k])
        ctx_t.sync()
        t0 = time.perf_counter()
        s = h.SessionFrame(dev[10], poke=True)[1]
        t1 = time.perf_counter()
        step = mm.Step()
        t2 = time.perf_counter()
        t, s2 = h.SessionFrame(dev[11])
        t3 = time.perf_counter()
        info = {"trails": s["n_trails"], "init_status": s2["init_status"], "tracked": s2["tracked"], "step_status": step["status"],
                "map_points": rmap.counts()["n_points"], "found": int(sum(t["track"]["found"])) if t else 0}
        assert s["init_requested"] and s2["tracked"], (s, s2)
        if n:
            rows.append([(t3 - t0) * 1e6, (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6])
        mm.RequestReset()            # Tracker::Reset: the mapmaker's side, then the tracker's
        mm.Step()
        mm.released()
        h.Restart()
    out = dict(info)
    for i, name in enumerate(("poke_to_tracked_us", "request_frame_us", "step_us", "first_tracked_frame_us")):
        v = [r[i] for r in rows]
        out[name] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    h.close()
    mm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--threshold", type=float, default=70.0)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--cameras", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--sessions", type=int, default=5)
    a = ap.parse_args()
    seq = synth.make_tracking_frames(n_frames=a.frames)
    frames = [np.ascontiguousarray(f) for f in (seq["frames"] if isinstance(seq, dict) else seq[0])]
    lib = load()
    cams = [Camera(lib, frames, a.threshold) for _ in range(max(a.cameras))]
    res = {"frames": a.frames, "passes": a.passes}
    for nc in a.cameras:
        sub = cams[:nc]
        one_pass(sub, a.frames, True)
        one_pass(sub, a.frames, False)          # (warm: kernels loaded, the job table allocated)
        legs = []
        for name, batch in (("batch", True), ("baseline", False), ("baseline", False), ("batch", True)):
            runs = [one_pass(sub, a.frames, batch) for _ in range(a.passes)]
            us = [r[0] for r in runs]
            assert all(r[1] == runs[0][1] for r in runs)
            legs.append({"leg": name, "median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)})
            alive = runs[0][1]
        res["cameras_%d" % nc] = {"legs": legs, "trails_alive": alive}
    res["session"] = poke_to_tracked(lib, a.sessions)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
