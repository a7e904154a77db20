"""Times ptam_camera_tracker_track_frames — one frame of Tracker::TrackFrame for a good map with its hand-over as one call — over the
closed 64-frame sequence (1 244 points; --tile T: the map T times over, 41: 51 004 points), and prints one JSON line.  Every camera has
its own resident map, snapshot, MapMaker and handle.  Per --nb cameras, us per frame of
  handle    ptam_camera_tracker_track_frames for all cameras: released tags, the two takes (polls), the chain with the draw and the
            report, the decision, ptam_mapmaker_note_frame or ptam_kf_copy + ptam_mapmaker_add_keyframe
The host clock runs around the handle's calls only.  Every 8 steps, outside the clock, each camera's MapMaker takes Step()s until its
keyframe queue is empty (at most max_queue + 1): the notes are counted, queued keyframes go into the map, the tags come back.
Reported: the median of --passes passes of 64 steps after one warm-up pass, min / max, and what the frames did.  The composed sequence
of calls this replaces, and the chain alone, are timed by time_report_chain.py (same sequence, same map, same clock)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ptam_cg_amd import host, synth  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402
from time_report_chain import N_FRAMES, map_tables  # noqa: E402


class Cam:
    def __init__(self, lib, kim, kpose, tile):
        self.ctx_m, self.ctx_t = host.Context(lib=lib), host.Context(lib=lib)
        self.kf0 = host.KeyFrame(self.ctx_m).MakeKeyFrame_Lite(kim)
        m = synth.make_sequence_map([self.kf0.level(l) for l in range(4)], kpose)
        if tile > 1:
            m = {k: np.concatenate([v] * tile) for k, v in m.items() if k not in ("shuffle_levels", "shuffle_fine")}
        self.n = len(m["world"])
        t = map_tables(m)
        t["poses"] = np.ascontiguousarray(kpose).reshape(1, 12)
        self.rmap = host.ResidentMap(self.ctx_m)
        self.rmap.upload(kfs=[self.kf0], **t)
        self.snap = host.MapSnapshot(self.ctx_m, 2 * self.n + 16384)
        self.snap.enable_keyframes(64)
        self.finder = host.ReFinder(self.ctx_m)
        self.mm = host.MapMaker(self.ctx_m, self.rmap, self.finder, self.snap, host.MapMaker.mapmaker_opts(self.ctx_m))
        self.rmap.publish(self.snap)
        self.tr = host.CameraTracker(self.ctx_t, self.snap, self.mm, max_points=2 * self.n + 16384, max_keyframes=64, shuffle_seed=1, reports=16, keyframes=64,
                                     keyframe_gap=40)      # (two keyframes a pass: the map's 64 keyframes last for 16 passes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--tile", type=int, default=1)
    a = ap.parse_args()
    lib = load()
    frames, poses, kim, kpose = synth.make_tracking_frames(N_FRAMES, period=N_FRAMES)
    cams = [Cam(lib, kim, kpose, a.tile) for _ in range(max(a.nb))]
    d_frames = [host.DevBuf(cams[0].ctx_t, f) for f in frames]       # (device memory: every context of the device reads it)
    out = {"passes": a.passes, "frames_per_pass": N_FRAMES, "points": cams[0].n, "nb": {}}
    for nb in a.nb:
        cs = cams[:nb]
        stride = max(1, N_FRAMES // nb)
        first = [(i * stride) % N_FRAMES for i in range(nb)]
        times, tally = [], {"added": 0, "noted": 0, "lost": 0, "in_chain": 0, "frames": 0}
        for rep in range(a.passes + 1):
            for i, c in enumerate(cs):
                c.tr.reset(poses[(first[i] - 1) % N_FRAMES])
            dt = 0.0
            for s in range(N_FRAMES):
                ds = [d_frames[(first[i] + s) % N_FRAMES] for i in range(nb)]
                t0 = time.perf_counter()
                res = host.CameraTracker.track_frames([c.tr for c in cs], ds)
                dt += time.perf_counter() - t0
                if rep:
                    for r in res:
                        tally["added"] += r["added_keyframe"]
                        tally["noted"] += r["noted_frame"]
                        tally["lost"] += int(r["track"]["n_meas"] < 50)
                        tally["in_chain"] += r["report_in_chain"]
                        tally["frames"] += 1
                if s % 8 == 7:
                    for c in cs:
                        for _ in range(4):
                            c.mm.Step()
            if rep:
                times.append(dt)
        per = lambda t: round(t / (nb * N_FRAMES) * 1e6, 2)
        row = {"handle": {"us_per_frame": per(statistics.median(times)), "us_per_frame_min_max": [per(min(times)), per(max(times))], **tally}}
        out["nb"][str(nb)] = row
        print("nb", nb, json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
