"""Times the SmallBlurryImage on the device and prints one JSON line:
  pair_us            ptam_sbi_make of one frame's SBI (sigma 0.75) + ptam_sbi_calc_rotation against the last one (6 iterations): two
                     launches and the mapped wait, on a queue with nothing else on it
  make_us            ptam_sbi_make + ptam_ctx_sync alone
  relocalise_us      ptam_relocalise (make, SSD against every entry, arg-min + alignment: three launches, one wait) at each --banks size;
                     the bank is filled with the sequence's frames over and over
  track_frame_us / track_frame_sbi_us   ptam_track_frame and ptam_track_frame_sbi per frame over the --frames-frame sequence, closed
                     loop (each from its own model, tracker and keyframe); their difference is what the estimator costs a frame
  lost_frames_*      frames with fewer than 50 measurements in those loops
Host clock around each synchronous call; the median of --reps runs after 3 warm-ups (the sequence: the median over its frames after
one warm-up pass).  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/tracking/time_sbi.py --frames 8`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host, synth  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402


def median_us(fn, reps):
    ts = []
    for _ in range(reps + 3):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts[3:]), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--banks", type=int, nargs="+", default=[16, 200])
    a = ap.parse_args()
    lib = load()
    ctx = host.Context(lib=lib)
    frames, poses, kim, kpose = synth.make_tracking_frames(a.frames, period=64)
    kf0 = host.KeyFrame(ctx).MakeKeyFrame_Lite(kim)
    m = synth.make_sequence_map([kf0.level(l) for l in range(4)], kpose)
    d_frames = [host.DevBuf(ctx, f) for f in frames]
    res = {"reps": a.reps, "frames": a.frames}

    kfs = [host.KeyFrame(ctx).MakeKeyFrame_Lite(frames[i]) for i in range(2)]
    last, this = host.SmallBlurryImage(ctx).MakeFromKF(kfs[0], 0.75), host.SmallBlurryImage(ctx)
    al = _abi.SbiAlignment()

    def pair():
        assert lib.sbi_make(this.h, kfs[1].h, 0.75) == 0 and lib.sbi_calc_rotation(this.h, last.h, 6, C.byref(al)) == 0

    def make():
        assert lib.sbi_make(this.h, kfs[1].h, 0.75) == 0 and lib.ctx_sync(ctx.h) == 0

    ctx.sync()
    res["pair_us"], res["make_us"] = median_us(pair, a.reps), median_us(make, a.reps)
    res["pair_n_used"] = al.n_used

    res["relocalise_us"] = {}
    for n in a.banks:
        rel = host.Relocaliser(ctx, n)
        rel.add_batch([kfs[i % 2] for i in range(n)], [poses[i % 2] for i in range(n)])      # one make launch
        ctx.sync()
        res["relocalise_us"][str(n)] = median_us(lambda: rel.AttemptRecovery(kfs[1]), a.reps)
        rel.close()

    def loop(with_sbi):
        tr = host.Tracker(ctx, len(m["world"]))
        tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], kf0, m["src_level"], m["center"])
        kf, est, opts = host.KeyFrame(ctx), host.RotationEstimator(ctx), tr.opts()
        ts, lost = [], 0
        for rep in range(2):                                       # the first pass warms up
            mm = tr.motion_model(poses[0])
            est.reset()
            for k in range(a.frames):
                tr.set_shuffle(m["shuffle_levels"], m["shuffle_fine"])
                t0 = time.perf_counter()
                r = tr.track_frame_sbi(kf, d_frames[k], mm, est, opts)[0] if with_sbi else tr.TrackFrameMoving(kf, d_frames[k], mm, opts)
                if rep:
                    ts.append((time.perf_counter() - t0) * 1e6)
                    lost += int(r["n_meas"] < 50)
        tr.close()
        est.close()
        return round(statistics.median(ts), 1), lost

    res["track_frame_us"], res["lost_frames_track_frame"] = loop(False)
    res["track_frame_sbi_us"], res["lost_frames_track_frame_sbi"] = loop(True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
