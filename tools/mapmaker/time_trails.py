"""Times the frames before a map exists at 640x480 with up to 1 000 trails on synth.make_tracking_frames and prints one JSON line:
  device_advance_us   ptam_trails_advance per frame (synchronous: two launches, one 16-byte read-back, one wait)
  download_us         what the host path needs first today: ptam_kf_read_level of level 0 (image, corners, row LUT) per frame
  host_loop_us        the reference's loop restated in C++ on the downloaded frames (tools/mapmaker/trails_host.cc, one thread)
  init_points_us      ptam_init_points_from_trails on the surviving trails padded to --matches by repetition
Host clock around each call; medians over the frames / --reps.  The host loop's counts are checked against the device's.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/mapmaker/time_trails.py --frames 12`."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import host, synth  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--stride", type=int, default=1, help="take every stride-th frame of the sequence")
    ap.add_argument("--threshold", type=float, default=70.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--matches", type=int, default=1000)
    a = ap.parse_args()
    seq = synth.make_tracking_frames(n_frames=a.frames * a.stride)
    frames = [np.ascontiguousarray(f) for f in (seq["frames"] if isinstance(seq, dict) else seq[0])][::a.stride]
    ctx = host.Context(lib=load())
    kf = host.KeyFrame(ctx)
    tr = host.Trails(ctx, 1000)
    dev, dl, counts, levels = [], [], [], []
    for k, f in enumerate(frames):
        kf.MakeKeyFrame_Lite(f)
        if k == 0:
            kf.MakeKeyFrame_Rest()
            n0 = tr.start(kf, a.threshold, 1000)
            starts = tr.read()
        else:
            ctx.sync()
            t0 = time.perf_counter()
            counts.append(tr.advance(kf))
            dev.append((time.perf_counter() - t0) * 1e6)
        ctx.sync()
        t0 = time.perf_counter()
        levels.append(kf.level(0))
        dl.append((time.perf_counter() - t0) * 1e6)
    table = tr.read()
    res = {"frames": len(frames), "trails_started": n0, "trails_alive": [c[1] for c in counts],
           "corners_per_frame": int(np.median([len(l["corners"]) for l in levels])),
           "device_advance_us": round(statistics.median(dev), 1), "device_advance_min_us": round(min(dev), 1),
           "download_us": round(statistics.median(dl), 1)}
    with tempfile.TemporaryDirectory() as td:
        exe, fin = os.path.join(td, "trails_host"), os.path.join(td, "frames.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "mapmaker", "trails_host.cc"), "-o", exe])
        with open(fin, "wb") as fp:
            fp.write(np.array([640, 480, len(frames), n0], np.int32).tobytes())
            fp.write(np.stack([starts["initial_x"], starts["initial_y"]], axis=1).astype(np.int32).tobytes())
            for l in levels:
                fp.write(l["im"].tobytes() + np.int32(len(l["corners"])).tobytes() + l["corners"].astype(np.int32).tobytes())
        lines = [l.split() for l in subprocess.check_output([exe, fin], text=True).strip().split("\n")]
    assert [(int(l[0]), int(l[1])) for l in lines] == counts, "the host loop and the device disagree"
    res["host_loop_us"] = round(statistics.median(float(l[2]) for l in lines), 1)
    # part B: the last two frames as the stereo pair, an arbitrary small sideways motion as se3
    first = host.KeyFrame(ctx).MakeKeyFrame_Lite(frames[0])
    m = np.resize(table, a.matches) if len(table) else table
    se3 = np.concatenate([np.eye(3).reshape(9), [-0.1, 0.0, 0.0]])
    ts = []
    for _ in range(a.reps + 3):
        t0 = time.perf_counter()
        pts, st = host.init_points_from_trails(ctx, first, kf, se3, m)
        ts.append((time.perf_counter() - t0) * 1e6)
    res.update(init_points_matches=len(m), init_points_made=len(pts), init_points_us=round(statistics.median(ts[3:]), 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
