"""-m gpu: builds examples/tracker_demo.cc (ptam::Tracker and ptam::MapMaker of ptam_shim.hpp: a tracker thread and a mapmaker thread
over one resident map, 20 frames) with g++ and runs it on the scene of tests/test_gpu_insert_keyframe.py written to a file.  The
threads interleave freely, so what is compared with the same sequence through host.CameraTracker is what no interleaving can change
— the first frame, taken from the map as uploaded — and what must hold at the end: one keyframe added and in the map, every other
frame noted, every tag home, the measurement table in order."""
import os
import re
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, uploaded  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 20


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tracker_demo") / "tracker_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "tracker_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def python_first_frame(d):
    """the demo's first frame through host.CameraTracker, no mapmaker step in between"""
    ctx = d["ctx"]
    cap = len(d["h"]["points3"]) + 4096
    m = uploaded(ctx, d["h"], d["kfs"])
    rf, snap = host.ReFinder(ctx), host.MapSnapshot(ctx, cap)
    snap.enable_keyframes(16)
    m.publish(snap)
    mm = host.MapMaker(ctx, m, rf, snap, host.MapMaker.mapmaker_opts(ctx, ba=dict(deterministic=1), min_shi_tomasi=I.THRESHOLD))
    tr = host.CameraTracker(ctx, snap, mm, max_points=cap, max_keyframes=16, shuffle_seed=7, reports=FRAMES + 2, keyframes=4)
    tr.reset(d["sp"])
    d_frame = host.DevBuf(ctx, np.ascontiguousarray(I.views()["ia"]))
    r = tr.TrackFrame(d_frame)
    out = (int(sum(r["track"]["found"])), int(sum(r["track"]["attempted"])), r["report"]["n_records"], r["added_keyframe"], r["map_take"]["n_points"])
    tr.close()
    mm.close()
    d_frame.free()
    for x in (snap, rf, m):
        x.close()
    return out


def test_two_threads_through_the_shim(dev, demo, tmp_path):
    h, sp = dev["h"], dev["sp"]
    found, attempted, records, added, n_points = python_first_frame(dev)
    assert added == 1 and records > 20
    v = I.views()
    height, width = v["ia"].shape
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), 0, width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp):
            f.write(np.ascontiguousarray(a).tobytes())
    p = subprocess.run([demo, fin], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.strip().split("\n")
    frames = [ln for ln in lines if ln.startswith("FRAME ")]
    assert len(frames) == FRAMES
    assert frames[0] == "FRAME 0 tracked found %d / %d records %d in-chain 1 added queue 0 map-points %d" % (found, attempted, records, n_points), frames[0]
    # 20 frames and the reference's gap of 20: the first frame becomes a keyframe, every other frame is noted
    assert all(re.match(r"FRAME %d tracked found \d+ / \d+ records \d+ in-chain 1 noted queue [01] map-points \d+$" % k, frames[k]) for k in range(1, FRAMES)), frames
    m = re.match(r"TRACKERDEMO rc 0 frames 20 added 1 noted 19 quality 1 lost 0 kf (\d+) points (\d+) meas (\d+) queue 0 free-reports (\d+) free-keyframes 3$", lines[-1])
    assert m, lines[-1]
    assert int(m.group(1)) == K0 + 1 and int(m.group(2)) > 100 and int(m.group(4)) == FRAMES + 2 - 1
