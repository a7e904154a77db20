"""-m gpu: builds examples/frame_report_demo.cc (ptam::FrameReport, MapTracker::ReportFrame, ResidentMap::NoteTracked(report) and
the InsertKeyFrame overload of ptam_shim.hpp; a tracker and a mapmaker thread, a pool of two reports between them) with g++, runs
it on the scene of tests/test_gpu_insert_keyframe.py written to a file, and checks its output file against the same sequence
through host.*, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, uploaded  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_report_demo") / "frame_report_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "frame_report_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def python_sequence(d):
    """what the demo's two threads do, through the Python wrappers in one thread, a fresh report per frame"""
    ctx, rows = d["ctx"], d["rows"]
    m = uploaded(ctx, d["h"], d["kfs"])
    rf, snap, tr = host.ReFinder(ctx), host.MapSnapshot(ctx, 8192), host.Tracker(ctx, 8192)
    m.publish(snap)
    pts = np.repeat(rows["point"][::5], 21).astype(np.int32)
    m.note_tracked(pts, np.ones(len(pts), np.uint8))
    tr.take_map(snap)
    per_frame, tail, first = [], [0, 0, 0, 0], None
    for frame in range(FRAMES):
        tr.TrackMap(d["ka"], d["sp"])
        rep = host.FrameReport(ctx, 8192)
        info = tr.report_frame(rep, tag=frame)
        if frame == 0:
            first = rep.read()
        note = m.note_reports([rep])
        per_frame.append([info["tag"], info["n_records"], info["n_outliers"], note["n_gone"]])
        if frame == 1:
            tail[0] = m.handle_bad_points()["n_removed"]
        if frame == FRAMES - 1:
            o = m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH)
            r = m.InsertKeyFrame(rf, d["ka"], d["sp"], 0, opts=o, report=rep)
            tail[1:] = [r["n_rows"], r["n_gone"], r["n_made"]]
        rep.close()
    c = m.counts()
    out = [np.array(per_frame, np.int32), np.array(tail, np.int32), np.array([c["n_points"], c["n_meas"]], np.int32),
           m.download("outlier_count"), m.download("inlier_count"), m.download("meas"), m.point_serials(), first]
    for x in (tr, snap, rf, m):
        x.close()
    return per_frame, tail, c, out


def test_shim_matches_python_calls(dev, demo, tmp_path):
    h, rows, sp = dev["h"], dev["rows"], dev["sp"]
    per_frame, tail, c, want = python_sequence(dev)
    v = I.views()
    height, width = v["ia"].shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), len(rows), width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp, rows):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("FRAMEREPORT frames %d records %d gone %d removed %d rows %d rows-gone %d made %d points %d meas %d" % (
        FRAMES, per_frame[-1][1], per_frame[-1][3], tail[0], tail[1], tail[2], tail[3], c["n_points"], c["n_meas"])), out
    assert open(fout, "rb").read() == b"".join(np.ascontiguousarray(w).tobytes() for w in want)
    # the sequence is worth comparing: points went between the reports, the keyframe got rows and made points
    assert [r[0] for r in per_frame] == list(range(FRAMES)) and all(r[1] > 20 for r in per_frame)
    assert per_frame[0][3] == per_frame[1][3] == 0 < per_frame[2][3] == per_frame[3][3] < per_frame[3][1]
    assert tail[0] > 0 and tail[1] > 0 and tail[2] == per_frame[3][3] and tail[3] > 0
