"""-m gpu: builds examples/publish_map_demo.cc (ptam::MapSnapshot, ResidentMap::Publish / PointSerials / ResolveSerials,
MapTracker::TakeMap / IterationSerials of ptam_shim.hpp, a mapmaker and a tracker thread) with g++, runs it on the scene of
tests/test_gpu_insert_keyframe.py written to a file, and checks its output file against the same sequence through host.*."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, uploaded  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("publish_map_demo") / "publish_map_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "publish_map_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def python_sequence(d):
    """what the demo does, through the Python wrappers, one thread -> (generation, counts, tracker serials, map serials, set serials, indices)"""
    ctx, rows = d["ctx"], d["rows"]
    m = uploaded(ctx, d["h"], d["kfs"])
    rf, snap, tr = host.ReFinder(ctx), host.MapSnapshot(ctx, 8192), host.Tracker(ctx, 8192)
    m.publish(snap)
    pts = np.repeat(rows["point"][::5], 21).astype(np.int32)
    m.note_tracked(pts, np.ones(len(pts), np.uint8))
    row_serials = m.point_serials()[rows["point"]]
    n_removed = m.handle_bad_points()["n_removed"]
    m.publish(snap)
    now, _ = m.resolve_serials(row_serials)
    kept = rows[now >= 0].copy()
    kept["point"] = now[now >= 0]
    o = m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH)
    n_made = m.InsertKeyFrame(rf, d["ka"], d["sp"], 0, kept, o)["n_made"]
    gen = m.publish(snap)["generation"]
    t = tr.take_map(snap)
    tr.TrackMap(d["ka"], d["sp"])
    ser = tr.iteration_serials()
    idx, gone = m.resolve_serials(ser)
    assert gone == 0 and np.array_equal(idx, tr.iteration_set()["point"])
    out = (gen, [t["n_points"], n_removed, n_made, len(kept)], tr.point_serials(), m.point_serials(), ser, idx)
    for x in (tr, snap, rf, m):
        x.close()
    return out


def test_shim_matches_python_calls(dev, demo, tmp_path):
    h, rows, sp = dev["h"], dev["rows"], dev["sp"]
    gen, counts, theirs, ours, ser, idx = python_sequence(dev)
    v = I.views()
    height, width = v["ia"].shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), len(rows), width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp, rows):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("PUBLISHMAP generation 3 points %d removed %d made %d rows %d new-to-fresh %d set %d same-lists 1" % (
        counts[0], counts[1], counts[2], counts[3], counts[0], len(ser))), out
    want = [np.array([gen], np.int64), np.array(counts, np.int32), theirs, ours, np.array([len(ser)], np.int32), ser, idx]
    assert open(fout, "rb").read() == b"".join(np.ascontiguousarray(w).tobytes() for w in want)
    assert gen == 3 and counts[1] > 0 and counts[2] > 0 and 0 < counts[3] < len(rows) and len(ser) > 20
