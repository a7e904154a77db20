"""-m gpu: builds examples/mapmaker_demo.cc (ptam::MapMaker of ptam_shim.hpp) with g++ and runs it on the scene of
tests/test_gpu_insert_keyframe.py written to a file.  Part 1, one thread: what every Step() prints and the tables it leaves are
those of the same sequence through host.MapMaker.  Part 2, a tracker thread calling AddKeyFrame / NoteFrame and a mapmaker thread
in Run(), a context each: the demo checks its invariants itself (every tag released exactly once, every keyframe in the map, the
measurement table in order) and must end, under the time limit given here."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, uploaded  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 8


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapmaker_demo") / "mapmaker_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "mapmaker_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def python_part_one(d):
    """the demo's first part through the Python wrappers -> (the lines it prints, the bytes it writes)"""
    ctx = d["ctx"]
    m = uploaded(ctx, d["h"], d["kfs"])
    rf, snap, own, tr = host.ReFinder(ctx), host.MapSnapshot(ctx, 16384), host.MapSnapshot(ctx, 16384), host.Tracker(ctx, 16384)
    ka = host.KeyFrame(ctx).MakeKeyFrame_Lite(I.views()["ia"])          # no MakeKeyFrame_Rest: the step's business
    m.publish(own)
    tr.take_map(own)
    mm = host.MapMaker(ctx, m, rf, snap, host.MapMaker.mapmaker_opts(ctx, ba=dict(deterministic=1), min_shi_tomasi=I.THRESHOLD, failure_period=1))
    reports = [host.FrameReport(ctx, 16384) for _ in range(2)]
    tr.TrackMap(d["ka"], d["sp"])
    tr.report_frame(reports[0], tag=1)
    mm.NoteFrame(reports[0], 1)
    tr.TrackMap(d["ka"], d["sp"])
    tr.report_frame(reports[1], tag=2)
    pose = d["sp"].copy()
    pose[9] += 0.015
    mm.AddKeyFrame(ka, pose, 0, reports[1], I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], 2)
    lines, steps = [], []
    for step in range(3):
        r = mm.Step()
        c = m.counts()
        steps.append(r)
        lines.append("MAPMAKER step %d status %d stages %d recent %d full %d queue %d draws %d kf %d points %d meas %d never %d new %d failure %d "
                     "rows %d made %d removed %d accepted %d generation %d released%s" % (
                         step, r["status"], r["stages"], r["converged_recent"], r["converged_full"], r["queue_size"], r["draws"], c["n_kf"],
                         c["n_points"], c["n_meas"], c["n_never"], c["n_new"], c["n_failure"], r["insert"]["n_rows"], r["insert"]["n_made"],
                         r["bad_points"]["n_removed"], r["all"]["accepted"], r["publish"]["generation"],
                         "".join(" %d" % t for t in mm.released())))
    out = b"".join(np.ascontiguousarray(x).tobytes() for x in (m.download("meas"), m.download("poses"), m.point_serials()))
    mm.close()
    for x in reports + [tr, own, snap, rf, m, ka]:
        x.close()
    return lines, steps, out


def test_shim_matches_the_python_path_and_the_two_threads_end(dev, demo, tmp_path):
    h, rows, sp = dev["h"], dev["rows"], dev["sp"]
    lines, steps, want = python_part_one(dev)
    # the sequence is worth comparing: the keyframe first and alone, then the new points and the full bundle, then the failure queue
    S = _abi
    assert steps[0]["stages"] == S.MM_STAGE_NOTES | S.MM_STAGE_BAD_POINTS | S.MM_STAGE_ADD_KEYFRAME | S.MM_STAGE_PUBLISH
    assert steps[0]["insert"]["n_rows"] > 20 and steps[0]["insert"]["n_made"] > 0 and lines[0].endswith("released 1 2")
    assert steps[1]["stages"] & S.MM_STAGE_REFIND_NEW and steps[1]["stages"] & S.MM_STAGE_BUNDLE_ALL and steps[1]["stages"] & S.MM_STAGE_BUNDLE_RECENT == 0
    assert steps[1]["refind_new"]["n_pairs"] > 0
    v = I.views()
    height, width = v["ia"].shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), len(rows), width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp, rows):
            f.write(np.ascontiguousarray(a).tobytes())
    p = subprocess.run([demo, fin, fout], capture_output=True, text=True, timeout=120)     # the two-thread part's own time limit
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    got = p.stdout.strip().split("\n")
    assert got[:3] == lines
    assert open(fout, "rb").read() == want
    two = got[3].split()
    assert two[:5] == ["TWOTHREAD", "rc", "0", "frames", str(FRAMES)] and int(two[6]) == K0 + FRAMES // 2 and two[-2:] == ["queue", "0"]
