"""-m gpu: builds examples/report_chain_demo.cc (ptam::MapTracker::TrackFramesReportBatch / DrawShuffles / ShuffleOrder / ReadShuffle and
ptam::KeyFrame::CopyFrom of ptam_shim.hpp) with g++, runs it on the scene of tests/test_gpu_insert_keyframe.py written to a file, and
checks its output file against the same sequence through host.*, byte for byte — the wrapper's own logic with it: what it makes of a
report that is too small for its frame."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, uploaded  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 3
SEED = 0x2545F4914F6CDD1D
E_ARG = -1


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("report_chain_demo") / "report_chain_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "report_chain_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def words(r):
    return np.array([r["tag"], r["n_records"], r["n_entries"], r["n_outliers"], r["report_in_chain"], r["report_too_small"]], np.int64)


def python_sequence(d):
    """what the demo does, through the Python wrappers -> (the output file's pieces, figures to look at)"""
    ctx = d["ctx"]
    ib, ia = I.views()["ib"], I.views()["ia"]
    m = uploaded(ctx, d["h"], d["kfs"])
    cap = len(d["h"]["points3"]) + 4096
    snap, tr = host.MapSnapshot(ctx, cap), host.Tracker(ctx, cap)
    m.publish(snap)
    n = tr.take_map(snap)["n_points"]
    d_frame = host.DevBuf(ctx, np.ascontiguousarray(ia))
    cur, pooled = host.KeyFrame(ctx), host.KeyFrame(ctx).MakeKeyFrame_Lite(ib)
    pooled.MakeKeyFrame_Rest()
    rep = host.FrameReport(ctx, cap)
    state = tr.track_state(d["sp"])
    out, seen = [], []
    first = None
    for frame in range(FRAMES):
        res, infos, rinfos, rc = host.Tracker.track_frames_report_batch([tr], [cur], [d_frame], [state], reports=[rep], tags=[10 + frame],
                                                                        shuffle_seeds=[SEED])
        assert rc == 0
        out += [res[0].tobytes(), bytes(state), words(rinfos[0]).tobytes()]
        seen.append(rinfos[0])
        if frame == 0:
            first, drawn = rep.read(), tr.read_shuffle()
    defined = [host.shuffle_order(ctx.lib, SEED, 0, w, n) for w in (0, 1)]
    out += [first.tobytes(), np.int32(n).tobytes(), drawn[0].tobytes(), drawn[1].tobytes(), defined[0].tobytes(), defined[1].tobytes()]
    assert all(np.array_equal(a, b) for a, b in zip(drawn, defined))
    tr.draw_shuffles(SEED, 77)
    again = tr.read_shuffle()
    assert not np.array_equal(again[0], drawn[0])
    out += [again[0].tobytes(), again[1].tobytes()]
    pooled.copy_from(cur)
    for l in range(4):
        L = pooled.level(l)
        out += [np.int32(len(L["corners"])).tobytes(), L["corners"].tobytes(), L["rowlut"].tobytes()]
        if l == 3:
            out.append(L["im"].tobytes())
    small = host.FrameReport(ctx, seen[-1]["n_records"] - 1)
    res, infos, rinfos, rc = host.Tracker.track_frames_report_batch([tr], [cur], [d_frame], [state], reports=[small], tags=[99],
                                                                    shuffle_seeds=[SEED])
    assert rc == E_ARG and rinfos[0]["report_too_small"] == 1
    out += [np.int64(0).tobytes(), bytes(state), words(rinfos[0]).tobytes(), np.int64(small.info()["n_records"]).tobytes()]
    frame_after = state.frame
    for x in (small, rep, cur, pooled, tr, snap, m):
        x.close()
    d_frame.free()
    return out, seen, n, frame_after


def test_shim_matches_python_calls(dev, demo, tmp_path):
    h, sp = dev["h"], dev["sp"]
    want, seen, n, frame_after = python_sequence(dev)
    v = I.views()
    height, width = v["ia"].shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), 0, width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("REPORTCHAIN frames %d points %d records %d in-chain 1 too-small-delivered 1 state-frame %d" % (
        FRAMES, n, seen[-1]["n_records"], frame_after)), out
    got = open(fout, "rb").read()
    at = 0
    for i, w in enumerate(want):
        assert got[at:at + len(w)] == w, "piece %d of the output differs" % i
        at += len(w)
    assert at == len(got)
    # the sequence is worth comparing: every frame found points and was reported in the chain, and the state moved through the
    # frame whose report was too small
    assert all(r["n_records"] > 20 and r["report_in_chain"] == 1 and r["tag"] == 10 + k for k, r in enumerate(seen))
    assert frame_after == FRAMES + 1 and n > 300
