"""-m gpu: builds examples/insert_keyframe_demo.cc (ptam::ResidentMap::InsertKeyFrame / ClosestKeyFrames of ptam_shim.hpp) with g++,
runs it on the scene of tests/test_gpu_insert_keyframe.py written to a file, and checks its output file against
host.ResidentMap.InsertKeyFrame / ClosestKeyFrames on the same map, byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests import insert_keyframe_ref as I
from tests.test_gpu_insert_keyframe import K0, dev, one_call  # noqa: F401  (dev: the module's fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("insert_keyframe_demo") / "insert_keyframe_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "insert_keyframe_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_matches_python_calls(dev, demo, tmp_path):
    h, rows, sp = dev["h"], dev["rows"], dev["sp"]
    res, tab, _, m, rf = one_call(dev)
    idx, dist = m.ClosestKeyFrames(res["kf"], K0)
    counts = m.counts()
    rf.close()
    m.close()

    v = I.views()
    height, width = v["ia"].shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K0, len(h["points3"]), len(h["meas"]), len(h["new_queue"]), len(rows), width, height, -1], np.int32).tobytes())
        f.write(np.array([I.DEPTH["depth_mean"], I.DEPTH["depth_sigma"], I.THRESHOLD], np.float64).tobytes())
        for a in (v["ib"], v["ic"], v["ia"], h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["new_queue"], sp, rows):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("INSERTKEYFRAME kf %d target %d refound %d never %d made %d first %d points %d meas %d closest %d " % (
        res["kf"], res["target_kf"], res["refind"]["n_found"], res["refind"]["n_never"], res["n_made"], res["first_point"], counts["n_points"],
        counts["n_meas"], idx[0])), out
    raw = open(fout, "rb").read()
    r = host._abi.RmapInsertResult.from_buffer_copy(raw[:ctypes.sizeof(host._abi.RmapInsertResult)])
    assert (r.kf, r.target_kf, r.first_point, r.n_made) == (res["kf"], res["target_kf"], res["first_point"], res["n_made"])
    assert r.target_dist == res["target_dist"] and host._counts(r.refind) == res["refind"]
    assert bytes(r.levels) == res["levels"].tobytes()
    want = [np.array([len(idx)], np.int32), idx, dist, np.array([counts[k] for k in ("n_kf", "n_points", "n_meas", "n_never", "n_new", "n_failure")], np.int32)]
    want += [tab[k] for k in host.ResidentMap.TABLES]
    assert raw[ctypes.sizeof(host._abi.RmapInsertResult):] == b"".join(np.ascontiguousarray(w).tobytes() for w in want)
    assert res["n_made"] > 0 and res["target_kf"] == I.TARGET and idx.tolist() == [I.TARGET, I.THIRD, I.DECOY]
