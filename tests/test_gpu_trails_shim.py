"""-m gpu: builds examples/trails_demo.cc (ptam::TrailTracker of ptam_shim.hpp) with g++, runs it on a frame sequence written by
the test, and compares the trail list it prints with host.Trails on the same frames."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host
from tests.test_gpu_trails import H, THRESHOLD, W, _frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trails_demo") / "trails_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "trails_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_prints_the_python_trail_list(hip, demo, tmp_path):
    frames = _frames("drift")
    fin = str(tmp_path / "frames.bin")
    with open(fin, "wb") as f:
        f.write(np.array([W, H, len(frames), 200], np.int32).tobytes() + np.array([THRESHOLD]).tobytes())
        for im in frames:
            f.write(im.tobytes())
    lines = subprocess.check_output([demo, fin], text=True, timeout=120).split("\n")
    ctx = host.Context(lib=hip, size=(W, H))
    kf = host.KeyFrame(ctx)
    tr = host.Trails(ctx, 200)
    want = []
    for k, im in enumerate(frames):
        kf.MakeKeyFrame_Lite(im)
        if k == 0:
            kf.MakeKeyFrame_Rest()
            want.append("START %d" % tr.start(kf, THRESHOLD, 200))
        else:
            want.append("ADVANCE %d %d" % tr.advance(kf))
    table = tr.read()
    want += ["TRAIL %d %d %d %d" % tuple(t) for t in table.tolist()]
    want.append("MATCHES %d" % len(tr.matches()))
    assert len(table) >= 20
    assert [l for l in lines if l] == want
