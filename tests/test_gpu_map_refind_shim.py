"""-m gpu: builds examples/map_refind_demo.cc (ptam::MapReFind of ptam_shim.hpp, std::vector tables) with g++, runs it on map
tables written by the test, and checks its results against the Python call host.map_refind on the same tables."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import map_refind_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_refind_demo") / "map_refind_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "map_refind_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.mark.parametrize("mode", [_abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE], ids=["new_points", "failure_queue"])
def test_shim_matches_python_call(hip, demo, tmp_path, mode):
    ctx = host.Context(lib=hip)
    scene = R.make_scene(ctx)
    points, work = R.make_work(mode, scene)
    rf = host.ReFinder(ctx)
    ref = host.map_refind(ctx, rf, mode, scene["kfs"], scene["poses"], points, scene["meas"], scene["never"], work)
    rf.close()
    a, b = synth.make_frame_pair()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([mode, len(scene["kfs"]), len(points), len(scene["meas"]), len(scene["never"]), len(work), b.shape[1], b.shape[0]],
                         np.int32).tobytes())
        f.write(np.ascontiguousarray(b, np.uint8).tobytes() + np.ascontiguousarray(a, np.uint8).tobytes())
        f.write(scene["poses"].tobytes() + points.tobytes() + scene["meas"].tobytes() + scene["never"].tobytes() + work.tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("MAPREFIND pairs %d " % ref["n_pairs"])
    raw = open(fout, "rb").read()
    assert list(np.frombuffer(raw[:32], np.int32)) == [ref[k] for k in R.COUNTS]
    o = 32
    for key in ("found", "found_subpix", "never", "meas_merged", "never_merged"):
        assert raw[o:o + ref[key].nbytes] == ref[key].tobytes(), key
        o += ref[key].nbytes
    assert o == len(raw) and ref["n_found"] > 0 and ref["n_never"] > 0 and ref["n_skipped"] > 0
    scene["close"]()
    ctx.close()
