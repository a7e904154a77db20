"""-m gpu: builds examples/map_ba_demo.cc (ptam::MapBundleAdjust of ptam_shim.hpp, std::vector tables) with g++, runs it on map
tables written by the test, and checks its results against the Python call host.map_bundle_adjust on the same tables."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import map_ba_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_ba_demo") / "map_ba_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "map_ba_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.mark.parametrize("mode", [_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL])
def test_shim_matches_python_call(hip, demo, tmp_path, mode):
    poses, fixed, points, meas = R.map_from_problem(synth.make_ba_problem(14, 900, 21, window=6), seed=21, extra_fixed=(5,))
    meas = np.ascontiguousarray(meas, host.MAP_MEAS_DT)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([mode, len(poses), len(points), len(meas)], np.int32).tobytes())
        f.write(poses.tobytes() + fixed.tobytes() + points.tobytes() + meas.tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("MAPBA ran 1")
    ctx = host.Context(lib=hip)
    ref = host.map_bundle_adjust(ctx, mode, poses, fixed, points, meas, deterministic=1)
    ctx.close()
    raw = open(fout, "rb").read()
    res = np.frombuffer(raw[:32], np.int32)
    assert list(res) == [ref[k] for k in ("ran", "accepted", "converged", "n_adjust", "n_fixed", "n_points", "n_meas", "n_outliers")]
    o = 32
    for key, nbytes in (("poses", poses.nbytes), ("points", points.nbytes), ("outliers", ref["outliers"].nbytes),
                        ("cam_kf", ref["cam_kf"].nbytes), ("point_ids", ref["point_ids"].nbytes)):
        assert raw[o:o + nbytes] == ref[key].tobytes(), key
        o += nbytes
    assert o == len(raw) and ref["accepted"] > 0
