"""-m gpu: builds examples/calib_demo.cc (ptam::CalibImage / ptam::CameraCalibrator of ptam_shim.hpp) with g++ -Wall, runs it on
grid corners written by the test, and compares its result file byte for byte with the same sequence through
host.CameraCalibrator; the camera.cfg line it saves must parse back to the parameters it returned."""
import os
import re
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import calib_cases as CC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("calib_demo") / "calib_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    out = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "examples", "calib_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                          "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert out.returncode == 0 and "warning" not in out.stderr, out.stderr
    return exe


def g17(values):
    return " ".join("%.17g" % float(v) for v in values)


@pytest.mark.parametrize("disable", [0, 1])
def test_shim_writes_what_the_python_classes_return(hip, demo, tmp_path, disable):
    grids = CC.recover_case(CC.TRUTH_NO_DISTORTION if disable else CC.TRUTH)
    steps_a, steps_b = 3, 40
    fin, fout, fcfg = str(tmp_path / "corners.bin"), str(tmp_path / "result.txt"), str(tmp_path / "camera.cfg")
    with open(fin, "wb") as f:
        f.write(np.array([CC.SIZE[0], CC.SIZE[1], len(grids), steps_a, steps_b, disable], np.int32).tobytes())
        f.write(np.array([len(c) for c, _ in grids], np.int32).tobytes())
        for c, _ in grids:
            f.write(np.ascontiguousarray(c, dtype=host.CALIB_CORNER_DT).tobytes())
    subprocess.check_call([demo, fin, fout, fcfg], timeout=120)

    ctx = host.Context(lib=hip, size=CC.SIZE)
    cal = host.CameraCalibrator(ctx, len(grids), 1 << 16)
    cal.Reset(None, bool(disable))
    lines = []
    for c, _ in grids:
        lines.append("ADDED %d" % (1 if cal.AddImage(c) == _abi.CALIB_GUESS_OK else 0))
    for _ in range(steps_a):
        r = cal.OptimizeOneStep()
        lines.append("STEP %d %s %d" % (r["status"] == _abi.CALIB_OK, g17([cal.MeanPixelError()]), r["n_measurements"]))
    r = cal.Optimize(steps_b)
    lines.append("OPT %d %s %d %s %d" % (r["status"] == _abi.CALIB_OK, g17([r["rms"]]), r["n_measurements"], g17([r["pixel_aspect_ratio"]]),
                                         len(r["history"])))
    params = cal.Params()
    lines.append("PARAMS " + g17(params))
    lines += ["POSE " + g17(p) for p in cal.Poses()]
    lines.append("CFG " + host.calib_cfg_line(params).rstrip("\n"))
    assert open(fout).read() == "\n".join(lines) + "\n"
    assert r["rms"] < 5.0 and len(lines) == 4 + steps_a + 1 + 1 + 4 + 1

    mine = str(tmp_path / "camera_py.cfg")
    cal.SaveCalib(mine)
    assert open(fcfg).read() == open(mine).read()
    m = re.fullmatch(r"Camera\.Parameters=\[ (.*) \]\n", open(fcfg).read())   # the line GVars reads (config/camera.cfg:7)
    assert m and np.array_equal(np.array(m.group(1).split(), dtype=np.float64), params)
    cal.close()
    ctx.close()
