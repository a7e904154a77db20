"""CPU: the Python side of the calibrator matches include/ptam_hip.h — the structs' fields and sizes and the numbers as a C
compiler reads the header, the argument counts, the defaults — and null handles are refused without touching a device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import calib_ref as CR
from tests.test_mapmaker_abi import header_fields, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)
ENTRIES = {"calib_create": 4, "calib_destroy": 1, "calib_reset": 3, "calib_counts": 3, "calib_add_images": 5, "calib_set_poses": 2,
           "calib_read_poses": 2, "calib_optimize": 4, "calib_params": 2, "calib_residuals": 4}
NUMBERS = {"PTAM_CALIB_OK": 0, "PTAM_CALIB_NO_MEASUREMENTS": 1, "PTAM_CALIB_GUESS_OK": 0, "PTAM_CALIB_GUESS_REFUSED": 1,
           "PTAM_CALIB_MAX_IMAGES": 65536, "PTAM_CALIB_MAX_CORNERS": 4194304, "PTAM_CALIB_MAX_STEPS": 65536}


def test_fields_argument_counts_and_methods():
    assert header_fields("ptam_calib_corner") == [f for f, _ in _abi.CalibCorner._fields_]
    assert header_fields("ptam_calib_result") == [f for f, _ in _abi.CalibResult._fields_]
    for name, n_args in ENTRIES.items():
        args = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == n_args == len(_abi.PROTOTYPES[name][1]), name
        assert _abi.PROTOTYPES[name][0] is ctypes.c_int and name in _abi.DECLARED
    for k, v in NUMBERS.items():
        assert getattr(_abi, k[len("PTAM_"):]) == v, k
    for m in ("Reset", "AddImages", "AddImage", "OptimizeOneStep", "Optimize", "Params", "MeanPixelError", "Poses", "SetPoses",
              "Residuals", "SaveCalib", "close"):
        assert callable(getattr(host.CameraCalibrator, m)), m
    assert host.CALIB_CORNER_DT == synth.CALIB_CORNER_DT == CR.CORNER_DT


def test_sizes_and_numbers_as_a_c_compiler_reads_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    py = {"ptam_calib_corner": _abi.CalibCorner, "ptam_calib_result": _abi.CalibResult}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ptam_hip.h"\nint main(void) {\n'
    src += "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (s, s) for s in py)
    src += "".join('    printf("%s %%d\\n", (int)%s);\n' % (k, k) for k in NUMBERS)
    src += "".join('    printf("off_%s %%zu\\n", offsetof(ptam_calib_result, %s));\n' % (f, f) for f, _ in _abi.CalibResult._fields_)
    src += "    return 0;\n}\n"
    (tmp_path / "sizes.c").write_text(src)
    exe = str(tmp_path / "sizes")
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(tmp_path / "sizes.c"), "-o", exe])
    got = dict((k, int(v)) for k, v in (ln.split() for ln in subprocess.check_output([exe], text=True).strip().split("\n")))
    assert got["ptam_calib_corner"] == ctypes.sizeof(_abi.CalibCorner) == 24 and got["ptam_calib_result"] == ctypes.sizeof(_abi.CalibResult) == 72
    for f, _ in _abi.CalibResult._fields_:
        assert got["off_" + f] == getattr(_abi.CalibResult, f).offset, f
    for k, v in NUMBERS.items():
        assert got[k] == v, k


def test_null_handles_are_refused():
    L = lib()
    h, res, five, word = ctypes.c_void_p(), _abi.CalibResult(), np.full(5, -7.0), ctypes.c_int32(-7)
    pd = five.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.calib_create(None, 4, 64, ctypes.byref(h)) == -1 and not h.value
    assert L.calib_destroy(None) == 0
    assert L.calib_reset(None, None, 0) == -1 and L.calib_counts(None, ctypes.byref(word), ctypes.byref(word)) == -1
    assert L.calib_add_images(None, 1, None, None, None) == -1
    assert L.calib_set_poses(None, pd) == -1 and L.calib_read_poses(None, pd) == -1
    assert L.calib_optimize(None, 1, ctypes.byref(res), None) == -1 and L.calib_params(None, pd) == -1
    assert L.calib_residuals(None, 0, pd, ctypes.byref(word)) == -1
    assert (five == -7.0).all() and word.value == -7 and res.steps == 0


def test_defaults_and_the_config_line():
    assert CR.DEFAULT_PARAMS == (0.5, 0.75, 0.5, 0.5, 0.1)                       # ATANCamera::mvDefaultParams src/ATANCamera.cc:286
    assert "0.5, 0.75, 0.5, 0.5, 0.1" in open(os.path.join(ROOT, "include", "ptam_hip.h")).read()
    line = host.calib_cfg_line(CR.DEFAULT_PARAMS)
    m = re.fullmatch(r"Camera\.Parameters=\[ (.*) \]\n", line)                   # config/camera.cfg:7
    assert m and tuple(float(v) for v in m.group(1).split()) == CR.DEFAULT_PARAMS


def test_make_calib_grids_is_seeded_and_keeps_corners_in_the_image():
    a = synth.make_calib_grids((0.62, 0.83, 0.48, 0.53, 0.9), (640, 480), 3, 8, 6, 7, noise_px=0.0)
    b = synth.make_calib_grids((0.62, 0.83, 0.48, 0.53, 0.9), (640, 480), 3, 8, 6, 7, noise_px=0.0)
    assert len(a) == 3 and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    for c, pose in a:
        assert 4 <= len(c) <= 48 and (c["u"] >= 0).all() and (c["u"] <= 639).all() and (c["v"] >= 0).all() and (c["v"] <= 479).all()
        assert len(set(zip(c["gx"].tolist(), c["gy"].tolist()))) == len(c)
    n = synth.make_calib_grids((0.62, 0.83, 0.48, 0.53, 0.9), (640, 480), 1, 8, 6, 7, noise_px=0.5)
    assert 0 < np.abs(n[0][0]["u"][:4] - a[0][0]["u"][:4]).max() < 5
