"""CPU: the calibrator's host side (its structs, numbers and argument counts are checked with the whole header in tests/test_abi.py):
the wrapper's methods, the defaults, the seeded grids — and null handles are refused without touching a device."""
import ctypes
import re

import numpy as np

from ptam_cg_amd import _abi, host, synth
from tests import calib_ref as CR
from tests.abi_header import RAW, lib


def test_methods_and_the_corner_record():
    for m in ("Reset", "AddImages", "AddImage", "OptimizeOneStep", "Optimize", "Params", "MeanPixelError", "Poses", "SetPoses",
              "Residuals", "SaveCalib", "close"):
        assert callable(getattr(host.CameraCalibrator, m)), m
    assert host.CALIB_CORNER_DT == synth.CALIB_CORNER_DT == CR.CORNER_DT


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
    assert "0.5, 0.75, 0.5, 0.5, 0.1" in RAW["ptam_hip.h"]
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
