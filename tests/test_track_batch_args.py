"""CPU: ptam_track_frames_batch refuses bad arguments before its first HIP call — nb out of range, NULL arrays, a NULL entry — so the
checks run on a machine without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from ptam_cg_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
PTAM_E_ARG = -1


@pytest.fixture(scope="module")
def fn():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(LIB)
    f = lib.ptam_track_frames_batch
    f.restype = C.c_int
    f.argtypes = [C.c_int] + [C.c_void_p] * 8
    return f


def _args(nb=2):
    """arrays of plausible non-null handles (never dereferenced: every call below is refused before that)"""
    dummy = [np.zeros(4096, np.uint8) for _ in range(3 * nb)]
    arr = lambda k: (C.c_void_p * nb)(*[dummy[k * nb + i].ctypes.data for i in range(nb)])
    models = (_abi.MotionModel * nb)()
    out = np.zeros(nb * 256, np.uint8)
    return dict(keep=dummy, trackers=arr(0), current=arr(1), d_frames=arr(2), models=models, out=out)


def _call(fn, nb, a, **over):
    v = dict(trackers=C.cast(a["trackers"], C.c_void_p), current=C.cast(a["current"], C.c_void_p), d_frames=C.cast(a["d_frames"], C.c_void_p),
             models=C.cast(a["models"], C.c_void_p), out=C.c_void_p(a["out"].ctypes.data))
    v.update(over)
    return fn(nb, v["trackers"], v["current"], v["d_frames"], v["models"], None, None, v["out"], None)


def test_batch_sizes_out_of_range_are_refused(fn):
    a = _args()
    assert _call(fn, 0, a) == PTAM_E_ARG
    assert _call(fn, 4097, a) == PTAM_E_ARG
    assert _call(fn, -1, a) == PTAM_E_ARG


def test_null_arrays_are_refused(fn):
    a = _args()
    before = bytes(a["models"])
    for name in ("trackers", "current", "d_frames", "models", "out"):
        assert _call(fn, 2, a, **{name: None}) == PTAM_E_ARG, name
    assert bytes(a["models"]) == before


def test_a_null_entry_is_refused(fn):
    for name in ("d_frames", "trackers", "current"):
        a = _args()
        a[name][1] = None
        assert _call(fn, 2, a) == PTAM_E_ARG, name
