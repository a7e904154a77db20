"""CPU: the session entries' host side (their structs, numbers and argument counts are checked with the whole header in
tests/test_abi.py): the wrappers exist, the defaults are the reference's and null handles are refused without a device."""
import ctypes

from ptam_cg_amd import _abi, host
from tests.abi_header import RAW, lib


def test_the_wrappers_exist():
    for cls, methods in ((host.Trails, ("advance_batch",)), (host.MapMaker, ("RequestInit", "InitPoll")),
                         (host.CameraTracker, ("EnableSession", "Restart", "SessionFrame", "session_frames", "stage", "trails", "init_result"))):
        for m in methods:
            assert callable(getattr(cls, m)), m
    assert "TrackForInitialMap (:181) is not here" not in RAW["ptam_hip.h"]


def test_defaults_and_null_handles():
    L = lib()
    o = _abi.CameraSessionOpts()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    assert L.camera_session_opts_default(ctypes.byref(o)) == 0 and L.camera_session_opts_default(None) == -1
    assert (o.max_initial_trails, o.min_good_trails, o.min_shi_tomasi) == (1000, 10, 70.0)        # src/Tracker.cc:360, :329
    init = _abi.RmapInitOpts()
    assert L.rmap_init_opts_default(ctypes.byref(init)) == 0 and bytes(o.init) == bytes(init)
    word, res = ctypes.c_int32(-7), _abi.RmapInitResult()
    assert L.camera_tracker_enable_session(None, ctypes.byref(o)) == -1 and L.camera_tracker_restart(None) == -1
    assert L.camera_tracker_stage(None, ctypes.byref(word)) == -1 and L.camera_tracker_init_result(None, ctypes.byref(res)) == -1
    assert not L.camera_tracker_trails(None) and word.value == -7
    assert L.camera_tracker_session_frames(1, None, None, None, None, None) == -1
    assert L.trails_advance_batch(1, None, None, None, None, None) == -1
    # the mapmaker's two entries touch no device: any non-null handles do
    mm = ctypes.c_void_p()
    zeros = ctypes.create_string_buffer(4096)
    fake = ctypes.c_void_p(ctypes.addressof(zeros))
    assert L.mapmaker_create(fake, fake, None, None, ctypes.byref(mm)) == 0
    assert L.mapmaker_init_poll(mm, ctypes.byref(word), None) == 0 and word.value == _abi.MM_INIT_NONE
    m = (_abi.Trail * 4)()
    assert L.mapmaker_request_init(None, fake, fake, 4, m, None, 1) == -1 and L.mapmaker_request_init(mm, fake, fake, 3, m, None, 1) == -1
    assert L.mapmaker_request_init(mm, fake, fake, 4, m, None, 1) == 0                           # (the zeroed fake map has no keyframe)
    assert L.mapmaker_request_init(mm, fake, fake, 4, m, None, 2) == -3                          # one at a time
    assert L.mapmaker_init_poll(mm, ctypes.byref(word), ctypes.byref(res)) == 0 and word.value == _abi.MM_INIT_PENDING
    assert L.mapmaker_destroy(mm) == 0
