"""CPU: ptam_camera_tracker's host side (its structs and argument counts are checked with the whole header in tests/test_abi.py): the
defaults ptam_camera_tracker_opts_default writes are the reference's (src/Tracker.cc:148-149: 20 frames, a queue of 3;
Tracker.RotationEstimatorBlur 0.75, the estimator on), and null handles are refused without a device."""
import ctypes as C

from ptam_cg_amd import _abi
from ptam_cg_amd._lib import load

E_ARG = -1


def test_the_defaults_are_the_references():
    lib = load()
    o = _abi.CameraTrackerOpts()
    assert lib.camera_tracker_opts_default(C.byref(o)) == 0
    assert (o.keyframe_gap, o.max_queue, o.rotation_blur, o.use_rotation_estimator) == (20, 3, 0.75, 1)
    t, s = _abi.TrackmapOpts(), _abi.TrackStateOpts()
    lib.trackmap_opts_default(C.byref(t))
    lib.track_state_opts_default(C.byref(s))
    assert bytes(o.trackmap) == bytes(t) and bytes(o.state) == bytes(s)
    assert (o.trackmap.coarse_min, o.trackmap.coarse_max, o.trackmap.max_patches) == (20, 60, 1000) and o.state.reloc_blur == 2.5
    assert (o.width, o.height, o.max_points, o.max_keyframes, o.reports, o.keyframes, o.shuffle_seed, o.tag_base, o.pad_) == \
        (640, 480, 8192, 64, 8, 32, 0, 0, 0)
    assert lib.camera_tracker_opts_default(None) == E_ARG


def test_null_handles_are_refused():
    lib = load()
    out, st, a = C.c_void_p(), _abi.TrackState(), C.c_int32()
    pose = (C.c_double * 12)()
    res = (_abi.CameraTrackResult * 1)()
    one = (C.c_void_p * 1)()
    assert lib.camera_tracker_create(None, None, None, None, C.byref(out)) == E_ARG and not out.value
    assert lib.camera_tracker_destroy(None) == 0
    assert lib.camera_tracker_reset(None, pose) == E_ARG
    assert lib.camera_tracker_state(None, C.byref(st)) == E_ARG
    assert lib.camera_tracker_pool(None, C.byref(a), C.byref(a)) == E_ARG
    assert lib.camera_tracker_tracker(None) is None and lib.camera_tracker_current_keyframe(None) is None and lib.camera_tracker_last_report(None) is None
    assert lib.camera_tracker_track_frames(0, one, one, res) == E_ARG
    assert lib.camera_tracker_track_frames(1, one, one, res) == E_ARG            # a null handle in the list
    assert lib.camera_tracker_track_frames(1, None, None, None) == E_ARG
    assert b"bad argument" in lib.last_error()
