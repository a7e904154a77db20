"""CPU: ptam_track_frames_report_batch, ptam_tracker_draw_shuffles / _read_shuffle and ptam_kf_copy (their structs and argument counts
are checked with the whole header in tests/test_abi.py): the report batch takes the recover batch's arguments and four more, and the
refusals that need no device (they are decided before the first HIP call)."""
import ctypes as C

from ptam_cg_amd import _abi
from ptam_cg_amd._lib import load

E_ARG = -1


def test_the_report_batch_extends_the_recover_batch():
    lib = load()
    for name in ("track_frames_report_batch", "tracker_draw_shuffles", "tracker_read_shuffle", "shuffle_order_host", "kf_copy"):
        assert name in _abi.PROTOTYPES and lib.has(name), name
    # the report batch takes the recover batch's twelve arguments and four more
    assert len(_abi.PROTOTYPES["track_frames_report_batch"][1]) == len(_abi.PROTOTYPES["track_frames_recover_batch"][1]) + 4
    assert _abi.PROTOTYPES["track_frames_report_batch"][1][:12] == _abi.PROTOTYPES["track_frames_recover_batch"][1]
    assert [f for f, _ in _abi.TrackReportInfo._fields_] == ["report", "report_in_chain", "report_too_small"]
    assert _abi.TrackReportInfo._fields_[0][1] is _abi.FrameReportInfo


def test_null_handles_are_refused():
    lib = load()
    buf = (C.c_int32 * 4)()
    assert lib.kf_copy(None, None, None) == E_ARG
    assert lib.tracker_draw_shuffles(None, 1, 2) == E_ARG
    assert lib.tracker_read_shuffle(None, buf, buf) == E_ARG
    assert lib.track_frames_report_batch(1, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None) == E_ARG
    assert b"bad argument" in lib.last_error()
