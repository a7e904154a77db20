"""CPU: the Python side of ptam_track_frames_report_batch, ptam_tracker_draw_shuffles / _read_shuffle and ptam_kf_copy against the header —
the struct the report batch fills, the symbols, and the refusals that need no device (they are decided before the first HIP call)."""
import ctypes as C
import os
import re

from ptam_cg_amd import _abi
from ptam_cg_amd._lib import load

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ptam_hip.h")
E_ARG = -1


def test_report_info_is_the_header_struct():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} ptam_track_report_info;", text).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    assert fields == [("ptam_frame_report_info_t", "report"), ("int32_t", "report_in_chain"), ("int32_t", "report_too_small")]
    assert [f[0] for f in _abi.TrackReportInfo._fields_] == [name for _, name in fields]
    assert C.sizeof(_abi.TrackReportInfo) == C.sizeof(_abi.FrameReportInfo) + 8 == 40
    assert _abi.TrackReportInfo.report_in_chain.offset == 32


def test_the_entries_are_declared_and_exported():
    text = open(HEADER).read()
    lib = load()
    for name in ("track_frames_report_batch", "tracker_draw_shuffles", "tracker_read_shuffle", "shuffle_order_host", "kf_copy"):
        assert re.search(r"\bint\s+ptam_%s\(" % name, text), name
        assert name in _abi.PROTOTYPES and lib.has(name), name
    # the report batch takes the recover batch's twelve arguments and four more
    assert len(_abi.PROTOTYPES["track_frames_report_batch"][1]) == len(_abi.PROTOTYPES["track_frames_recover_batch"][1]) + 4
    assert _abi.PROTOTYPES["track_frames_report_batch"][1][:12] == _abi.PROTOTYPES["track_frames_recover_batch"][1]


def test_null_handles_are_refused():
    lib = load()
    buf = (C.c_int32 * 4)()
    assert lib.kf_copy(None, None, None) == E_ARG
    assert lib.tracker_draw_shuffles(None, 1, 2) == E_ARG
    assert lib.tracker_read_shuffle(None, buf, buf) == E_ARG
    assert lib.track_frames_report_batch(1, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None) == E_ARG
    assert b"bad argument" in lib.last_error()
