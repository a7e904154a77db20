"""CPU: the frame report's host side (ptam_frame_report_*, ptam_tracker_report_frames, ptam_rmap_note_reports,
ptam_rmap_insert_keyframe_report; their structs and argument counts are checked with the whole header in tests/test_abi.py): the
built library exports each of them and host.py wraps them."""
import inspect

from ptam_cg_amd import host

ENTRIES = ("frame_report_create", "frame_report_destroy", "frame_report_info", "frame_report_read", "frame_report_from_host",
           "tracker_report_frames", "rmap_note_reports", "rmap_insert_keyframe_report")


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.FrameReport, ("info", "read", "from_host", "close")), (host.Tracker, ("report_frame", "report_frames")),
                       (host.ResidentMap, ("note_reports", "InsertKeyFrame"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert "report" in inspect.signature(host.ResidentMap.InsertKeyFrame).parameters
