"""CPU: the Python side of the frame report (ptam_frame_report_*, ptam_tracker_report_frames, ptam_rmap_note_reports,
ptam_rmap_insert_keyframe_report) matches include/ptam_hip.h: every entry bound with as many arguments as the header declares, the
structs of the header's sizes and field order, the built library exports each of them and host.py wraps them."""
import ctypes
import os
import re

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)
ENTRIES = ("frame_report_create", "frame_report_destroy", "frame_report_info", "frame_report_read", "frame_report_from_host",
           "tracker_report_frames", "rmap_note_reports", "rmap_insert_keyframe_report")


def declared(name):
    m = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def struct_fields(name):
    """the fields of `typedef struct { ... } name;` in order -> [(c type, field, array length or None)]"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", HEADER, flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                a = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
                out.append((ctype, a.group(1), int(a.group(2)) if a.group(2) else None))
    return out


def test_every_new_entry_is_bound_with_the_header_s_argument_count():
    for name in ENTRIES:
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == declared(name), (name, len(args), declared(name))
    # every frame-report entry of the header is one of them
    assert sorted(re.findall(r"\bint\s+ptam_(frame_report_[a-z0-9_]+)\s*\(", HEADER)) == sorted(n for n in ENTRIES if n.startswith("frame_report_"))


def test_the_structs_match_the_header():
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8, "double": ctypes.c_double}
    for name, cls, size in (("ptam_frame_record", _abi.FrameRecord, 32), ("ptam_frame_report_info_t", _abi.FrameReportInfo, 32),
                            ("ptam_rmap_note_result", _abi.RmapNoteResult, 8)):
        want = [(f, ctype[t] * n if n else ctype[t]) for t, f, n in struct_fields(name)]
        assert [(f, t) for f, t in cls._fields_] == want, name
        assert ctypes.sizeof(cls) == size, (name, ctypes.sizeof(cls))
    # the numpy record is the ctypes one, field by field
    assert host.FRAME_RECORD_DT.itemsize == ctypes.sizeof(_abi.FrameRecord)
    for f, _ in _abi.FrameRecord._fields_:
        assert host.FRAME_RECORD_DT.fields[f][1] == getattr(_abi.FrameRecord, f).offset, f


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.FrameReport, ("info", "read", "from_host", "close")), (host.Tracker, ("report_frame", "report_frames")),
                       (host.ResidentMap, ("note_reports", "InsertKeyFrame"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    import inspect
    assert "report" in inspect.signature(host.ResidentMap.InsertKeyFrame).parameters
