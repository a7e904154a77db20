"""CPU: the Python side of the keyframes' publication to the relocaliser (ptam_snapshot_keyframes_enable / _info,
ptam_sbi_bank_take_keyframes / _clear / _read) matches include/ptam_hip.h: every entry bound with as many arguments as the header
declares, the two structs of the header's sizes and field order, the built library exports each of them and the wrappers exist."""
import ctypes

from ptam_cg_amd import _abi, host
from tests.test_map_snapshot_abi import HEADER, declared, struct_fields

ENTRIES = ("snapshot_keyframes_enable", "snapshot_keyframes_info", "sbi_bank_take_keyframes", "sbi_bank_clear", "sbi_bank_read")
ARGS = {"snapshot_keyframes_enable": 3, "snapshot_keyframes_info": 2, "sbi_bank_take_keyframes": 3, "sbi_bank_clear": 1, "sbi_bank_read": 5}


def test_every_new_entry_is_bound_with_the_header_s_argument_count():
    for name in ENTRIES:
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == declared(name) == ARGS[name], (name, len(args), declared(name))
    # the names the older lists pin stay as they were: no new entry begins with ptam_map_snapshot_ or ptam_frame_report_
    assert not [n for n in ENTRIES if n.startswith(("map_snapshot_", "frame_report_"))]
    assert "ptam_snapshot_keyframes_enable" in HEADER


def test_the_two_structs_match_the_header():
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    for name, cls, size in (("ptam_snapshot_keyframes_info_t", _abi.SnapshotKeyframesInfo, 56),
                            ("ptam_keyframes_take_result", _abi.KeyframesTakeResult, 32)):
        want = [(f, ctype[t]) for t, f in struct_fields(name)]
        assert [(f, t) for f, t in cls._fields_] == want, name
        assert ctypes.sizeof(cls) == size, (name, ctypes.sizeof(cls))
    for f in ("changed", "n_kf", "n_new", "generation", "map_id", "link_bytes"):      # what a take reports
        assert f in dict(_abi.KeyframesTakeResult._fields_)
    # the snapshot's older structs keep their sizes
    assert (ctypes.sizeof(_abi.MapPublishResult), ctypes.sizeof(_abi.MapTakeResult), ctypes.sizeof(_abi.MapSnapshotInfo)) == (32, 40, 24)
    assert _abi.RMAP_TABLES == 12


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.MapSnapshot, ("enable_keyframes", "keyframes")), (host.Relocaliser, ("take_keyframes", "clear", "read"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
