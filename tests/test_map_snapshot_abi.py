"""CPU: the Python side of the map's publication to the tracker (ptam_map_snapshot_*, ptam_rmap_publish / point_serials /
resolve_serials, ptam_tracker_take_map / point_serials / read_iteration_serials) matches include/ptam_hip.h: every entry bound
with as many arguments as the header declares, the result structs of the header's sizes and field order, and the built library
exports each of them."""
import ctypes
import os
import re

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)
ENTRIES = ("map_snapshot_create", "map_snapshot_destroy", "map_snapshot_reserve", "map_snapshot_info", "rmap_publish", "rmap_point_serials",
           "rmap_resolve_serials", "tracker_take_map", "tracker_point_serials", "tracker_read_iteration_serials")


def declared(name):
    m = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def struct_fields(name):
    """the fields of `typedef struct { ... } name;` in order -> [(c type, field)]"""
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", HEADER, flags=re.S)
    assert m, name
    out = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            out += [(ctype, n.strip()) for n in names.split(",")]
    return out


def test_every_new_entry_is_bound_with_the_header_s_argument_count():
    for name in ENTRIES:
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == declared(name), (name, len(args), declared(name))
    # every snapshot entry of the header is one of them
    assert sorted(re.findall(r"\bint\s+ptam_(map_snapshot_[a-z0-9_]+)\s*\(", HEADER)) == sorted(n for n in ENTRIES if n.startswith("map_snapshot_"))


def test_the_result_structs_match_the_header():
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for name, cls, size in (("ptam_map_publish_result", _abi.MapPublishResult, 32), ("ptam_map_take_result", _abi.MapTakeResult, 40),
                            ("ptam_map_snapshot_info_t", _abi.MapSnapshotInfo, 24)):
        want = [(f, ctype[t]) for t, f in struct_fields(name)]
        assert [(f, t) for f, t in cls._fields_] == want, name
        assert ctypes.sizeof(cls) == size, (name, ctypes.sizeof(cls))
    for f in ("changed", "generation", "n_points", "n_carried", "n_new", "n_dropped"):      # what a take reports
        assert f in dict(_abi.MapTakeResult._fields_)


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.ResidentMap, ("publish", "point_serials", "resolve_serials")), (host.Tracker, ("take_map", "point_serials", "iteration_serials")),
                       (host.MapSnapshot, ("reserve", "info", "close"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    # the table numbers of ptam_rmap_download stay: the serial column is not one of them
    assert _abi.RMAP_TABLES == 12 and len(host.ResidentMap.TABLES) == 12
