"""CPU: the Python side of the resident map (ptam_rmap) matches include/ptam_hip.h — every entry bound with as many arguments as the
header declares, the table numbers, the record sizes — and host.ResidentMap names every table once."""
import ctypes
import os
import re

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)


def declared():
    """name (without ptam_) -> number of arguments, for every ptam_rmap_* function of the header"""
    out = {}
    for name, args in re.findall(r"\bint\s+ptam_(rmap_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


def test_every_resident_entry_is_bound_with_the_header_s_argument_count():
    d = declared()
    assert len(d) >= 14 and {"rmap_upload", "rmap_download", "rmap_traffic", "rmap_apply_outliers", "rmap_scene_depth"} <= set(d)
    for name, n_args in d.items():
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == n_args, (name, len(args), n_args)
    assert sorted(n for n in _abi.PROTOTYPES if n.startswith("rmap_")) == sorted(d)


def test_table_numbers_and_record_sizes_match_the_header():
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(PTAM_RMAP_[A-Z0-9_]+)\s*=\s*(\d+)", HEADER))
    for k, v in enum.items():
        assert getattr(_abi, k[len("PTAM_"):]) == v, k
    assert enum["PTAM_RMAP_TABLES"] == len(host.ResidentMap.TABLES) == 12
    assert sorted(i for i, _ in host.ResidentMap.TABLES.values()) == list(range(12))
    row_bytes = {k: dt.itemsize for k, (_, dt) in host.ResidentMap.TABLES.items()}
    assert row_bytes == dict(poses=96, fixed=1, points3=24, points=96, sources=80, bad=1, outlier_count=4, inlier_count=4, meas=32, never=8,
                             new_queue=4, failure=8)
    assert ctypes.sizeof(_abi.MapKfRow) == host.MAP_KF_ROW_DT.itemsize == 24 and ctypes.sizeof(_abi.RmapCounts) == 24
    assert re.search(r"int32_t\s+point,\s*level;\s*double\s+root_pos\[2\];\s*}\s*ptam_map_kf_row", HEADER)
    assert re.search(r"int32_t\s+n_kf,\s*n_points,\s*n_meas,\s*n_never,\s*n_new,\s*n_failure;\s*}\s*ptam_rmap_counts_t", HEADER)
