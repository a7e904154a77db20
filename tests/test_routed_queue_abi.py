"""CPU: the Python side of ptam_rmap_bundle_adjust_routed and ptam_rmap_refind_queue matches include/ptam_hip.h — the argument
counts, the result structs they share with the calls they stand for — the built library exports both, the shim compiles with its
two methods, and the header states each call's host-link bytes without a term in the outlier count or a queue's length."""
import ctypes
import os
import re
import subprocess

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW = open(os.path.join(ROOT, "include", "ptam_hip.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", RAW, flags=re.S)
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
NEW = {"rmap_bundle_adjust_routed": 6, "rmap_refind_queue": 6}


def test_argument_counts_and_result_structs_match_the_header():
    for name, n_args in NEW.items():
        args = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == n_args == len(_abi.PROTOTYPES[name][1]), name
        assert _abi.PROTOTYPES[name][0] is ctypes.c_int and name in _abi.DECLARED
    routed, queue = _abi.PROTOTYPES["rmap_bundle_adjust_routed"][1], _abi.PROTOTYPES["rmap_refind_queue"][1]
    # the results are those of the calls they stand for
    assert routed[4] is _abi.PROTOTYPES["rmap_bundle_adjust"][1][4] and routed[5] is _abi.PROTOTYPES["rmap_apply_outliers"][1][3]
    assert queue[2] is _abi.PROTOTYPES["rmap_refind"][1][2] and queue[5] is _abi.PROTOTYPES["rmap_refind"][1][7]
    assert ctypes.sizeof(_abi.MapOutliersResult) == 24 and ctypes.sizeof(_abi.MapRefindResult) == 32
    for method in ("bundle_adjust_routed", "refind_queue"):
        assert callable(getattr(host.ResidentMap, method))


def test_the_library_exports_both_and_refuses_null_handles():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = _abi.bind(ctypes.CDLL(LIB), "ptam_")
    assert not set(NEW) & set(lib.missing)
    ba, out, rr = _abi.MapBaResult(), _abi.MapOutliersResult(), _abi.MapRefindResult()
    assert lib.rmap_bundle_adjust_routed(None, None, _abi.MAP_BA_ALL, None, ctypes.byref(ba), ctypes.byref(out)) == -1   # PTAM_E_ARG
    assert lib.rmap_refind_queue(None, None, None, _abi.MAP_REFIND_NEW_POINTS, None, ctypes.byref(rr)) == -1


def test_the_header_states_the_bytes_of_both_calls():
    for name in NEW:
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+ptam_" + name + r"\b", RAW, flags=re.S)[-1]
        assert "Moves" in comment and re.search(r"No term grows with (the outlier count|a queue's length)", comment), name


def test_the_shim_compiles_with_its_two_methods(tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "ptam_shim.hpp"\n'
                   "ptam_map_refind_result f(ptam::ResidentMap& m, ptam::ReFinder& r) {\n"
                   "    ptam::ResidentMap::BundleAdjustRoutedResult b = m.BundleAdjustRouted(PTAM_MAP_BA_RECENT);\n"
                   "    (void)b.outliers.n_never_added;\n"
                   "    return m.ReFindQueue(r, PTAM_MAP_REFIND_FAILURE_QUEUE);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
