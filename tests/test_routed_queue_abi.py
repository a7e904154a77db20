"""CPU: ptam_rmap_bundle_adjust_routed and ptam_rmap_refind_queue (their argument counts and structs are checked with the whole header
in tests/test_abi.py) share the result structs of the calls they stand for, the built library exports both, the shim compiles with
its two methods, and the header states each call's host-link bytes without a term in the outlier count or a queue's length."""
import ctypes
import re
import subprocess

from ptam_cg_amd import _abi, host
from tests.abi_header import INCLUDE, RAW, lib as bound_lib

NEW = ("rmap_bundle_adjust_routed", "rmap_refind_queue")


def test_the_results_are_those_of_the_calls_they_stand_for():
    for name in NEW:
        assert _abi.PROTOTYPES[name][0] is ctypes.c_int and name in _abi.DECLARED
    routed, queue = _abi.PROTOTYPES["rmap_bundle_adjust_routed"][1], _abi.PROTOTYPES["rmap_refind_queue"][1]
    assert routed[4] is _abi.PROTOTYPES["rmap_bundle_adjust"][1][4] and routed[5] is _abi.PROTOTYPES["rmap_apply_outliers"][1][3]
    assert queue[2] is _abi.PROTOTYPES["rmap_refind"][1][2] and queue[5] is _abi.PROTOTYPES["rmap_refind"][1][7]
    for method in ("bundle_adjust_routed", "refind_queue"):
        assert callable(getattr(host.ResidentMap, method))


def test_the_library_exports_both_and_refuses_null_handles():
    lib = bound_lib()
    assert not set(NEW) & set(lib.missing)
    ba, out, rr = _abi.MapBaResult(), _abi.MapOutliersResult(), _abi.MapRefindResult()
    assert lib.rmap_bundle_adjust_routed(None, None, _abi.MAP_BA_ALL, None, ctypes.byref(ba), ctypes.byref(out)) == -1   # PTAM_E_ARG
    assert lib.rmap_refind_queue(None, None, None, _abi.MAP_REFIND_NEW_POINTS, None, ctypes.byref(rr)) == -1


def test_the_header_states_the_bytes_of_both_calls():
    for name in NEW:
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*int\s+ptam_" + name + r"\b", RAW["ptam_hip.h"], flags=re.S)[-1]
        assert "Moves" in comment and re.search(r"No term grows with (the outlier count|a queue's length)", comment), name


def test_the_shim_compiles_with_its_two_methods(tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "ptam_shim.hpp"\n'
                   "ptam_map_refind_result f(ptam::ResidentMap& m, ptam::ReFinder& r) {\n"
                   "    ptam::ResidentMap::BundleAdjustRoutedResult b = m.BundleAdjustRouted(PTAM_MAP_BA_RECENT);\n"
                   "    (void)b.outliers.n_never_added;\n"
                   "    return m.ReFindQueue(r, PTAM_MAP_REFIND_FAILURE_QUEUE);\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + INCLUDE, str(src)])
