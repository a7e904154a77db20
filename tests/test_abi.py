"""CPU: ptam_cg_amd/_abi.py, and the numpy record types host.py and synth.py derive from it, state what include/ptam_hip.h and
include/ptam_hip_bench.h state — every struct, every number, every prototype — with the layout and the values as the host C compiler
reads the headers (tests/abi_header.py: compiled_layout, built once per session), and the literals pinned there hold."""
import ctypes
import re
import shutil
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import abi_header as H

STRUCT_OF = {H.class_name(s): s for s in H.STRUCTS}                                  # class name -> header struct
DT_CLASS = {"EPIPOLAR_STATS_DT": "EpipolarLevelStats"}                               # FOO_BAR_DT is FooBar's, but for these


@pytest.fixture
def layout():
    got = H.compiled_layout()
    if got is None:
        pytest.skip("no C compiler")
    return got


def test_every_struct_has_its_class_with_the_header_s_fields_and_layout(layout):
    structs, _ = layout
    classes = sorted(k for k, v in vars(_abi).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _abi.__name__)
    assert len(STRUCT_OF) == len(H.STRUCTS) == len(structs) >= 74
    assert classes == sorted(STRUCT_OF)                                              # no struct without a class, no class without a struct
    for s, fields in H.STRUCTS.items():
        cls = getattr(_abi, H.class_name(s))
        assert [f for f, _ in cls._fields_] == fields, s
        size, by_field = structs[s]
        assert ctypes.sizeof(cls) == size, (s, ctypes.sizeof(cls), size)
        for f in fields:
            assert (getattr(cls, f).offset, getattr(cls, f).size) == by_field[f], (s, f, getattr(cls, f), by_field[f])


def test_every_enumerator_and_define_has_its_constant(layout):
    _, numbers = layout
    assert sorted(numbers) == sorted(H.NUMBERS) and len(numbers) == len(H.NUMBERS) >= 140
    for name, value in numbers.items():
        assert name.startswith("PTAM_") and getattr(_abi, name[len("PTAM_"):], None) == value, (name, value)


def test_every_prototype_is_bound_with_the_header_s_types():
    assert sorted(_abi.PROTOTYPES) == sorted(n[len("ptam_"):] for n in H.PROTOTYPES) == _abi.DECLARED and len(H.PROTOTYPES) >= 246
    for name, (ret, params) in H.PROTOTYPES.items():
        res, args = _abi.PROTOTYPES[name[len("ptam_"):]]
        assert len(args) == len(params), (name, len(args), len(params))
        want = [H.c_type_class(ret)] + [H.c_type_class(p) for p in params]
        got = [H.py_type_class(res)] + [H.py_type_class(a) for a in args]
        wrong = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]       # (0: the return value, then the arguments)
        assert not wrong, "%s: (position, _abi, header) %s" % (name, wrong)
    assert _abi.PROTOTYPES["ba_set_comm"][1][3] is _abi.ALLREDUCE_FN


def test_every_record_type_is_its_class_s(layout):
    structs, _ = layout
    seen = []
    for mod in (host, synth):
        for name, dt in sorted(vars(mod).items()):
            if name.endswith("_DT"):
                cls = DT_CLASS.get(name) or "".join(w.capitalize() for w in name[:-len("_DT")].split("_"))
                assert isinstance(dt, np.dtype) and dt == np.dtype(getattr(_abi, cls)), name
                assert dt.itemsize == structs[STRUCT_OF[cls]][0], (name, dt.itemsize)
                assert list(dt.names) == H.STRUCTS[STRUCT_OF[cls]], name
                seen.append(name)
    assert len(seen) >= 33 and "POSE_MEAS_DT" in seen and synth.CALIB_CORNER_DT == host.CALIB_CORNER_DT
    assert "lambda" in host.BA_TRIAL_DT.names and host.PVS_RESULT_DT["proj"] == host.PROJECTION_DT          # nested structs nested


def test_the_headers_are_c_plus_plus_too(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    (tmp_path / "use.cc").write_text("".join('#include "%s"\n' % h for h in H.HEADERS))
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-I", H.INCLUDE, str(tmp_path / "use.cc")])


def test_the_pinned_literals_hold(layout):
    structs, numbers = layout
    for s, size in H.PINNED_SIZES.items():
        assert structs[s][0] == size == ctypes.sizeof(getattr(_abi, H.class_name(s))), (s, structs[s][0], size)
    for (s, f), off in H.PINNED_OFFSETS.items():
        assert structs[s][1][f][0] == off == getattr(getattr(_abi, H.class_name(s)), f).offset, (s, f)
    for name, value in H.PINNED_NUMBERS.items():
        assert numbers[name] == value == getattr(_abi, name[len("PTAM_"):]), name
    for family in H.PINNED_NUMBER_FAMILIES:
        assert sorted(n for n in H.NUMBERS if n.startswith(family)) == sorted(n for n in H.PINNED_NUMBERS if n.startswith(family)), family
    for name, n_args in H.PINNED_ENTRIES.items():
        assert len(H.PROTOTYPES["ptam_" + name][1]) == n_args == len(_abi.PROTOTYPES[name][1]), name
    for family in H.PINNED_ENTRY_FAMILIES:
        assert sorted(n[len("ptam_"):] for n in H.PROTOTYPES if n.startswith("ptam_" + family)) == \
            sorted(n for n in H.PINNED_ENTRIES if n.startswith(family)), family


def test_the_reader_reads_what_it_says():
    """the helper's own parsing, on declarations whose answer is known"""
    assert H.STRUCTS["ptam_patch_result"] == ["found", "best_ssd", "best_x", "best_y", "n_scored", "pad_", "pos"]
    assert H.STRUCTS["ptam_homography_opts"][-1] == "samples" and H.class_name("ptam_rmap_counts_t") == "RmapCounts"
    assert H.PROTOTYPES["ptam_last_error"] == ("const char*", []) and H.PROTOTYPES["ptam_ctx_stream"][0] == "void*"
    assert len(H.PROTOTYPES["ptam_ba_set_comm"][1]) == 5 and H.c_type_class(H.PROTOTYPES["ptam_ba_set_comm"][1][3]) == "ptr"
    assert [H.c_type_class(t) for t in ("int n", "const double out[8]", "size_t bytes", "uint64_t seed", "int64_t tag", "double", "unsigned", "void")] == \
        ["i32", "ptr", "u64", "u64", "i64", "f64", "u32", "void"]
    assert [H.py_type_class(t) for t in (ctypes.c_int, ctypes.c_size_t, ctypes.c_int64, ctypes.c_longlong, ctypes.c_char_p, None, _abi.ALLREDUCE_FN)] == \
        ["i32", "u64", "i64", "i64", "ptr", "void", "ptr"]
    assert not re.search(r"/\*|\*/", H.HEADER) and "PTAM_HIP_H" not in H.NUMBERS and "PTAM_LEVELS" in H.NUMBERS
