"""CPU: the Python side of ptam_mapmaker matches include/ptam_hip.h — the field order and sizes of ptam_mapmaker_opts and
ptam_mapmaker_step_result, the status and stage numbers, the argument counts — the defaults ptam_mapmaker_opts_default writes are the
reference's (src/MapMaker.cc:103, :511-514), and the handle's host-only entries (queue, flags, reset request, released tags) do what
the header says without a device."""
import ctypes
import os
import re

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
ENTRIES = {"mapmaker_opts_default": 1, "mapmaker_create": 5, "mapmaker_destroy": 1, "mapmaker_add_keyframe": 8, "mapmaker_note_frame": 3,
           "mapmaker_queue_size": 2, "mapmaker_request_reset": 1, "mapmaker_reset_done": 2, "mapmaker_flags": 4, "mapmaker_set_flags": 3,
           "mapmaker_released": 4, "mapmaker_step": 2}


def header_fields(struct):
    """the field names of `typedef struct { ... } struct;`, in order, arrays without their bounds"""
    body = re.search(r"typedef\s+struct\s*{([^{}]*)}\s*" + struct + r"\s*;", HEADER).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names.append(re.sub(r"\[.*", "", first.split()[-1]).lstrip("*"))
            names += [re.sub(r"\[.*", "", r.strip()).lstrip("*") for r in rest]
    return names


def test_struct_fields_and_sizes_match_the_header():
    assert header_fields("ptam_mapmaker_opts") == [f for f, _ in _abi.MapmakerOpts._fields_]
    assert header_fields("ptam_mapmaker_step_result") == [f for f, _ in _abi.MapmakerStepResult._fields_]
    S = ctypes.sizeof
    assert S(_abi.MapmakerOpts) == S(_abi.BaOpts) + S(_abi.MapRefindOpts) + S(_abi.RmapInsertOpts) + 4 + 4 + 8
    parts = (_abi.MapBaResult, _abi.MapOutliersResult, _abi.MapRefindResult, _abi.MapBaResult, _abi.MapOutliersResult, _abi.MapRefindResult,
             _abi.RmapNoteResult, _abi.MapBadPointsResult, _abi.RmapInsertResult, _abi.MapPublishResult)
    assert S(_abi.MapmakerStepResult) == 8 + sum(S(p) for p in parts) + 8 + 16 + 8
    assert _abi.MapmakerStepResult.insert.offset % 8 == 0 and _abi.MapmakerStepResult.draws.offset % 8 == 0


def test_numbers_and_argument_counts_match_the_header():
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(PTAM_MM_[A-Z_]+)\s*=\s*(\d+)", HEADER))
    assert sorted(enum) == sorted(["PTAM_MM_RAN", "PTAM_MM_IDLE", "PTAM_MM_RESET"] + ["PTAM_MM_STAGE_" + s for s in (
        "BUNDLE_RECENT", "REFIND_NEW", "BUNDLE_ALL", "REFIND_FAILURE", "NOTES", "BAD_POINTS", "ADD_KEYFRAME", "PUBLISH")])
    for k, v in enum.items():
        assert getattr(_abi, k[len("PTAM_"):]) == v, k
    for name, n_args in ENTRIES.items():
        args = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == n_args == len(_abi.PROTOTYPES[name][1]), name
        assert _abi.PROTOTYPES[name][0] is ctypes.c_int
    for method in ("AddKeyFrame", "NoteFrame", "QueueSize", "RequestReset", "ResetDone", "Step", "flags", "set_flags", "released", "mapmaker_opts"):
        assert callable(getattr(host.MapMaker, method))


def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return _abi.bind(ctypes.CDLL(LIB), "ptam_")


def test_defaults_are_the_reference_s():
    L = lib()
    o = _abi.MapmakerOpts()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    assert L.mapmaker_opts_default(ctypes.byref(o)) == 0 and L.mapmaker_opts_default(None) == -1
    assert (o.failure_period, o.failure_seed) == (20, 0)                                              # rand() % 20
    assert o.insert.epipolar.n_levels == 4 and list(o.insert.epipolar.levels) == [3, 0, 1, 2]        # :511-514
    assert (o.insert.target_kf, o.insert.skip_refind, o.insert.skip_points, o.refind.max_pairs_per_pass) == (-1, 0, 0, 0)
    ba, epi = _abi.BaOpts(), _abi.EpipolarOpts()
    L.ba_opts_default(ctypes.byref(ba))
    L.epipolar_opts_default(ctypes.byref(epi))
    assert bytes(o.ba) == bytes(ba)
    assert (o.insert.epipolar.wiggle_scale, o.insert.epipolar.min_shi_tomasi, o.insert.epipolar.subpix_max_its) == (
        epi.wiggle_scale, epi.min_shi_tomasi, epi.subpix_max_its)


def test_queue_flags_reset_request_and_tags_without_a_device():
    """the entries the tracker's thread calls touch no device: any non-null handles do (they are only kept)"""
    L = lib()
    mm, word = ctypes.c_void_p(), ctypes.c_int32()
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.mapmaker_create(None, fake, None, None, ctypes.byref(mm)) == -1
    bad = _abi.MapmakerOpts()
    L.mapmaker_opts_default(ctypes.byref(bad))
    bad.failure_period = 0
    assert L.mapmaker_create(fake, fake, None, ctypes.byref(bad), ctypes.byref(mm)) == -1
    assert L.mapmaker_create(fake, fake, None, None, ctypes.byref(mm)) == 0
    r, f, b = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert L.mapmaker_flags(mm, ctypes.byref(r), ctypes.byref(f), ctypes.byref(b)) == 0 and (r.value, f.value, b.value) == (1, 1, 0)   # Reset()
    assert L.mapmaker_set_flags(mm, 0, 1) == 0 and L.mapmaker_flags(mm, ctypes.byref(r), ctypes.byref(f), ctypes.byref(b)) == 0
    assert (r.value, f.value) == (0, 1)
    pose = (ctypes.c_double * 12)()
    assert L.mapmaker_add_keyframe(mm, None, pose, 0, fake, 1.0, 0.3, 7) == -1
    assert L.mapmaker_add_keyframe(mm, fake, pose, 0, fake, 1.0, 0.3, 7) == 0 and L.mapmaker_add_keyframe(mm, fake, pose, 0, fake, 1.0, 0.3, 8) == 0
    assert L.mapmaker_note_frame(mm, fake, 9) == 0 and L.mapmaker_note_frame(mm, None, 9) == -1
    assert L.mapmaker_queue_size(mm, ctypes.byref(word)) == 0 and word.value == 2
    tags = (ctypes.c_int64 * 4)()
    assert L.mapmaker_released(mm, 4, tags, ctypes.byref(word)) == 0 and word.value == 0          # nothing is finished with yet
    assert L.mapmaker_reset_done(mm, ctypes.byref(word)) == 0 and word.value == 1
    assert L.mapmaker_request_reset(mm) == 0 and L.mapmaker_reset_done(mm, ctypes.byref(word)) == 0 and word.value == 0
    assert L.mapmaker_destroy(mm) == 0 and L.mapmaker_destroy(None) == 0
