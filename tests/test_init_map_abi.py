"""CPU: the Python side of ptam_rmap_init_from_stereo, ptam_rmap_align_to_plane and ptam_rmap_clear matches include/ptam_hip.h — the
struct sizes and the field order of ptam_rmap_init_opts / ptam_rmap_init_result, the status numbers, the argument counts — and the
defaults ptam_rmap_init_opts_default writes are the reference's (src/MapMaker.cc:34, :283, :333, :374, :382-385)."""
import ctypes
import os
import re

from ptam_cg_amd import _abi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptam_hip.h")).read(), flags=re.S)
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")


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
    assert header_fields("ptam_rmap_init_opts") == [f for f, _ in _abi.RmapInitOpts._fields_]
    assert header_fields("ptam_rmap_init_result") == [f for f, _ in _abi.RmapInitResult._fields_]
    parts = (_abi.HomographyOpts, _abi.BaOpts, _abi.EpipolarOpts, _abi.PlaneOpts)
    assert ctypes.sizeof(_abi.RmapInitOpts) == sum(ctypes.sizeof(p) for p in parts) + 8 + 4 * 4 == 184
    assert ctypes.sizeof(_abi.RmapInitResult) == (8 + ctypes.sizeof(_abi.HomographyInfo) + 8 + 4 * 4 + 6 * 4 + 2 * ctypes.sizeof(_abi.SceneDepth) + 8
                                                  + 2 * 4 + 4 * ctypes.sizeof(_abi.EpipolarLevelStats) + ctypes.sizeof(_abi.PlaneInfo) + 2 * 96
                                                  + ctypes.sizeof(_abi.RmapCounts)) == 688
    assert _abi.RmapInitResult.tracker_pose.offset % 8 == 0 and _abi.RmapInitResult.depth.offset == 176


def test_status_numbers_and_argument_counts_match_the_header():
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(PTAM_INIT_MAP_[A-Z_]+)\s*=\s*(\d+)", HEADER))
    assert sorted(enum) == ["PTAM_INIT_MAP_NO_HOMOGRAPHY", "PTAM_INIT_MAP_OK", "PTAM_INIT_MAP_STOPPED", "PTAM_INIT_MAP_TOO_FEW_POINTS",
                            "PTAM_INIT_MAP_ZERO_BASELINE"]
    for k, v in enum.items():
        assert getattr(_abi, k[len("PTAM_"):]) == v, k
    for name, n_args in (("rmap_init_opts_default", 1), ("rmap_init_from_stereo", 9), ("rmap_align_to_plane", 5), ("rmap_clear", 1)):
        args = re.search(r"\bint\s+ptam_" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, flags=re.S).group(1)
        assert len([a for a in args.split(",") if a.strip()]) == n_args == len(_abi.PROTOTYPES[name][1]), name
        assert _abi.PROTOTYPES[name][0] is ctypes.c_int
    for method in ("init_opts", "InitFromStereo", "align_to_plane", "clear"):
        assert callable(getattr(host.ResidentMap, method))


def test_defaults_are_the_reference_s():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = _abi.bind(ctypes.CDLL(LIB), "ptam_")
    o = _abi.RmapInitOpts()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    assert lib.rmap_init_opts_default(ctypes.byref(o)) == 0 and lib.rmap_init_opts_default(None) == -1
    assert (o.homography.max_pixel_error, o.homography.trials, o.homography.seed, bool(o.homography.samples)) == (5.0, 300, 0, False)
    assert (o.wiggle_scale, o.subpix_max_its, o.first_bundles, o.max_bundles) == (0.1, 10, 5, 0)
    assert o.epipolar.n_levels == 4 and list(o.epipolar.levels) == [0, 3, 1, 2]
    ba, epi, plane = _abi.BaOpts(), _abi.EpipolarOpts(), _abi.PlaneOpts()
    lib.ba_opts_default(ctypes.byref(ba))
    lib.epipolar_opts_default(ctypes.byref(epi))
    lib.plane_opts_default(ctypes.byref(plane))
    assert bytes(o.ba) == bytes(ba)
    assert (o.epipolar.wiggle_scale, o.epipolar.min_shi_tomasi, o.epipolar.subpix_max_its) == (epi.wiggle_scale, epi.min_shi_tomasi, epi.subpix_max_its)
    assert (o.plane.max_dist, o.plane.trials, o.plane.seed, bool(o.plane.samples)) == (plane.max_dist, plane.trials, plane.seed, False) == (0.05, 100, 0, False)
