"""The one reader of include/ptam_hip.h and include/ptam_hip_bench.h for the tests (a helper, not a test module): the structs, the
numbers and the prototypes as the headers' text states them, the layout as the host C compiler reads them (compiled_layout), and the
literals the suite pins against both (PINNED_*).  tests/test_abi.py checks ptam_cg_amd/_abi.py against all of it."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("ptam_hip.h", "ptam_hip_bench.h")
RAW = {h: open(os.path.join(INCLUDE, h)).read() for h in HEADERS}                   # with the comments: the doc-comment rules read it
HEADER = "\n".join(re.sub(r"/\*.*?\*/|//[^\n]*", "", RAW[h], flags=re.S) for h in HEADERS)
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")

_STRUCT = r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"
_ENUM = r"\benum\s*\{([^{}]*)\}\s*;"


def _field_names(body):
    """the field names of a struct body, in order, without array bounds and pointer stars"""
    names = []
    for decl in body.split(";"):
        if decl.strip():
            names += [re.sub(r"\[.*", "", d.split()[-1]).lstrip("*") for d in decl.split(",")]
    return names


def _split_params(text):
    """the parameter texts of a prototype: split at the commas outside parentheses; (void) and () are no parameters"""
    out, depth, cur = [], 0, ""
    for ch in text:
        depth += (ch == "(") - (ch == ")")
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return [] if out in ([""], ["void"]) else out


def _prototypes():
    text = re.sub(r"^[ \t]*#.*$", "", HEADER, flags=re.M)                           # (no directive of the headers runs over a line)
    text = re.sub(_STRUCT + "|" + _ENUM + r'|extern\s+"C"\s*\{|\}', "", text)       # what is left of braces closes extern "C"
    out = {}
    for stmt in text.split(";"):
        if not stmt.strip() or stmt.split()[0] == "typedef":
            continue
        m = re.fullmatch(r"\s*(.*?)\b(ptam_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        assert m and m.group(2) not in out, "not a prototype this reader knows: %r" % stmt
        out[m.group(2)] = (" ".join(m.group(1).split()), _split_params(m.group(3)))
    return out


# name -> field names in order, for every `typedef struct {...} name;`
STRUCTS = {name: _field_names(body) for body, name in re.findall(_STRUCT, HEADER)}
# every enumerator and every #define with a value, in header order
NUMBERS = [re.match(r"\s*(\w+)", item).group(1) for body in re.findall(_ENUM, HEADER) for item in body.split(",") if item.strip()] + \
    re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PTAM_\w+)[ \t]+\S", HEADER, flags=re.M)
# name -> (return type text, [parameter text])
PROTOTYPES = _prototypes()
FUNCTION_POINTER_TYPES = re.findall(r"typedef\s+[^;{}]*?\(\s*\*\s*(\w+)\s*\)\s*\(", HEADER)

_SCALARS = {"int": "i32", "int32_t": "i32", "unsigned": "u32", "unsigned int": "u32", "uint32_t": "u32", "int64_t": "i64",
            "uint64_t": "u64", "size_t": "u64", "double": "f64", "void": "void"}


def class_name(struct):
    """ptam_foo_bar or ptam_foo_bar_t -> FooBar, the name of its ctypes.Structure in _abi"""
    return "".join(w.capitalize() for w in re.sub(r"^ptam_|_t$", "", struct).split("_"))


def c_type_class(text):
    """a parameter or return type text -> "ptr", "i32", "u32", "i64", "u64", "f64" or "void" """
    if re.search(r"[*\[(]", text) or any(re.search(r"\b%s\b" % t, text) for t in FUNCTION_POINTER_TYPES):
        return "ptr"
    words = [w for w in text.split() if w != "const"]
    for n in (len(words), len(words) - 1):                                          # without and with a parameter name
        if " ".join(words[:n]) in _SCALARS:
            return _SCALARS[" ".join(words[:n])]
    raise ValueError("a type this reader does not know: %r" % text)


def py_type_class(t):
    """a ctypes restype or argtype -> the same classes"""
    if t is None:
        return "void"
    if issubclass(t, (ctypes._Pointer, ctypes._CFuncPtr, ctypes.Array)) or t._type_ in "PzZ":
        return "ptr"
    if t._type_ == "d":
        return "f64"
    assert t._type_ in "bhilqBHILQ", t
    return "%s%d" % ("i" if t._type_.islower() else "u", 8 * ctypes.sizeof(t))


def layout_program():
    """a C99 program that prints sizeof and every field's offsetof and size for every struct, and the value of every number"""
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + ['#include "%s"' % h for h in HEADERS] + ["int main(void) {"]
    for s, fields in STRUCTS.items():
        lines.append('    printf("S %s %%zu\\n", sizeof(%s));' % (s, s))
        lines += ['    printf("F %s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f) for f in fields]
    lines += ['    printf("N %s %%lld\\n", (long long)%s);' % (n, n) for n in NUMBERS]
    return "\n".join(lines + ["    return 0;", "}", ""])


def run_layout_program(include=INCLUDE):
    """layout_program() built with the host C compiler against the headers of `include` and run -> its output (None: no compiler)"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        return None
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "layout.c"), os.path.join(td, "layout")
        with open(src, "w") as f:
            f.write(layout_program())
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", include, src, "-o", exe])
        return subprocess.check_output([exe], text=True)


@functools.lru_cache(maxsize=None)
def compiled_layout():
    """-> (structs: name -> (size, {field: (offset, size)}), numbers: name -> value) as the C compiler reads the headers, once per
    session; None without a C compiler (the callers skip)"""
    text = run_layout_program()
    if text is None:
        return None
    structs, numbers = {}, {}
    for kind, *rest in (ln.split() for ln in text.splitlines()):
        if kind == "S":
            structs[rest[0]] = (int(rest[1]), {})
        elif kind == "F":
            structs[rest[0]][1][rest[1]] = (int(rest[2]), int(rest[3]))
        else:
            numbers[rest[0]] = int(rest[1])
    return structs, numbers


def lib():
    """the built library, bound (built first where it is missing); no device is touched"""
    from ptam_cg_amd import _abi
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return _abi.bind(ctypes.CDLL(LIB), "ptam_")


# ---- the pinned literals: what a published struct, number or entry is today, whatever the header and _abi agree on tomorrow ----
PINNED_SIZES = {
    "ptam_patch_query": 16, "ptam_patch_result": 40, "ptam_projection": 80, "ptam_pose_meas": 48, "ptam_pose_update_meas": 136,
    "ptam_ba_trial": 48, "ptam_cam_params": 48, "ptam_gn_opts": 40, "ptam_ba_opts": 40, "ptam_motion_model": 12 * 8 * 2 + 6 * 8 + 4 * 8 + 16,
    "ptam_trackmap_opts": 32, "ptam_trackmap_result": 192, "ptam_trackmap_meas": 40, "ptam_calib_corner": 24, "ptam_calib_result": 72,
    "ptam_camera_tracker_opts": 152, "ptam_camera_track_result": 872, "ptam_mapmaker_step_result": 472,
    "ptam_rmap_init_opts": 184, "ptam_rmap_init_result": 688, "ptam_frame_record": 32, "ptam_frame_report_info_t": 32,
    "ptam_rmap_note_result": 8, "ptam_snapshot_keyframes_info_t": 56, "ptam_keyframes_take_result": 32, "ptam_map_publish_result": 32,
    "ptam_map_take_result": 40, "ptam_map_snapshot_info_t": 24, "ptam_map_kf_row": 24, "ptam_rmap_counts_t": 24,
    "ptam_map_outliers_result": 24, "ptam_map_refind_result": 32, "ptam_track_report_info": 40, "ptam_refind_pair": 248,
    "ptam_new_map_point": 200, "ptam_trail": 16, "ptam_homography_match": 64, "ptam_map_point_source": 80, "ptam_scene_depth": 24,
    "ptam_map_pair": 8, "ptam_map_refind_point": 96, "ptam_map_column": 16, "ptam_map_bad_points_result": 32,
}
PINNED_OFFSETS = {("ptam_rmap_init_result", "depth"): 176, ("ptam_track_report_info", "report_in_chain"): 32}
PINNED_NUMBERS = {
    "PTAM_CALIB_OK": 0, "PTAM_CALIB_NO_MEASUREMENTS": 1, "PTAM_CALIB_GUESS_OK": 0, "PTAM_CALIB_GUESS_REFUSED": 1,
    "PTAM_CALIB_MAX_IMAGES": 65536, "PTAM_CALIB_MAX_CORNERS": 4194304, "PTAM_CALIB_MAX_STEPS": 65536,
    "PTAM_MM_RAN": 0, "PTAM_MM_IDLE": 1, "PTAM_MM_RESET": 2, "PTAM_MM_INIT": 3,
    "PTAM_MM_STAGE_BUNDLE_RECENT": 1, "PTAM_MM_STAGE_REFIND_NEW": 2, "PTAM_MM_STAGE_BUNDLE_ALL": 4, "PTAM_MM_STAGE_REFIND_FAILURE": 8,
    "PTAM_MM_STAGE_NOTES": 16, "PTAM_MM_STAGE_BAD_POINTS": 32, "PTAM_MM_STAGE_ADD_KEYFRAME": 64, "PTAM_MM_STAGE_PUBLISH": 128,
    "PTAM_MM_STAGE_INIT": 256, "PTAM_MM_INIT_NONE": 0, "PTAM_MM_INIT_PENDING": 1, "PTAM_MM_INIT_DONE": 2,
    "PTAM_TRAIL_TRACKING_NOT_STARTED": 0, "PTAM_TRAIL_TRACKING_STARTED": 1, "PTAM_TRAIL_TRACKING_COMPLETE": 2,
    "PTAM_INIT_MAP_OK": 0, "PTAM_INIT_MAP_NO_HOMOGRAPHY": 1, "PTAM_INIT_MAP_ZERO_BASELINE": 2, "PTAM_INIT_MAP_TOO_FEW_POINTS": 3,
    "PTAM_INIT_MAP_STOPPED": 4,
    "PTAM_RMAP_KF_POSES": 0, "PTAM_RMAP_KF_FIXED": 1, "PTAM_RMAP_POINTS3": 2, "PTAM_RMAP_REFIND_POINTS": 3, "PTAM_RMAP_SOURCES": 4,
    "PTAM_RMAP_BAD": 5, "PTAM_RMAP_OUTLIER_COUNT": 6, "PTAM_RMAP_INLIER_COUNT": 7, "PTAM_RMAP_MEAS": 8, "PTAM_RMAP_NEVER": 9,
    "PTAM_RMAP_NEW_QUEUE": 10, "PTAM_RMAP_FAILURE": 11, "PTAM_RMAP_TABLES": 12, "PTAM_RMAP_OUTLIERS": 12, "PTAM_RMAP_WORD_BYTES": 64,
    "PTAM_RMAP_KF_RECORD_BYTES": 512,
}
# of these families the header has exactly the names pinned above / below: a new one is added here with its number or count
PINNED_NUMBER_FAMILIES = ("PTAM_MM_", "PTAM_INIT_MAP_", "PTAM_RMAP_")
PINNED_ENTRY_FAMILIES = ("map_snapshot_", "frame_report_")
# entry -> its number of arguments
PINNED_ENTRIES = {
    "calib_create": 4, "calib_destroy": 1, "calib_reset": 3, "calib_counts": 3, "calib_add_images": 5, "calib_set_poses": 2,
    "calib_read_poses": 2, "calib_optimize": 4, "calib_params": 2, "calib_residuals": 4,
    "mapmaker_opts_default": 1, "mapmaker_create": 5, "mapmaker_destroy": 1, "mapmaker_add_keyframe": 8, "mapmaker_note_frame": 3,
    "mapmaker_queue_size": 2, "mapmaker_request_reset": 1, "mapmaker_reset_done": 2, "mapmaker_flags": 4, "mapmaker_set_flags": 3,
    "mapmaker_released": 4, "mapmaker_step": 2,
    "trails_advance_batch": 6, "mapmaker_request_init": 7, "mapmaker_init_poll": 3, "camera_session_opts_default": 1,
    "camera_tracker_enable_session": 2, "camera_tracker_restart": 1, "camera_tracker_session_frames": 6,
    "camera_tracker_init_result": 2, "camera_tracker_stage": 2,
    "camera_tracker_opts_default": 1, "camera_tracker_create": 5, "camera_tracker_destroy": 1, "camera_tracker_reset": 2,
    "camera_tracker_state": 2, "camera_tracker_tracker": 1, "camera_tracker_current_keyframe": 1, "camera_tracker_last_report": 1,
    "camera_tracker_pool": 3, "camera_tracker_track_frames": 4,
    "rmap_init_opts_default": 1, "rmap_init_from_stereo": 9, "rmap_align_to_plane": 5, "rmap_clear": 1,
    "snapshot_keyframes_enable": 3, "snapshot_keyframes_info": 2, "sbi_bank_take_keyframes": 3, "sbi_bank_clear": 1, "sbi_bank_read": 5,
    "rmap_bundle_adjust_routed": 6, "rmap_refind_queue": 6,
    "frame_report_create": 3, "frame_report_destroy": 1, "frame_report_info": 2, "frame_report_read": 4, "frame_report_from_host": 6,
    "tracker_report_frames": 4, "rmap_note_reports": 4, "rmap_insert_keyframe_report": 10,
    "map_snapshot_create": 3, "map_snapshot_destroy": 1, "map_snapshot_reserve": 2, "map_snapshot_info": 2, "rmap_publish": 3,
    "rmap_point_serials": 4, "rmap_resolve_serials": 5, "tracker_take_map": 3, "tracker_point_serials": 4,
    "tracker_read_iteration_serials": 4,
    "rmap_upload": 20, "rmap_download": 5, "rmap_traffic": 3, "rmap_apply_outliers": 4, "rmap_scene_depth": 2,
    "track_frames_recover_batch": 12, "track_frames_report_batch": 16, "tracker_draw_shuffles": 3, "tracker_read_shuffle": 3,
    "shuffle_order_host": 5, "kf_copy": 3,
}


if __name__ == "__main__":
    # the layout program's output for the headers of a directory (default: this tree's include/): two trees' outputs are diffed
    sys.stdout.write(run_layout_program(*sys.argv[1:2]))
