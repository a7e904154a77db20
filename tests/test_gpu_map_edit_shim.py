"""-m gpu: builds examples/map_edit_demo.cc (ptam::ApplyBundleOutliers / HandleBadPoints / AddPointsToTables of ptam_shim.hpp,
std::vector tables) with g++, runs it on map tables written by the test, and checks its output file against the Python calls
host.map_apply_outliers / map_handle_bad_points / map_add_points on the same tables, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import map_edit_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("map_edit_demo") / "map_edit_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "map_edit_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_matches_python_calls(hip, demo, tmp_path):
    t = E.gpu_case()
    K, N = t["n_kf"], t["n_points"]
    made, points3 = E.make_made(10, 120), E.point_columns(9, N)[0]
    src_kf, target_kf, source = 6, 4, _abi.SRC_EPIPOLAR
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K, N, len(t["meas"]), len(t["never"]), len(t["new_queue"]), len(t["failure"]), len(t["outliers"]), len(made),
                          src_kf, target_kf, source, 0], np.int32).tobytes())
        for a in (t["bad"], t["outlier_count"], t["inlier_count"], t["meas"], t["never"], t["new_queue"], t["failure"], t["outliers"], made, points3):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    ctx = host.Context(lib=hip)
    a = host.map_apply_outliers(ctx, K, t["bad"], t["meas"], t["never"], t["failure"], t["outliers"])
    b = host.map_handle_bad_points(ctx, K, N, a["meas"], a["never"], bad=a["bad"], outlier_count=t["outlier_count"],
                                   inlier_count=t["inlier_count"], new_queue=t["new_queue"], failure=a["failure"], columns=[points3])
    c = host.map_add_points(ctx, K, b["n_kept"], b["meas"], src_kf, target_kf, made, source)
    ctx.close()
    assert out.startswith("MAPEDIT outliers %d/%d/%d removed %d kept %d " % (a["n_point_bad"], a["n_failure_added"], a["n_never_added"],
                                                                             b["n_removed"], b["n_kept"]))
    want = [np.array([a[k] for k in E.OUTLIER_COUNTS], np.int32), a["bad"], a["meas"], a["never"], a["failure"],
            np.array([b[k] for k in E.BAD_COUNTS], np.int32), b["new_index"], b["kept"], b["meas"], b["never"], b["new_queue"], b["failure"],
            b["columns"][0][:b["n_kept"]], c["meas"], c["points"], c["sources"]]
    assert open(fout, "rb").read() == b"".join(np.ascontiguousarray(w).tobytes() for w in want)
    assert a["n_never_added"] > 0 and b["n_marked"] > 0 and b["n_new_dropped"] > 0 and len(c["meas"]) == len(b["meas"]) + 2 * len(made)
