"""-m gpu: builds examples/plane_align_demo.cc (ptam::AlignMapToPlane / ptam::RefreshSceneDepth of ptam_shim.hpp) with g++, runs it
once, and works the map it prints through the numpy restatement (tests/plane_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import plane_ref as PR
from tests.test_gpu_plane_align import TOL, _rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plane_align_demo") / "plane_align_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "plane_align_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_prints_the_restatement_s_aligner(demo):
    lines = [l.split() for l in subprocess.check_output([demo], text=True, timeout=120).split("\n") if l]
    rows = lambda tag: np.array([l[1:] for l in lines if l[0] == tag], dtype=np.float64)
    points, src, se3, pix, depth = rows("POINT"), rows("SOURCE"), rows("SE3")[0], rows("ROW"), rows("DEPTH")
    n = len(points)
    assert n == 120 and len(src) == n and len(pix) == n and len(depth) == 2
    sources = np.zeros(n, PR.SOURCE_DT)
    sources["src_kf"] = src[:, 0]
    sources["center_nc"], sources["one_right_nc"], sources["one_down_nc"] = src[:, 1:4], src[:, 4:7], src[:, 7:10]
    poses = np.stack([PR.IDENTITY, PR.IDENTITY])
    poses[1, 9:] = 0.1, 0.0, 0.05
    meas = np.zeros(n + n // 2, PR.MEAS_DT)
    meas["kf"][n:], meas["point"] = 1, np.concatenate([np.arange(n), np.arange(1, n, 2)])
    table = PR.samples(5, n, 100)
    g = PR.guards(points, table, 0.05)
    assert g["score_gap"] >= 1e-6 and g["threshold_gap"] >= 1e-9 and g["eigen_gap"] >= 1e-3 and g["normal_z"] >= 1e-3
    r = PR.calc_plane_aligner(points, table, 0.05)
    assert [l for l in lines if l[0] == "STATUS"][0] == ["STATUS", "0", "INLIERS", str(r["n_inliers"]), "BEST_TRIAL", str(r["best_trial"]),
                                                        "SKIPPED", "0"]
    assert r["n_inliers"] == 90
    poses_r, points_r, (right_r, down_r) = PR.apply_global_transform(r["se3"], poses, points, sources)
    depth_r = PR.scene_depth(poses_r, points_r, meas)
    figures = dict(R=_rel(se3[:9], r["se3"][:9]), t=_rel(se3[9:], r["se3"][9:]), right=_rel(pix[:, :3], right_r), down=_rel(pix[:, 3:], down_r),
                   depth=_rel(depth[:, :2], depth_r[:, :2]))
    print(figures)
    assert max(figures.values()) <= TOL and np.array_equal(depth[:, 2], depth_r[:, 2])
