"""-m gpu: builds examples/resident_map_demo.cc (ptam::ResidentMap of ptam_shim.hpp) with g++, runs it on a map written by the test
(the scene of tests/map_refind_ref.make_scene), and checks its output file against host.ResidentMap running the same iteration on
the same map, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import map_edit_ref as E
from tests import map_refind_ref as F
from tests.test_gpu_resident_map import UPLOAD_KEYS, kf_rows
from tests.test_gpu_resident_map_refind import scene_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYFRAME, NEW_POINTS, QUEUE = _abi.MAP_REFIND_KEYFRAME, _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_map_demo") / "resident_map_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "resident_map_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_matches_python_calls(hip, demo, tmp_path):
    ctx = host.Context(lib=hip)
    scene = F.make_scene(ctx)
    points, new = F.make_work(NEW_POINTS, scene)
    h = scene_map(scene, points, new_queue=new)
    K, target, source = len(scene["kfs"]), 5, _abi.SRC_EPIPOLAR
    pose = scene["poses"][3].copy()
    pose[11] += 3e-4 * scene["z"]
    made = E.make_made(14, 80)
    m, rf = host.ResidentMap(ctx), host.ReFinder(ctx)
    m.upload(kfs=scene["kfs"], **{k: h[k] for k in UPLOAD_KEYS if not k.endswith("_count")})
    n_out, refound = [], []
    ba = m.bundle_adjust(_abi.MAP_BA_RECENT, deterministic=1)
    m.apply_outliers(ba["outliers"])
    n_out.append(ba["n_outliers"])
    refound.append(m.refind(rf, NEW_POINTS, lists=False))
    ba = m.bundle_adjust(_abi.MAP_BA_ALL, deterministic=1)
    m.apply_outliers(ba["outliers"])
    n_out.append(ba["n_outliers"])
    refound.append(m.refind(rf, QUEUE, lists=False))
    b = m.handle_bad_points(kept=True)
    rows = kf_rows(13, b["n_kept"], 200)          # (drawn for the compacted table: the demo gets the same rows)
    m.add_keyframe(pose, 0, rows, kf=scene["kfs"][1])
    refound.append(m.refind(rf, KEYFRAME, [K], lists=False))
    m.add_points(K, target, made, source)
    depth = m.scene_depth()
    counts, tab = m.counts(), m.tables()
    rf.close()
    m.close()
    scene["close"]()
    ctx.close()

    a_img, b_img = synth.make_frame_pair()
    height, width = a_img.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([K, len(h["points3"]), len(h["meas"]), len(h["never"]), len(new), len(made), len(rows), width, height, target, source, 0],
                         np.int32).tobytes())
        for a in (b_img, a_img, h["poses"], h["fixed"], h["points3"], h["points"], h["sources"], h["bad"], h["meas"], h["never"], new, made, pose, rows):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([demo, fin, fout], text=True, timeout=300)
    assert out.startswith("RESIDENTMAP kf %d points %d meas %d never %d new %d failure %d outliers %d+%d refound %d+%d+%d removed %d " % (
        counts["n_kf"], counts["n_points"], counts["n_meas"], counts["n_never"], counts["n_new"], counts["n_failure"], n_out[0], n_out[1],
        refound[0]["n_found"], refound[1]["n_found"], refound[2]["n_found"], b["n_removed"]))
    want = [np.array([counts[k] for k in ("n_kf", "n_points", "n_meas", "n_never", "n_new", "n_failure")], np.int32), np.array(n_out, np.int32)]
    want += [np.array([r[k] for k in F.COUNTS], np.int32) for r in refound]
    want += [np.array([b[k] for k in E.BAD_COUNTS], np.int32), b["kept"]] + [tab[k] for k in host.ResidentMap.TABLES] + [depth]
    assert open(fout, "rb").read() == b"".join(np.ascontiguousarray(w).tobytes() for w in want)
    assert refound[0]["n_pairs"] > 0 and refound[2]["n_pairs"] == b["n_kept"] and b["n_removed"] > 0 and counts["n_kf"] == K + 1
