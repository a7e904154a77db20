"""-m gpu: builds examples/init_map_demo.cc (ptam::ResidentMap::InitFromStereo of ptam_shim.hpp: trails, the one call, Publish, TakeMap,
one tracked frame) with g++, runs it on the frames of tests/init_map_ref.stereo_sequence, and compares what it prints — status, counts,
the tracker's pose, a hash of the tables — with the Python call on the same frames."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import init_map_ref as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TRAILS, MAX_BUNDLES, THRESHOLD, SEEDS = 1000, 20, 70.0, (3, 5)
HASHED = ("poses", "points3", "points", "sources", "bad", "meas", "new_queue")


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("init_map_demo") / "init_map_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "init_map_demo.cc"), "-L" + lib_dir, "-lptam_hip",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def fnv1a(tables):
    """FNV-1a over the tables' bytes, as the demo hashes them"""
    h = 1469598103934665603
    for t in tables:
        for b in np.ascontiguousarray(t).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_shim_prints_the_python_call(hip, demo, tmp_path):
    frames, _ = IR.stereo_sequence()
    fin = str(tmp_path / "frames.bin")
    with open(fin, "wb") as f:
        f.write(np.array([IR.SIZE[0], IR.SIZE[1], len(frames), MAX_TRAILS, MAX_BUNDLES], np.int32).tobytes() + np.array([THRESHOLD]).tobytes()
                + np.array(SEEDS, np.uint64).tobytes())
        for im in frames:
            f.write(im.tobytes())
    lines = [l.split() for l in subprocess.check_output([demo, fin], text=True, timeout=120).split("\n") if l]
    got = {l[0]: l[1:] for l in lines}
    ctx = host.Context(lib=hip, size=IR.SIZE)
    first, second, tr = IR.run_trails(ctx, frames, THRESHOLD, MAX_TRAILS)
    m = host.ResidentMap(ctx)
    r = m.InitFromStereo(first, second, trails=tr, opts=m.init_opts(max_bundles=MAX_BUNDLES, ba=dict(deterministic=1), homography=dict(seed=SEEDS[0]),
                                                                    plane=dict(seed=SEEDS[1])))
    assert r["status"] == _abi.INIT_MAP_OK
    assert [int(x) for x in got["ALIVE"]] == [len(tr.read())]
    assert [int(x) for x in got["INIT"]] == [1, r["status"], r["n_matches"], r["n_made"], r["n_bundles"], r["n_outliers"], r["n_epipolar"],
                                             r["plane"]["status"], r["plane"]["n_inliers"]]
    c = r["counts"]
    assert [int(x) for x in got["COUNTS"]] == [c["n_kf"], c["n_points"], c["n_meas"], c["n_never"], c["n_new"], c["n_failure"]]
    assert np.array([float(x) for x in got["POSE"]]).tobytes() == r["tracker_pose"].tobytes()
    tab = m.tables()
    assert int(got["TABLES"][0]) == fnv1a([tab[k] for k in HASHED])
    # the same hand-over and frame through the binding
    snap, trk = host.MapSnapshot(ctx, c["n_points"]), host.Tracker(ctx, c["n_points"])
    pub = m.publish(snap)
    took = trk.take_map(snap)
    assert [int(x) for x in got["TAKE"]] == [pub["n_points"], took["n_points"], took["n_new"]] and took["n_new"] == c["n_points"]
    t = trk.TrackMap(second, r["tracker_pose"])
    print("tracked:", t["n_meas"], list(t["found"]))
    assert [int(x) for x in got["TRACK"]] == [t["n_meas"]] + [int(x) for x in t["found"]] and t["n_meas"] > 0
    assert np.array([float(x) for x in got["TRACKED"]]).tobytes() == np.asarray(t["pose"], dtype=np.float64).tobytes()
    for x in (trk, snap, m, tr):
        x.close()
    ctx.close()
