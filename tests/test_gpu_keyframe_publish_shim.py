"""-m gpu: builds examples/publish_keyframes_demo.cc (ptam::MapSnapshot::EnableKeyFrames, ptam::Relocaliser::TakeKeyFrames beside
MapTracker::TakeMap, two threads, a lost camera that recovers through TrackFramesRecoverBatch) with g++, runs it once, and fills a
bank by hand through the Python binding from the frames it prints: the demo's bank — poses and images — must be that bank, byte for
byte, and its poses the map's own pose table."""
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (160, 120)


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("publish_keyframes_demo") / "publish_keyframes_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "publish_keyframes_demo.cc"), "-L" + lib_dir, "-lptam_hip", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_the_demo_s_bank_is_the_hand_filled_one(demo, hip):
    lines = [l.split() for l in subprocess.check_output([demo], text=True, timeout=120).split("\n") if l]
    frames = [np.frombuffer(bytes.fromhex(l[2]), np.uint8).reshape(SIZE[::-1]) for l in lines if l[0] == "FRAME"]
    printed = {(l[0], int(l[1])): bytes.fromhex(l[2]) for l in lines if l[0] in ("KFPOSE", "BANKPOSE", "SMALL", "TMPL", "JACS")}
    summary = [l for l in lines if l[0] == "PUBLISHKEYFRAMES"][0]
    s = dict(zip(summary[1::2], summary[2::2]))
    assert len(frames) == 4
    assert (int(s["generation"]), int(s["keyframes"]), int(s["bank"])) == (3, 2, 2)
    assert int(s["recovered"]) >= 1 and int(s["takes"]) >= 1
    # the poses: the bank's are the map's own table, and the global transform moved both off the uploaded ones
    identity = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    for i in range(2):
        assert printed[("BANKPOSE", i)] == printed[("KFPOSE", i)], i
    poses = np.stack([np.frombuffer(printed[("KFPOSE", i)], np.float64) for i in range(2)])
    assert not np.array_equal(poses[0], identity) and np.array_equal(poses[:, :9], np.stack([identity[:9]] * 2))
    # the images: keyframes 0 and 1 are frames 0 and 3
    ctx = host.Context(lib=hip, size=SIZE)
    kfs = [host.KeyFrame(ctx).MakeKeyFrame_Lite(frames[k]) for k in (0, 3)]
    rel = host.Relocaliser(ctx, 8)
    rel.add_batch(kfs, poses)
    for i in range(2):
        e = rel.read(i)
        assert (printed[("SMALL", i)], printed[("TMPL", i)], printed[("JACS", i)]) == (e["small"].tobytes(), e["tmpl"].tobytes(), e["jacs"].tobytes()), i
    assert rel.bank_poses().tobytes() == printed[("BANKPOSE", 0)] + printed[("BANKPOSE", 1)]
    for o in [rel] + kfs:
        o.close()
    ctx.close()
