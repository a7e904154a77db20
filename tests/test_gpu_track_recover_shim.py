"""-m gpu: builds examples/track_recover_demo.cc (ptam::MapTracker::TrackFramesRecoverBatch, ptam::TrackState and
Relocaliser::SetKeyFramePose of ptam_shim.hpp) with g++, runs it once, and feeds the frames and the map it prints through the Python
binding of ptam_track_frames_recover_batch: every printed result, info and state must be the binding's, byte for byte — the same
library on the same inputs — and the three branches must all have been taken."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ptam_cg_amd import _abi, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, ROUNDS, CAMERAS = (160, 120), 4, 3


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("track_recover_demo") / "track_recover_demo")
    lib_dir = os.path.join(ROOT, "ptam_cg_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "track_recover_demo.cc"),
                           "-L" + lib_dir, "-lptam_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_shim_recover_batch_prints_what_the_binding_computes(demo, hip):
    lines = [l.split() for l in subprocess.check_output([demo], text=True, timeout=120).split("\n") if l]
    frames = [np.frombuffer(bytes.fromhex(l[3]), np.uint8).reshape(SIZE[::-1]) for l in lines if l[0] == "FRAME"]
    points = np.frombuffer(b"".join(bytes.fromhex(l[3]) for l in lines if l[0] == "POINT"), host.PVS_POINT_DT)
    centers = np.array([[int(l[1]), int(l[2])] for l in lines if l[0] == "POINT"], np.int32)
    assert len(frames) == 4 and len(points) == len(centers) >= 4
    printed = {(l[0], int(l[1]), int(l[2])): bytes.fromhex(l[3]) for l in lines if l[0] in ("RESULT", "INFO", "STATE")}
    assert len(printed) == 3 * ROUNDS * CAMERAS
    identity = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    moved = identity.copy()
    moved[9] = 0.02

    class Cam:
        def __init__(self, estimator):
            self.ctx = host.Context(lib=hip, size=SIZE)
            self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(frames[0])
            self.kf3 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(frames[3])
            self.tr = host.Tracker(self.ctx, len(points) + 1)
            self.tr.set_map(points["world"], points["pixel_right_w"], points["pixel_down_w"], self.kf0, np.zeros(len(points), np.int32), centers)
            self.rel = host.Relocaliser(self.ctx, 4)
            self.rel.add_batch([self.kf0, self.kf3], [identity, identity])
            self.rel.set_poses(1, [moved])
            self.kf = host.KeyFrame(self.ctx)
            self.est = host.RotationEstimator(self.ctx) if estimator else None
            self.d = [host.DevBuf(self.ctx, f) for f in frames]
            self.state = self.tr.track_state(identity)

    cams = [Cam(i != 1) for i in range(CAMERAS)]
    for c in cams[1:]:
        c.state.lost_frames, c.state.quality = 3, _abi.TRACK_BAD
    branches = set()
    for r in range(ROUNDS):
        so = cams[0].tr.state_opts(**({"reloc_max_score": 0.0} if r < ROUNDS // 2 else {}))
        res, infos = host.Tracker.track_frames_recover_batch([c.tr for c in cams], [c.kf for c in cams], [c.d[r % 4] for c in cams],
                                                             [c.state for c in cams], [c.est for c in cams], [c.rel for c in cams], None, so)
        for i, c in enumerate(cams):
            assert printed[("RESULT", r, i)] == res[i].tobytes(), (r, i)
            assert printed[("STATE", r, i)] == bytes(c.state), (r, i)
            inf = _abi.TrackFrameStateInfo.from_buffer_copy(printed[("INFO", r, i)])
            f = infos[i]
            assert (inf.branch, inf.closest_kf, inf.closest_kf_dist, inf.need_new_keyframe, inf.want_keyframe) == \
                (f["branch"], f["closest_kf"], f["closest_kf_dist"], f["need_new_keyframe"], f["want_keyframe"]), (r, i)
            assert bytes(inf.frame.pose_in) == f["pose_in"].tobytes() and bytes(inf.reloc.pose) == f["reloc"]["pose"].tobytes(), (r, i)
            assert (inf.reloc.best, inf.reloc.good, inf.reloc.best_ssd, inf.reloc.align.score) == \
                (f["reloc"]["best"], f["reloc"]["good"], f["reloc"]["best_ssd"], f["reloc"]["align"]["score"]), (r, i)
            assert inf.frame.align.score == f["align"]["score"] and np.array_equal(np.array(inf.frame.align.rotation).reshape(3, 3), f["align"]["rotation"])
            assert (inf.frame.try_coarse, inf.frame.coarse_max, inf.frame.coarse_range) == (f["try_coarse"], f["coarse_max"], f["coarse_range"])
            branches.add(f["branch"])
            want = (_abi.FRAME_TRACKED if i == 0 or r == 3 else _abi.FRAME_RECOVERY_FAILED if r < 2 else _abi.FRAME_RECOVERED)
            assert f["branch"] == want, (r, i)
            if f["want_keyframe"]:
                c.state.last_keyframe_dropped = c.state.frame
    assert branches == {_abi.FRAME_TRACKED, _abi.FRAME_RECOVERED, _abi.FRAME_RECOVERY_FAILED}
    assert np.array_equal(cams[1].rel.bank_poses(), np.stack([identity, moved]))
    for c in cams:
        for o in [c.tr, c.kf, c.kf0, c.kf3, c.rel] + ([c.est] if c.est else []):
            o.close()
        for d in c.d:
            d.free()
        c.ctx.close()
