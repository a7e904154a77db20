"""Times a batch of cameras tracked with the rotation estimator on, over the closed 64-frame sequence, and prints one JSON line.
Per --nb cameras (each in a context of its own, camera i a few frames ahead of camera i - 1), frames/s and us per frame of
  a  ptam_track_frames_batch: one chain of launches and one wait per camera for the whole batch
  b  ptam_track_frame_sbi, camera after camera (two waits per frame)
  c  the composed batch: per camera ptam_make_keyframe_lite_dev + ptam_sbi_make + ptam_sbi_calc_rotation (a wait each) + the host's
     ptam_motion_predict_sbi, then ptam_track_map_frames_batch (which makes the keyframes again), then ptam_motion_update
  d  ptam_track_map_frames_batch alone, from the true poses (what the batch chain itself costs; runs on any build of the library)
A pass is 64 steps of the whole batch; host clock around the pass (every call ends in the wait for its results).  Reported: the median
of --passes passes after one warm-up pass, and their spread (min, max).  The paths are run in turn, pass by pass, so that drift of
the machine hits all alike.  The calls go through ctypes with their arguments prepared: about a microsecond of interpreter per call,
which b and c pay per camera and a per batch.  `lost`: frames with fewer than 50 measurements in the timed passes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host, synth  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402

N_FRAMES = 64


def load_lib():
    """the library; a build from before ptam_track_frames_batch (PTAM_HIP_LIB) is accepted for the paths b, c and d"""
    try:
        return load()
    except RuntimeError:
        from ptam_cg_amd import _lib
        b = _abi.bind(C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL), "ptam_")
        if set(b.missing) - {"track_frames_batch", "motion_predict_sbi_dev"}:
            raise
        return b


class Cam:
    def __init__(self, lib, kim, kpose):
        self.ctx = host.Context(lib=lib)
        self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(kim)
        m = synth.make_sequence_map([self.kf0.level(l) for l in range(4)], kpose)
        self.tr = host.Tracker(self.ctx, len(m["world"]))
        self.tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], self.kf0, m["src_level"], m["center"])
        self.tr.set_shuffle(m["shuffle_levels"], m["shuffle_fine"])
        self.kf = host.KeyFrame(self.ctx)
        self.est = host.RotationEstimator(self.ctx)
        self.sbi = [host.SmallBlurryImage(self.ctx), host.SmallBlurryImage(self.ctx)]
        self.model = _abi.MotionModel()
        self.al = _abi.SbiAlignment()
        self.res = np.zeros(1, host.TRACKMAP_RESULT_DT)
        self.last = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[1, 4, 16, 64, 128])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--paths", default="abcd")
    a = ap.parse_args()
    lib = load_lib()
    has_new = lib.has("track_frames_batch")
    paths = [p for p in a.paths if p != "a" or has_new]
    frames, poses, kim, kpose = synth.make_tracking_frames(N_FRAMES, period=N_FRAMES)
    nb_max = max(a.nb)
    cams = [Cam(lib, kim, kpose) for _ in range(nb_max)]
    d_frames = [host.DevBuf(cams[0].ctx, f) for f in frames]       # (device memory: every context of the device reads it)
    raw = lambda h: h.value if hasattr(h, "value") else int(h)
    fp = [raw(d.p) for d in d_frames]
    opts = cams[0].tr.opts()
    p_opts = host._ptr(opts)
    out = {"passes": a.passes, "frames_per_pass": N_FRAMES, "nb": {}}

    for nb in a.nb:
        cs = cams[:nb]
        stride = max(1, N_FRAMES // nb) if nb <= N_FRAMES else 1
        first = [(i * stride) % N_FRAMES for i in range(nb)]
        trs = (C.c_void_p * nb)(*[raw(c.tr.h) for c in cs])
        kfs = (C.c_void_p * nb)(*[raw(c.kf.h) for c in cs])
        ests = (C.c_void_p * nb)(*[raw(c.est.h) for c in cs])
        res = np.zeros(nb, host.TRACKMAP_RESULT_DT)
        p_res = host._ptr(res)
        models = (_abi.MotionModel * nb)()
        pose_in = np.zeros((nb, 12))
        p_pose = host._pd(pose_in)
        dis = [(C.c_void_p * nb)(*[fp[(first[i] + s) % N_FRAMES] for i in range(nb)]) for s in range(N_FRAMES)]
        lost = {p: 0 for p in paths}

        def reset(path):
            for i, c in enumerate(cs):
                start = poses[(first[i] - 1) % N_FRAMES]        # (closed trajectory: the pose of the frame before the first)
                lib.motion_reset(C.byref(c.model), host._pd(np.ascontiguousarray(start)))
                C.memmove(C.byref(models[i]), C.byref(c.model), C.sizeof(_abi.MotionModel))
                lib.rotation_estimator_reset(c.est.h)
                c.last = None

        def step_a(s):
            rc = lib.track_frames_batch(nb, trs, kfs, dis[s], models, ests, p_opts, p_res, None)
            assert rc == 0, rc
            return res["n_meas"]

        def step_b(s):
            n = []
            for i, c in enumerate(cs):
                rc = lib.track_frame_sbi(c.tr.h, c.kf.h, dis[s][i], C.byref(c.model), c.est.h, p_opts, host._ptr(c.res), C.byref(c.al))
                assert rc == 0, rc
                n.append(c.res[0]["n_meas"])
            return n

        def step_c(s):
            for i, c in enumerate(cs):
                this = 0 if c.last is None else 1 - c.last
                rc = lib.make_keyframe_lite_dev(c.ctx.h, c.kf.h, dis[s][i])
                rc |= lib.sbi_make(c.sbi[this].h, c.kf.h, 0.75)
                rc |= lib.sbi_calc_rotation(c.sbi[this].h, c.sbi[this if c.last is None else c.last].h, 6, C.byref(c.al))
                assert rc == 0, rc
                c.last = this
                lib.motion_predict_sbi(C.byref(c.model), c.al.rotation)
                pose_in[i] = c.model.pose
            rc = lib.track_map_frames_batch(nb, trs, kfs, dis[s], p_pose, p_opts, p_res)
            assert rc == 0, rc
            for i, c in enumerate(cs):
                lib.motion_update(C.byref(c.model), C.c_void_p(res.ctypes.data + i * res.itemsize))
            return res["n_meas"]

        def step_d(s):
            for i in range(nb):
                pose_in[i] = poses[(first[i] + s) % N_FRAMES]
            rc = lib.track_map_frames_batch(nb, trs, kfs, dis[s], p_pose, p_opts, p_res)
            assert rc == 0, rc
            return res["n_meas"]

        steps = {"a": step_a, "b": step_b, "c": step_c, "d": step_d}
        times = {p: [] for p in paths}
        for rep in range(a.passes + 1):
            for p in paths:
                reset(p)
                t0 = time.perf_counter()
                for s in range(N_FRAMES):
                    n = steps[p](s)
                    if rep:
                        lost[p] += int(sum(1 for v in n if v < 50))
                dt = time.perf_counter() - t0
                if rep:
                    times[p].append(dt)
        row = {}
        for p in paths:
            med = statistics.median(times[p])
            per = lambda t: round(t / (nb * N_FRAMES) * 1e6, 2)
            row[p] = {"frames_per_s": round(nb * N_FRAMES / med), "us_per_frame": per(med), "us_per_frame_min_max": [per(min(times[p])), per(max(times[p]))],
                      "lost": lost[p]}
        out["nb"][str(nb)] = row
        print("nb", nb, json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
