"""Times ptam_track_frames_recover_batch over the closed 64-frame sequence (the cameras of time_track_batch.py, each with a relocaliser
of 16 keyframes: frames 0, 4, .. 60 at their true poses) and prints one JSON line.  Per --nb cameras, us per frame of
  p    ptam_track_frames_batch, no camera lost (the existing entry; its min-max is its run-to-run spread)
  n    ptam_track_frames_recover_batch, no camera lost, every camera with its bank (the closest keyframe is walked on the host)
  m    the same without banks
  r16  ptam_track_frames_recover_batch, every step one camera in 16 is made lost (lost_frames = 3) and recovers in the chain
  q16  the same from the existing entries: ptam_track_frames_batch for the cameras that track; for the lost ones
       ptam_make_keyframe_lite_dev + ptam_relocalise camera after camera, then ptam_track_map_frames_batch from the relocalisers' poses
       with the doubled coarse options, the model set by hand
  rall / qall  the same with every camera lost every step
A pass is 64 steps of the whole batch, host clock around it; reported: the median of --passes passes after one warm-up pass, and
min / max.  The paths are run in turn, pass by pass.  `lost`: tracked or recovered frames with fewer than 50 measurements; `failed`:
recoveries that were not good."""
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

N_FRAMES, BANK = 64, 16


class Cam:
    def __init__(self, lib, kim, kpose, bank_kfs, bank_poses):
        self.ctx = host.Context(lib=lib)
        self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(kim)
        m = synth.make_sequence_map([self.kf0.level(l) for l in range(4)], kpose)
        self.tr = host.Tracker(self.ctx, len(m["world"]))
        self.tr.set_map(m["world"], m["pixel_right_w"], m["pixel_down_w"], self.kf0, m["src_level"], m["center"])
        self.tr.set_shuffle(m["shuffle_levels"], m["shuffle_fine"])
        self.kf = host.KeyFrame(self.ctx)
        self.est = host.RotationEstimator(self.ctx)
        self.rel = host.Relocaliser(self.ctx, BANK)
        self.rel.add_batch(bank_kfs, bank_poses)
        self.ctx.sync()
        self.reloc = _abi.RelocResult()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--paths", nargs="+", default=["p", "n", "m", "r16", "q16", "rall", "qall"])
    a = ap.parse_args()
    lib = load()
    frames, poses, kim, kpose = synth.make_tracking_frames(N_FRAMES, period=N_FRAMES)
    ctx0 = host.Context(lib=lib)
    bank_poses = np.ascontiguousarray(poses[::N_FRAMES // BANK])
    bank_kfs = [host.KeyFrame(ctx0).MakeKeyFrame_Lite(frames[k]) for k in range(0, N_FRAMES, N_FRAMES // BANK)]
    ctx0.sync()
    cams = [Cam(lib, kim, kpose, bank_kfs, bank_poses) for _ in range(max(a.nb))]
    d_frames = [host.DevBuf(cams[0].ctx, f) for f in frames]       # (device memory: every context of the device reads it)
    raw = lambda h: h.value if hasattr(h, "value") else int(h)
    fp = [raw(d.p) for d in d_frames]
    opts = cams[0].tr.opts()
    p_opts = host._ptr(opts)
    doubled = cams[0].tr.opts()
    doubled["try_coarse"], doubled["coarse_max"], doubled["coarse_range"] = 1, 2 * opts["coarse_max"], 2 * opts["coarse_range"]
    p_doubled = host._ptr(doubled)
    p_bank_poses = host._ptr(bank_poses)
    out = {"passes": a.passes, "frames_per_pass": N_FRAMES, "bank": BANK, "nb": {}}

    for nb in a.nb:
        cs = cams[:nb]
        stride = max(1, N_FRAMES // nb) if nb <= N_FRAMES else 1
        first = [(i * stride) % N_FRAMES for i in range(nb)]
        arr = lambda xs: (C.c_void_p * len(xs))(*xs)
        trs, kfs, ests = arr([raw(c.tr.h) for c in cs]), arr([raw(c.kf.h) for c in cs]), arr([raw(c.est.h) for c in cs])
        banks, scr = arr([raw(c.rel.h) for c in cs]), arr([raw(c.rel.scratch.h) for c in cs])
        res = np.zeros(nb, host.TRACKMAP_RESULT_DT)
        p_res = host._ptr(res)
        models = (_abi.MotionModel * nb)()
        states = (_abi.TrackState * nb)()
        infos = (_abi.TrackFrameStateInfo * nb)()
        dis = [arr([fp[(first[i] + s) % N_FRAMES] for i in range(nb)]) for s in range(N_FRAMES)]
        # who is made lost at step s, and the argument arrays of the two groups for the composed path
        lost_of = {"16": [[i for i in range(nb) if (i + s) % 16 == 0] for s in range(N_FRAMES)], "all": [list(range(nb))] * N_FRAMES}
        groups = {}
        for key, per_step in lost_of.items():
            groups[key] = []
            for s, L in enumerate(per_step):
                O = [i for i in range(nb) if i not in set(L)]
                pick = lambda idx, xs: arr([xs[i] for i in idx])
                g = {"L": L, "O": O}
                for name, idx in (("L", L), ("O", O)):
                    g[name + "_args"] = (pick(idx, trs), pick(idx, kfs), pick(idx, dis[s]), pick(idx, ests)) if idx else None
                g["O_models"] = (_abi.MotionModel * max(len(O), 1))()
                g["O_res"] = np.zeros(max(len(O), 1), host.TRACKMAP_RESULT_DT)
                g["L_res"] = np.zeros(max(len(L), 1), host.TRACKMAP_RESULT_DT)
                g["L_pose"] = np.zeros((max(len(L), 1), 12))
                groups[key].append(g)
        counts = {p: {"lost": 0, "failed": 0} for p in a.paths}

        def reset(path):
            for i, c in enumerate(cs):
                start = np.ascontiguousarray(poses[(first[i] - 1) % N_FRAMES])       # (closed trajectory: the pose of the frame before the first)
                lib.track_state_reset(C.byref(states[i]), host._pd(start))
                C.memmove(C.byref(models[i]), C.byref(states[i].model), C.sizeof(_abi.MotionModel))
                lib.rotation_estimator_reset(c.est.h)

        def step_p(s, tally):
            rc = lib.track_frames_batch(nb, trs, kfs, dis[s], models, ests, p_opts, p_res, None)
            assert rc == 0, rc
            tally["lost"] += int((res["n_meas"] < 50).sum())

        def recover(s, with_banks, key, tally):
            if key:
                for i in lost_of[key][s]:
                    states[i].lost_frames = 3
            rc = lib.track_frames_recover_batch(nb, trs, kfs, dis[s], states, ests, banks if with_banks else None, scr if with_banks else None,
                                                p_opts, None, p_res, infos)
            assert rc == 0, rc
            if key:
                failed = sum(1 for i in lost_of[key][s] if infos[i].branch != _abi.FRAME_RECOVERED)
                tally["failed"] += failed
                tally["lost"] += int((res["n_meas"] < 50).sum()) - failed
            else:
                tally["lost"] += int((res["n_meas"] < 50).sum())

        def composed(s, key, tally):
            g = groups[key][s]
            L, O = g["L"], g["O"]
            for i in L:
                states[i].lost_frames = 3        # (the same bookkeeping as the new call's side)
            if O:
                mo = g["O_models"]
                for k, i in enumerate(O):
                    C.memmove(C.byref(mo[k]), C.byref(models[i]), C.sizeof(_abi.MotionModel))
                t_, k_, d_, e_ = g["O_args"]
                rc = lib.track_frames_batch(len(O), t_, k_, d_, mo, e_, p_opts, host._ptr(g["O_res"]), None)
                assert rc == 0, rc
                for k, i in enumerate(O):
                    C.memmove(C.byref(models[i]), C.byref(mo[k]), C.sizeof(_abi.MotionModel))
                tally["lost"] += int((g["O_res"][:len(O)]["n_meas"] < 50).sum())
            if L:
                for k, i in enumerate(L):
                    c = cs[i]
                    rc = lib.make_keyframe_lite_dev(c.ctx.h, c.kf.h, dis[s][i])
                    rc |= lib.relocalise(c.rel.h, c.rel.scratch.h, c.kf.h, p_bank_poses, 2.5, 9e6, C.byref(c.reloc), None)
                    assert rc == 0, rc
                    tally["failed"] += 0 if c.reloc.good else 1
                    g["L_pose"][k] = c.reloc.pose
                t_, k_, d_, _ = g["L_args"]
                rc = lib.track_map_frames_batch(len(L), t_, k_, d_, host._pd(g["L_pose"]), p_doubled, host._ptr(g["L_res"]))
                assert rc == 0, rc
                for k, i in enumerate(L):
                    lib.motion_recover(C.byref(models[i]), cs[i].reloc.pose)
                    models[i].pose[:] = g["L_res"][k]["pose"].tolist()
                    models[i].just_recovered = 0
                    states[i].lost_frames = 0
                tally["lost"] += int((g["L_res"][:len(L)]["n_meas"] < 50).sum())

        steps = {"p": step_p, "n": lambda s, t: recover(s, True, None, t), "m": lambda s, t: recover(s, False, None, t),
                 "r16": lambda s, t: recover(s, True, "16", t), "q16": lambda s, t: composed(s, "16", t),
                 "rall": lambda s, t: recover(s, True, "all", t), "qall": lambda s, t: composed(s, "all", t)}
        times = {p: [] for p in a.paths}
        for rep in range(a.passes + 1):
            for p in a.paths:
                reset(p)
                tally = {"lost": 0, "failed": 0}
                t0 = time.perf_counter()
                for s in range(N_FRAMES):
                    steps[p](s, tally)
                dt = time.perf_counter() - t0
                if rep:
                    times[p].append(dt)
                    for k, v in tally.items():
                        counts[p][k] += v
        row = {}
        per = lambda t: round(t / (nb * N_FRAMES) * 1e6, 2)
        for p in a.paths:
            row[p] = {"us_per_frame": per(statistics.median(times[p])), "us_per_frame_min_max": [per(min(times[p])), per(max(times[p]))], **counts[p]}
        out["nb"][str(nb)] = row
        print("nb", nb, json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
