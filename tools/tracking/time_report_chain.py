"""Times ptam_track_frames_report_batch — the recover batch with the frames' reports filled inside the chain and the frames' two
random orders drawn there — against the sequence of calls it replaces, over the closed 64-frame sequence (1 244 points; the cameras of
time_track_recover_batch.py without banks, their maps taken from a snapshot), and prints one JSON line.  Per --nb cameras, us per frame of
  recover   ptam_track_frames_recover_batch alone, the shuffles set once (the existing entry: its min-max is the run-to-run spread)
  composed  per camera two numpy permutations (Generator.permutation) + ptam_tracker_set_shuffle, then ptam_track_frames_recover_batch,
            then ptam_tracker_report_frames for all cameras — what a caller does today; runs with any library that has these entries
            (PTAM_HIP_LIB: the parent commit's)
  report    ptam_track_frames_report_batch with reports, the shuffles set once (what the report in the chain saves)
  chain     ptam_track_frames_report_batch with reports and seeds (the draw on the device as well)
--tile T runs the same legs on the sequence's map T times over (41: 51 004 points; the frames are the sequence's).
A pass is 64 steps of the whole batch, host clock around it; reported: the median of --passes passes after one warm-up pass, and
min / max.  The paths are run in turn, pass by pass.
`draw`: at 1 244 and at --big points (a synthetic map), us per call of
  device    ptam_tracker_draw_shuffles, --draws calls enqueued back to back and one wait (the kernel alone on the queue)
  host      two numpy permutations + ptam_tracker_set_shuffle, each call behind the other (the validation, the copy, the upload)"""
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
SEED = 0x2545F4914F6CDD1D


def load_any():
    """-> (the library, whether it has this tree's entries): a library of the parent commit still runs `recover` and `composed`"""
    try:
        return load(), True
    except RuntimeError as e:
        if "lacks symbols" not in str(e):
            raise
        from ptam_cg_amd import _lib
        return _abi.bind(C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL), "ptam_"), False


def map_tables(m):
    """whole-map tables (ResidentMap.upload) of a tracking map whose points all come from keyframe 0"""
    n = len(m["world"])
    pts = np.zeros(n, host.MAP_REFIND_POINT_DT)
    pts["pv"]["world"], pts["pv"]["pixel_right_w"], pts["pv"]["pixel_down_w"] = m["world"], m["pixel_right_w"], m["pixel_down_w"]
    pts["src_level"] = m["src_level"]
    c = np.asarray(m["center"], np.int32).reshape(n, 2)
    pts["center_x"], pts["center_y"] = c[:, 0], c[:, 1]
    meas = np.zeros(n, host.MAP_MEAS_DT)
    meas["point"], meas["level"] = np.arange(n), m["src_level"]
    pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None]
    return dict(poses=pose, fixed=np.ones(1, np.uint8), points3=np.ascontiguousarray(pts["pv"]["world"]), points=pts,
                sources=np.zeros(n, host.MAP_POINT_SOURCE_DT), bad=np.zeros(n, np.uint8), meas=meas)


class Cam:
    def __init__(self, lib, kim, kpose, tile=1):
        self.ctx = host.Context(lib=lib)
        self.kf0 = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(kim)
        self.map = synth.make_sequence_map([self.kf0.level(l) for l in range(4)], kpose)
        if tile > 1:       # the same map `tile` times over: a large map the sequence still tracks
            self.map = {k: np.concatenate([v] * tile) for k, v in self.map.items() if k not in ("shuffle_levels", "shuffle_fine")}
            rng = np.random.default_rng(tile)
            n = len(self.map["world"])
            self.map["shuffle_levels"], self.map["shuffle_fine"] = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
        self.n = len(self.map["world"])
        self.rmap = host.ResidentMap(self.ctx)
        self.rmap.upload(kfs=[self.kf0], **map_tables(self.map))
        self.snap = host.MapSnapshot(self.ctx, self.n)
        self.rmap.publish(self.snap)
        self.tr = host.Tracker(self.ctx, self.n)
        self.tr.take_map(self.snap)
        self.tr.set_shuffle(self.map["shuffle_levels"], self.map["shuffle_fine"])
        self.kf = host.KeyFrame(self.ctx)
        self.est = host.RotationEstimator(self.ctx)
        self.report = host.FrameReport(self.ctx, self.n)
        self.ctx.sync()


def time_draws(lib, ctx, kf0, n, draws):
    rng = np.random.default_rng(n)
    tr = host.Tracker(ctx, n)
    tr.set_map(rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)), kf0, np.zeros(n, np.int32), np.full((n, 2), 40, np.int32))
    out = {}
    for name in ("device", "host"):
        ts = []
        for rep in range(8):
            ctx.sync()
            t0 = time.perf_counter()
            if name == "device":
                for k in range(draws):
                    rc = lib.tracker_draw_shuffles(tr.h, SEED, k)
                    assert rc == 0, rc
            else:
                for k in range(draws):
                    a, b = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
                    rc = lib.tracker_set_shuffle(tr.h, host._ptr(a), host._ptr(b))
                    assert rc == 0, rc
            ctx.sync()
            if rep:
                ts.append((time.perf_counter() - t0) / draws * 1e6)
        out[name] = {"us_per_call": round(statistics.median(ts), 2), "us_per_call_min_max": [round(min(ts), 2), round(max(ts), 2)]}
    tr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--paths", nargs="+", default=["recover", "composed", "report", "chain"])
    ap.add_argument("--big", type=int, default=50000)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--tile", type=int, default=1, help="the sequence's map this many times over (41: 51 004 points)")
    a = ap.parse_args()
    lib, full = load_any()
    if not full:
        a.paths = [p for p in a.paths if p in ("recover", "composed")]
    frames, poses, kim, kpose = synth.make_tracking_frames(N_FRAMES, period=N_FRAMES)
    cams = [Cam(lib, kim, kpose, a.tile) for _ in range(max(a.nb))]
    d_frames = [host.DevBuf(cams[0].ctx, f) for f in frames]       # (device memory: every context of the device reads it)
    raw = lambda h: h.value if hasattr(h, "value") else int(h)
    fp = [raw(d.p) for d in d_frames]
    p_opts = host._ptr(cams[0].tr.opts())
    out = {"library_has_the_chain": full, "passes": a.passes, "frames_per_pass": N_FRAMES, "points": cams[0].n, "nb": {}, "draw": {}}
    rng = np.random.default_rng(1)

    for nb in a.nb:
        cs = cams[:nb]
        stride = max(1, N_FRAMES // nb)
        first = [(i * stride) % N_FRAMES for i in range(nb)]
        arr = lambda xs: (C.c_void_p * len(xs))(*xs)
        trs, kfs, ests = arr([raw(c.tr.h) for c in cs]), arr([raw(c.kf.h) for c in cs]), arr([raw(c.est.h) for c in cs])
        reps = arr([raw(c.report.h) for c in cs])
        seeds = (C.c_uint64 * nb)(*[SEED + i for i in range(nb)])
        tags = (C.c_int64 * nb)()
        res = np.zeros(nb, host.TRACKMAP_RESULT_DT)
        p_res = host._ptr(res)
        states = (_abi.TrackState * nb)()
        infos = (_abi.TrackFrameStateInfo * nb)()
        dis = [arr([fp[(first[i] + s) % N_FRAMES] for i in range(nb)]) for s in range(N_FRAMES)]
        records = {p: 0 for p in a.paths}

        def reset():
            for i, c in enumerate(cs):
                start = np.ascontiguousarray(poses[(first[i] - 1) % N_FRAMES])       # (closed trajectory: the pose of the frame before the first)
                lib.track_state_reset(C.byref(states[i]), host._pd(start))
                lib.rotation_estimator_reset(c.est.h)
                c.tr.set_shuffle(c.map["shuffle_levels"], c.map["shuffle_fine"])
                if c.n > 8192:
                    c.ctx.sync()       # (see composed)

        def recover(s):
            rc = lib.track_frames_recover_batch(nb, trs, kfs, dis[s], states, ests, None, None, p_opts, None, p_res, infos)
            assert rc == 0, rc

        def composed(s):
            for c in cs:
                pa, pb = rng.permutation(c.n).astype(np.int32), rng.permutation(c.n).astype(np.int32)
                rc = lib.tracker_set_shuffle(c.tr.h, host._ptr(pa), host._ptr(pb))
                assert rc == 0, rc
                if c.n > 8192:
                    # beyond 8192 points set_shuffle stages the orders in the context's pinned block and copies them up
                    # asynchronously; a batch call fills its arguments into the same block: the copy must be done first
                    c.ctx.sync()
            recover(s)
            rc = lib.tracker_report_frames(nb, trs, reps, tags)
            assert rc == 0, rc

        def chain(s, with_seeds):
            rc = lib.track_frames_report_batch(nb, trs, kfs, dis[s], states, ests, None, None, p_opts, None, p_res, infos, reps, tags,
                                               seeds if with_seeds else None, None)
            assert rc == 0, rc

        steps = {"recover": recover, "composed": composed, "report": lambda s: chain(s, False), "chain": lambda s: chain(s, True)}
        times = {p: [] for p in a.paths}
        for rep in range(a.passes + 1):
            for p in a.paths:
                reset()
                t0 = time.perf_counter()
                for s in range(N_FRAMES):
                    steps[p](s)
                dt = time.perf_counter() - t0
                if rep:
                    times[p].append(dt)
                    records[p] = cs[0].report.info()["n_records"] if p != "recover" else int(res[0]["n_meas"])
        per = lambda t: round(t / (nb * N_FRAMES) * 1e6, 2)
        row = {p: {"us_per_frame": per(statistics.median(times[p])), "us_per_frame_min_max": [per(min(times[p])), per(max(times[p]))],
                   "last_records": records[p]} for p in a.paths}
        out["nb"][str(nb)] = row
        print("nb", nb, json.dumps(row), file=sys.stderr, flush=True)
    if full and a.draws > 0:
        for n in (cams[0].n, a.big):
            out["draw"][str(n)] = time_draws(lib, cams[0].ctx, cams[0].kf0, n, a.draws)
            print("draw", n, json.dumps(out["draw"][str(n)]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
