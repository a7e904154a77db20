"""Times ptam_rmap_insert_keyframe (host.ResidentMap.InsertKeyFrame) beside the sequence of resident calls it replaces — add_keyframe,
refind(KEYFRAME), the download of the keyframe's run as the busy list, the closest keyframe from the downloaded poses,
MapMaker.AddSomeMapPoints, add_points — in one process, on two maps:

    scene   the map of tests/test_gpu_insert_keyframe.py: three keyframes, the points made between two of them at threshold 400
    big     the same views and points inside a map of --kf keyframes x --points points x --rows rows (tests/map_edit_ref.make_tables):
            the scene's point rows repeated up to --points (the repeats moved 100 units aside, out of every view), the target and
            the third view at keyframes 1 and 2, every other keyframe far away

    python tools/mapmaker/time_insert_keyframe.py [--reps 15] [--kf 200 --points 50000 --rows 800000] [--threshold 400] [--cases scene,big]

Method of time_resident_map.py: host clock around the synchronous calls, median of --reps after two warm-up runs; a call changes
the map it runs on, so the map is uploaded again before every repetition, outside the clock.  Both paths go through the host.*
wrappers.  The traffic columns are ptam_rmap_traffic's deltas of one run; the composed path's also counts what
ptam_add_map_points_epipolar copies outside the handle: the busy list up, its header and its record buffer (one
ptam_new_map_point of room per maximal corner of the visited levels) down."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import insert_keyframe_ref as I  # noqa: E402
from tests import map_edit_ref as E  # noqa: E402

UPLOAD_KEYS = ("poses", "fixed", "points3", "points", "sources", "bad", "meas", "never", "new_queue", "failure", "outlier_count", "inlier_count")


def median_ms(fn, reps, prep):
    t = []
    for r in range(reps + 2):
        prep()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= 2:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t))


def big_map(h, kfs, K, N, rows_total, seed=7):
    """the scene's tables inside a map of K keyframes, N points and rows_total measurement rows"""
    t = E.make_tables(seed, K, N, rows_total, bad_share=0.0, count_share=0.0, lonely=0)
    rng = np.random.default_rng(seed)
    n0 = len(h["points3"])
    take = np.arange(N) % n0
    poses = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (K, 1))
    poses[:, 9:] = rng.uniform(-0.2, 0.2, (K, 3))                                  # centres near the origin: far from the new keyframe
    poses[:3] = h["poses"]
    points3, points = h["points3"][take], h["points"][take]
    points3[n0:, 0] += 100.0                                                        # the repeated points lie outside every view, as most
    points["pv"]["world"] = points3                                                 # of a large map's points do for one keyframe
    out = dict(poses=poses, fixed=(np.arange(K) == 0).astype(np.uint8), points3=points3, points=points, sources=h["sources"][take],
               bad=np.zeros(N, np.uint8), outlier_count=np.zeros(N, np.int32), inlier_count=np.zeros(N, np.int32), meas=t["meas"], never=t["never"],
               new_queue=np.zeros(0, np.int32), failure=np.zeros(0, host.MAP_PAIR_DT))
    return out, list(kfs) + [kfs[I.DECOY]] * (K - 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    ap.add_argument("--threshold", type=float, default=I.THRESHOLD)
    ap.add_argument("--cases", default="scene,big")
    a = ap.parse_args()

    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    mm = host.MapMaker(ctx)
    kfs, ka, poses, sp = I.make_keyframes(ctx)
    eo = mm.opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=a.threshold, **I.DEPTH)
    m0 = host.ResidentMap(ctx)
    m0.upload(kfs=kfs, **{k: v for k, v in I.empty_tables(poses).items() if k in UPLOAD_KEYS})
    made0, _ = mm.AddSomeMapPoints(kfs[I.THIRD], poses[I.THIRD], kfs[I.TARGET], poses[I.TARGET], mm.opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH))
    m0.add_points(I.THIRD, I.TARGET, made0)
    scene = m0.tables()
    m0.close()
    rows = I.tracker_rows(scene, sp)
    cand_cap = sum(len(I.M.read_rest(ctx, ka, l)[0]) for l in I.KEYFRAME_ORDER)

    for case in a.cases.split(","):
        h, hk = (scene, kfs) if case == "scene" else big_map(scene, kfs, a.kf, a.points, a.rows)
        K, N, M = len(h["poses"]), len(h["points3"]), len(h["meas"])
        m, rf = host.ResidentMap(ctx), host.ReFinder(ctx)
        m.reserve(n_kf=2 * K, n_points=2 * N + cand_cap, n_meas=2 * M + 2 * N + 2 * cand_cap, n_never=2 * len(h["never"]) + 2 * N, n_new=2 * cand_cap)
        opts = m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=a.threshold, **I.DEPTH)
        out = {}

        def prep():
            m.upload(kfs=hk, **{k: h[k] for k in UPLOAD_KEYS})

        def one_call():
            out["one"] = m.InsertKeyFrame(rf, ka, sp, 0, rows, opts)

        def composed():
            m.add_keyframe(sp, 0, rows, kf=ka)
            r = m.refind(rf, _abi.MAP_REFIND_KEYFRAME, np.array([K], np.int32), lists=False)
            run = m.download("meas", M)                                            # the new keyframe's run: the table's tail
            p = m.download("poses")
            t = int(I.closest_keyframes_np(p, K, 1)[0][0])
            made, stats = mm.AddSomeMapPoints(ka, sp, hk[t], p[t], eo, busy_level=run["level"], busy_root=run["root_pos"], cap=cand_cap)
            m.add_points(K, t, made)
            out["composed"] = dict(target_kf=t, n_made=len(made), n_found=r["n_found"], candidates=int(stats["candidates"].sum()), n_busy=len(run))

        line = {}
        for name, fn in (("one call", one_call), ("composed", composed)):
            prep()
            before = m.traffic()
            fn()
            moved = [x - y for x, y in zip(m.traffic(), before)]
            if name == "composed":   # ptam_add_map_points_epipolar's own copies: the busy list up, the header and the record buffer down
                moved[0] += 4 + 24 * out["composed"]["n_busy"]
                moved[1] += 16 + 4 * host.EPIPOLAR_STATS_DT.itemsize + cand_cap * host.NEW_MAP_POINT_DT.itemsize
            line[name] = (median_ms(fn, a.reps, prep), moved)
        one, comp = out["one"], out["composed"]
        assert (one["target_kf"], one["n_made"], one["refind"]["n_found"]) == (comp["target_kf"], comp["n_made"], comp["n_found"]), (one, comp)
        print(f"{case:6s} K={K} N={N} M={M} keyframe rows={len(rows)} threshold={a.threshold:g}: target {one['target_kf']}, re-found {one['refind']['n_found']}, "
              f"candidates {comp['candidates']}, made {one['n_made']}")
        for name, (ms, moved) in line.items():
            print(f"    {name:9s} {ms:8.3f} ms | traffic up {moved[0]} B, down {moved[1]} B", flush=True)
        rf.close()
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
