"""Times the map's hand-over from a resident map to a tracker on the device — ptam_rmap_publish into a ptam_map_snapshot and
ptam_tracker_take_map — beside the composed hand-over through the host that it replaces, in one process, on two maps:

    scene   the map of tests/test_gpu_insert_keyframe.py: three keyframes, the points made between two of them at threshold 400
    big     the same views and points inside --kf keyframes x --points points x --rows rows (time_insert_keyframe.big_map)

    python tools/mapmaker/time_publish.py [--reps 15] [--kf 200 --points 50000 --rows 800000] [--bad 0.005] [--cases scene,big]

One repetition: the map is uploaded with --bad of its points marked bad, published, and handed to both trackers (tracker A by
take_map, tracker B by ptam_tracker_set_map), all outside the clock.  Inside it,

    device    ptam_rmap_handle_bad_points (no lists down), ptam_rmap_publish, ptam_tracker_take_map
    composed  ptam_rmap_handle_bad_points with `kept` down, ptam_rmap_download of the point rows, the host's marshalling of the
              rows and sources (numpy, vectorised: the ptam_pvs_point rows packed, src_kf turned into keyframe handles),
              ptam_tracker_update_map with prev_index = kept (its per-point loop over the sources, its uploads)

and `publish` and `take` alone.  Method of time_resident_map.py: host clock around the synchronous calls through ctypes with every
buffer allocated beforehand, median of --reps after two warm-up runs.  Bytes over the host link: ptam_rmap_traffic's deltas, the
take's link_bytes, and for ptam_tracker_update_map what it uploads (72 + 24 + 4 bytes a point)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import insert_keyframe_ref as I  # noqa: E402
from time_insert_keyframe import UPLOAD_KEYS, big_map  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    ap.add_argument("--bad", type=float, default=0.005)
    ap.add_argument("--cases", default="scene,big")
    a = ap.parse_args()

    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    lib, mm = ctx.lib, host.MapMaker(ctx)
    kfs, ka, poses, sp = I.make_keyframes(ctx)
    m0 = host.ResidentMap(ctx)
    m0.upload(kfs=kfs, **{k: v for k, v in I.empty_tables(poses).items() if k in UPLOAD_KEYS})
    made0, _ = mm.AddSomeMapPoints(kfs[I.THIRD], poses[I.THIRD], kfs[I.TARGET], poses[I.TARGET], mm.opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH))
    m0.add_points(I.THIRD, I.TARGET, made0)
    scene = m0.tables()
    m0.close()
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def ok(rc):
        assert rc == 0, (rc, lib.last_error())

    for case in a.cases.split(","):
        h, hk = (scene, kfs) if case == "scene" else big_map(scene, kfs, a.kf, a.points, a.rows)
        h = {k: np.array(v) for k, v in h.items()}
        K, N = len(h["poses"]), len(h["points3"])
        bad = (np.random.default_rng(1).random(N) < a.bad).astype(np.uint8)
        bad[0] = 1
        h["bad"], h["points"]["bad"] = bad, bad
        handles = np.array([k.h.value if hasattr(k.h, "value") else int(k.h) for k in hk], np.uint64)
        m, snap = host.ResidentMap(ctx), host.MapSnapshot(ctx, 2 * N)
        m.reserve(n_kf=2 * K, n_points=2 * N, n_meas=2 * len(h["meas"]), n_never=2 * len(h["never"]) + 1)
        ta, tb = host.Tracker(ctx, 2 * N), host.Tracker(ctx, 2 * N)
        # everything the timed calls write, allocated beforehand
        pub, took, hb = _abi.MapPublishResult(), _abi.MapTakeResult(), _abi.MapBadPointsResult()
        kept, rows = np.zeros(N, np.int32), np.zeros(N, host.MAP_REFIND_POINT_DT)
        pvs, q = np.zeros(N, host.PVS_POINT_DT), np.zeros(N, host.TEMPLATE_QUERY_DT)
        seen = {}

        def marshal(n):
            """the rows as ptam_tracker_set_map / update_map take them"""
            r = rows[:n]
            pvs[:n] = r["pv"]
            q["src_kf"][:n], q["src_level"][:n] = handles[r["src_kf"]], r["src_level"]
            q["center_x"][:n], q["center_y"][:n] = r["center_x"], r["center_y"]

        def prep():
            m.upload(kfs=hk, **{k: h[k] for k in UPLOAD_KEYS})
            ok(lib.rmap_publish(m.h, snap.h, C.byref(pub)))
            ok(lib.tracker_take_map(ta.h, snap.h, C.byref(took)))
            ok(lib.rmap_download(m.h, _abi.RMAP_REFIND_POINTS, 0, N, p(rows)))
            marshal(N)
            ok(lib.tracker_set_map(tb.h, N, p(pvs), p(q)))

        def device():
            ok(lib.rmap_handle_bad_points(m.h, C.byref(hb), None, None))
            ok(lib.rmap_publish(m.h, snap.h, C.byref(pub)))
            ok(lib.tracker_take_map(ta.h, snap.h, C.byref(took)))
            seen["device"] = (hb.n_kept, took.n_carried, took.link_bytes)

        def composed():
            ok(lib.rmap_handle_bad_points(m.h, C.byref(hb), p(kept), None))
            n = hb.n_kept
            ok(lib.rmap_download(m.h, _abi.RMAP_REFIND_POINTS, 0, n, p(rows)))
            marshal(n)
            ok(lib.tracker_update_map(tb.h, n, p(pvs), p(q), p(kept)))
            seen["composed"] = n

        def prep_edited():
            prep()
            ok(lib.rmap_handle_bad_points(m.h, C.byref(hb), None, None))

        def prep_published():
            prep_edited()
            ok(lib.rmap_publish(m.h, snap.h, C.byref(pub)))

        line = {}
        for name, fn, pr in (("device", device, prep), ("composed", composed, prep), ("publish", lambda: ok(lib.rmap_publish(m.h, snap.h, C.byref(pub))), prep_edited),
                             ("take", lambda: ok(lib.tracker_take_map(ta.h, snap.h, C.byref(took))), prep_published)):
            pr()
            before = m.traffic()
            fn()
            moved = [x - y for x, y in zip(m.traffic(), before)]
            if name in ("device", "take"):
                moved[1] += took.link_bytes
            if name == "composed":
                moved[0] += seen["composed"] * (72 + 24 + 4)
            line[name] = (median_ms(fn, a.reps, pr), moved)
        n_kept, n_carried, _ = seen["device"]
        assert n_kept == n_carried == seen["composed"] == N - int(bad.sum()), (seen, N, int(bad.sum()))
        assert np.array_equal(ta.point_serials(0, took.n_points), m.point_serials())
        print(f"{case:6s} K={K} N={N}: {int(bad.sum())} points removed, {n_carried} carried")
        for name, (ms, moved) in line.items():
            print(f"    {name:9s} {ms:8.3f} ms | over the host link: up {moved[0]} B, down {moved[1]} B", flush=True)
        for x in (ta, tb, snap, m):
            x.close()
    ctx.close()


if __name__ == "__main__":
    main()
