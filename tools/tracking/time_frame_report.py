"""Times a tracked frame's way from the tracker into the resident map — ptam_tracker_report_frames, ptam_rmap_note_reports,
ptam_rmap_insert_keyframe_report — beside the composed host path it replaces, in one process on one card:

    python tools/tracking/time_frame_report.py [--frames 64] [--reps 15] [--kf 200 --points 50000 --rows 800000] [--cases scene,big]

    scene   the map of tests/test_gpu_insert_keyframe.py (three keyframes, about 600 points), published and taken by a tracker, which
            then tracks --frames frames of the new keyframe's view, each with shuffles of its own.  After every frame, inside the clock,
                report    ptam_tracker_report_frames (1 camera) + ptam_rmap_note_reports (1 report)
                composed  ptam_tracker_read_iteration_set + ptam_tracker_read_iteration_serials + ptam_rmap_resolve_serials + the
                          host's filter of the found and the live entries (numpy) + ptam_rmap_note_tracked
            both on the same map one after the other (the counts only grow).  Median over the frames after two warm-up frames.
            The keyframe hand-over, --reps repetitions, the map uploaded, published, taken and a frame tracked again before each:
                report    ptam_tracker_report_frames + ptam_rmap_insert_keyframe_report
                composed  read_iteration_set + read_iteration_serials + resolve_serials + filter + sort by point (numpy) +
                          ptam_rmap_insert_keyframe
    big     the same views and points inside --kf keyframes x --points points x --rows rows (time_insert_keyframe.big_map).  The
            tracker keeps the scene's map (the points in view); the report is made by ptam_frame_report_from_host from the scene
            frame's iteration set with the big map's serials, outside the clock, so this case times the consumers alone:
                report    ptam_rmap_note_reports | ptam_rmap_insert_keyframe_report
                composed  resolve_serials + filter + note_tracked | resolve_serials + filter + sort + ptam_rmap_insert_keyframe

Host clock around the synchronous calls through ctypes with every buffer allocated beforehand.  Bytes over the host link are
ptam_rmap_traffic's deltas (the tracker-side calls are not in them: the report moves 144 + 16 bytes per camera, the two reads of
the composed path 136 bytes of control block twice and 76 + 8 bytes per entry).  Prints one line per case and one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "mapmaker"))

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import insert_keyframe_ref as I  # noqa: E402
from time_insert_keyframe import UPLOAD_KEYS, big_map  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    ap.add_argument("--cases", default="scene,big")
    a = ap.parse_args()

    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    lib, mm = ctx.lib, host.MapMaker(ctx)
    kfs, ka, poses, sp = I.make_keyframes(ctx)
    m0 = host.ResidentMap(ctx)
    m0.upload(kfs=kfs, **{k: v for k, v in I.empty_tables(poses).items() if k in UPLOAD_KEYS})
    made0, _ = mm.AddSomeMapPoints(kfs[I.THIRD], poses[I.THIRD], kfs[I.TARGET], poses[I.TARGET],
                                   mm.opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH))
    m0.add_points(I.THIRD, I.TARGET, made0)
    scene = m0.tables()
    m0.close()
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    sp12 = np.ascontiguousarray(sp, np.float64).reshape(12)

    def ok(rc):
        assert rc == 0, (rc, lib.last_error())

    # everything the timed calls write, allocated beforehand
    cap = 8192
    it, ser, idx = np.zeros(cap, host.TRACKMAP_MEAS_DT), np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    n_it, n_ser, gone = C.c_int(), C.c_int(), C.c_int32()
    note, ins = _abi.RmapNoteResult(), _abi.RmapInsertResult()
    n_rows, n_gone = C.c_int32(), C.c_int32()
    res = np.zeros(1, host.TRACKMAP_RESULT_DT)
    out = {}

    for case in a.cases.split(","):
        h, hk = (scene, kfs) if case == "scene" else big_map(scene, kfs, a.kf, a.points, a.rows)
        h = {k: np.array(v) for k, v in h.items()}
        K, N = len(h["poses"]), len(h["points3"])
        m, rf = host.ResidentMap(ctx), host.ReFinder(ctx)
        m.reserve(n_kf=2 * K, n_points=2 * N, n_meas=2 * len(h["meas"]), n_never=2 * len(h["never"]) + N)
        ms, snap, tr = host.ResidentMap(ctx), host.MapSnapshot(ctx, cap), host.Tracker(ctx, cap)      # the tracker's map: the scene
        rep = host.FrameReport(ctx, cap)
        reps_h = (C.c_void_p * 1)(rep.h)
        trs_h = (C.c_void_p * 1)(tr.h)
        tag = (C.c_int64 * 1)(0)
        opts = m.insert_opts(levels=I.KEYFRAME_ORDER, min_shi_tomasi=I.THRESHOLD, **I.DEPTH)
        frame_no = [0]

        def upload_and_take():
            """the map uploaded; the tracker holds its points in view with their serials"""
            m.upload(kfs=hk, **{k: h[k] for k in UPLOAD_KEYS})
            src = m if case == "scene" else ms
            if case != "scene":
                ms.upload(kfs=kfs, **{k: scene[k] for k in UPLOAD_KEYS})
            src.publish(snap)
            tr.take_map(snap)

        def track():
            rng = np.random.default_rng(100 + frame_no[0])
            frame_no[0] += 1
            tr.set_shuffle(rng.permutation(tr.n).astype(np.int32), rng.permutation(tr.n).astype(np.int32))
            ok(lib.track_map(tr.h, ka.h, host._pd(sp12), None, p(res)))

        def fill_report():
            ok(lib.tracker_report_frames(1, trs_h, reps_h, tag))

        def read_set():
            """the tracker side of the composed path -> (serials of the found entries, the found entries)"""
            if case == "scene":
                ok(lib.tracker_read_iteration_set(tr.h, p(it), cap, C.byref(n_it)))
                ok(lib.tracker_read_iteration_serials(tr.h, p(ser), cap, C.byref(n_ser)))
                e, s = it[:n_it.value], ser[:n_ser.value]
            else:
                e, s = held[0], held[1]
            f = e["found"] != 0
            return s[f], e[f]

        def resolve(s):
            ok(lib.rmap_resolve_serials(m.h, len(s), p(s), p(idx), C.byref(gone)))
            return idx[:len(s)]

        def note_report():
            fill_report() if case == "scene" else None
            ok(lib.rmap_note_reports(m.h, 1, reps_h, C.byref(note)))

        def note_composed():
            s, e = read_set()
            at = resolve(np.ascontiguousarray(s))
            live = at >= 0
            pts, fl = np.ascontiguousarray(at[live]), np.ascontiguousarray((e["outlier"][live] != 0).astype(np.uint8))
            ok(lib.rmap_note_tracked(m.h, len(pts), p(pts), p(fl)))

        def insert_report():
            fill_report() if case == "scene" else None
            ok(lib.rmap_insert_keyframe_report(m.h, rf.h, ka.h, host._pd(sp12), 0, rep.h, C.byref(opts), C.byref(ins), C.byref(n_rows), C.byref(n_gone)))

        def insert_composed():
            s, e = read_set()
            at = resolve(np.ascontiguousarray(s))
            live = at >= 0
            rows = np.zeros(int(live.sum()), host.MAP_KF_ROW_DT)
            rows["point"], rows["level"], rows["root_pos"] = at[live], e["level"][live], e["v2_found"][live]
            rows = rows[np.argsort(rows["point"], kind="stable")]
            ok(lib.rmap_insert_keyframe(m.h, rf.h, ka.h, host._pd(sp12), 0, len(rows), p(rows), C.byref(opts), C.byref(ins)))
            n_rows.value = len(rows)

        def clock(fn):
            before = m.traffic()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            return (t1 - t0) * 1e3, [x - y for x, y in zip(m.traffic(), before)]

        held = [None, None]

        def after_upload():
            """big: the report and the host's lists of the scene frame, named by the big map's serials (outside the clock)"""
            if case == "scene":
                return
            e = tr.iteration_set()
            col = m.point_serials()
            m.publish(snap_big)                                          # (the map_id, as a tracker would learn it)
            rep.from_host(snap_big.info()["map_id"], col, e)
            held[0], held[1] = e, col[e["point"]]

        snap_big = host.MapSnapshot(ctx, 2 * N) if case != "scene" else None
        line = {}
        # ---- per tracked frame
        upload_and_take()
        t_rep, t_com = [], []
        for f in range(a.frames + 2):
            track()
            if f == 0:
                after_upload()
            ms_r, mv_r = clock(note_report)
            ms_c, mv_c = clock(note_composed)
            if f >= 2:
                t_rep.append(ms_r)
                t_com.append(ms_c)
        line["frame"] = dict(report_ms=float(np.median(t_rep)), composed_ms=float(np.median(t_com)), report_link=mv_r, composed_link=mv_c,
                             records=note.n_records, gone=note.n_gone)
        # ---- the keyframe hand-over
        for name, fn in (("report", insert_report), ("composed", insert_composed)):
            t = []
            for r in range(a.reps + 2):
                upload_and_take()
                track()
                after_upload()
                dt, mv = clock(fn)
                if r >= 2:
                    t.append(dt)
            line.setdefault("keyframe", {}).update({name + "_ms": float(np.median(t)), name + "_link": mv, name + "_rows": n_rows.value,
                                                    name + "_made": ins.n_made})
        k = line["keyframe"]
        assert k["report_rows"] == k["composed_rows"] and k["report_made"] == k["composed_made"], k
        out[case] = dict(K=K, N=N, tracker_points=tr.n, **line)
        fr = line["frame"]
        print(f"{case:6s} K={K} N={N}, tracker {tr.n} points, {fr['records']} records")
        print(f"    per frame   report {fr['report_ms']:7.3f} ms (link up/down {fr['report_link']}) | composed {fr['composed_ms']:7.3f} ms ({fr['composed_link']})")
        print(f"    keyframe    report {k['report_ms']:7.3f} ms (link {k['report_link']}) | composed {k['composed_ms']:7.3f} ms ({k['composed_link']}); "
              f"{k['report_rows']} rows, {k['report_made']} points made", flush=True)
        for x in (rep, tr, snap, ms, rf, m) + ((snap_big,) if snap_big else ()):
            x.close()
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
