"""Times the map-table edits ptam_map_apply_outliers / ptam_map_handle_bad_points / ptam_map_add_points at 200 keyframes x 50 000
points x 800 000 rows with 1 % of the points bad, 0.5 % of the rows outliers and 2 000 new points, against two things measured in
the same run: the vectorised numpy restatement (tests/map_edit_ref.py) and a plain C++ host loop over std::map / std::set
containers shaped like the reference's (tools/mapmaker/map_edit_host.cc, g++ -O2, one thread).

    python tools/mapmaker/time_map_edit.py [--reps 15] [--only device|host] [--kf 200 --points 50000 --rows 800000]

Per entry: the whole call (host clock around the synchronous C call, its output buffers allocated beforehand, median of --reps
after two warm-up calls) and the copies alone — the same bytes up and down through ptam_dev_upload / ptam_dev_download, no
kernel between them.  The difference is the
call's host-side checks of the tables plus its kernels; the kernels alone come from a kernel trace of the same command with
--only device (rocprofv3 --kernel-trace --stats: the mt_* kernels), see docs/LOG_mapmaker.md.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import map_edit_ref as E  # noqa: E402


def median_ms(fn, reps, prep=None):
    t = []
    for r in range(reps + 2):
        if prep is not None:
            prep()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= 2:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t))


def copies(ctx, up, down):
    """the bytes of `up` to the device and the bytes of `down` back, one transfer per table"""
    bufs = [(host.DevBuf(ctx, max(a.nbytes, 8)), a) for a in up]
    outs = [(host.DevBuf(ctx, max(a.nbytes, 8)), a) for a in down]

    def run():
        for b, a in bufs:
            if a.nbytes:
                b.upload(a)
        for b, a in outs:
            if a.nbytes:
                ctx._check(ctx.lib.dev_download(ctx.h, a.ctypes.data, b.p, a.nbytes), "dev_download")
    return run, lambda: [b.free() for b, _ in bufs + outs]


def raw_calls(ctx, K, N, t, a, b, outliers, made, points3, src_kf, target_kf):
    """the three entries through ctypes with every output buffer allocated beforehand -> name: (prepare, call)"""
    import ctypes as C
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    meas, never, failure, nq = t["meas"], t["never"], t["failure"], t["new_queue"]
    M, V, F, O, A = len(meas), len(never), len(failure), len(outliers), len(made)
    mo, no, fo = np.zeros(M + 2 * A, E.MEAS_DT), np.zeros(V + O, E.PAIR_DT), np.zeros(F + O, E.PAIR_DT)
    ni, kept, qo = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(len(nq), np.int32)
    pts, src = np.zeros(A, E.POINT_DT), np.zeros(A, E.SOURCE_DT)
    bad, col = t["bad"].copy(), points3.copy()
    ro, rb = _abi.MapOutliersResult(), _abi.MapBadPointsResult()
    ctab, _ = host.map_columns([col])

    def check(rc):
        assert rc == 0, (rc, ctx.lib.last_error())

    def reset():
        bad[:] = t["bad"]
        col[:] = points3
    return {
        "apply_outliers": (reset, lambda: check(ctx.lib.map_apply_outliers(ctx.h, K, N, M, p(meas), V, p(never), F, p(failure), O, p(outliers),
                                                                            p(bad), C.byref(ro), p(mo), p(no), p(fo)))),
        "handle_bad_points": (reset, lambda: check(ctx.lib.map_handle_bad_points(
            ctx.h, K, N, p(a["bad"]), p(t["outlier_count"]), p(t["inlier_count"]), len(a["meas"]), p(a["meas"]), len(a["never"]), p(a["never"]),
            len(nq), p(nq), len(a["failure"]), p(a["failure"]), 1, C.cast(ctab, C.c_void_p), C.byref(rb), p(ni), p(kept), p(mo), p(no), p(qo),
            p(fo)))),
        "add_points": (None, lambda: check(ctx.lib.map_add_points(ctx.h, K, b["n_kept"], len(b["meas"]), p(b["meas"]), src_kf, target_kf,
                                                                  _abi.SRC_EPIPOLAR, A, p(made), p(mo), p(pts), p(src)))),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", choices=["device", "host"])
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    ap.add_argument("--made", type=int, default=2000)
    a = ap.parse_args()
    K, N = a.kf, a.points
    t = E.make_tables(7, K, N, a.rows, bad_share=0.005, count_share=0.005, lonely=0)
    meas, never, failure, nq = t["meas"], t["never"], t["failure"], t["new_queue"]
    outliers = E.make_outliers(8, K, N, meas, len(meas) // 200)
    made, points3 = E.make_made(9, a.made), E.point_columns(9, N)[0]
    src_kf, target_kf = K - 1, K - 2
    print(f"K={K} N={N} rows={len(meas)} never={len(never)} new queue={len(nq)} failure queue={len(failure)} outliers={len(outliers)} "
          f"made={len(made)}")

    ref_a = E.np_apply_outliers(K, t["bad"], meas, never, failure, outliers)
    ref_b = E.np_handle_bad_points(K, N, ref_a["meas"], ref_a["never"], ref_a["bad"], t["outlier_count"], t["inlier_count"], nq,
                                   ref_a["failure"], [points3])
    ref_c = E.np_add_points(K, ref_b["n_kept"], ref_b["meas"], src_kf, target_kf, made)
    print(f"removed {ref_b['n_removed']} points ({ref_b['n_marked']} by the counts), rows {len(meas)} -> {len(ref_a['meas'])} -> "
          f"{len(ref_b['meas'])} -> {len(ref_c['meas'])}")
    calls = {
        "apply_outliers": (lambda: E.np_apply_outliers(K, t["bad"], meas, never, failure, outliers),
                           lambda c: host.map_apply_outliers(c, K, t["bad"], meas, never, failure, outliers),
                           [meas, never, outliers, t["bad"]], [ref_a["meas"], ref_a["never"], ref_a["failure"][len(failure):], ref_a["bad"]]),
        "handle_bad_points": (lambda: E.np_handle_bad_points(K, N, ref_a["meas"], ref_a["never"], ref_a["bad"], t["outlier_count"],
                                                             t["inlier_count"], nq, ref_a["failure"], [points3]),
                              lambda c: host.map_handle_bad_points(c, K, N, ref_a["meas"], ref_a["never"], bad=ref_a["bad"],
                                                                   outlier_count=t["outlier_count"], inlier_count=t["inlier_count"],
                                                                   new_queue=nq, failure=ref_a["failure"], columns=[points3]),
                              [ref_a["meas"], ref_a["never"], ref_a["bad"], t["outlier_count"], t["inlier_count"], nq, ref_a["failure"], points3],
                              [ref_b["meas"], ref_b["never"], ref_b["new_index"], ref_b["kept"], ref_b["new_queue"], ref_b["failure"],
                               points3[:ref_b["n_kept"]]]),
        "add_points": (lambda: E.np_add_points(K, ref_b["n_kept"], ref_b["meas"], src_kf, target_kf, made),
                       lambda c: host.map_add_points(c, K, ref_b["n_kept"], ref_b["meas"], src_kf, target_kf, made),
                       [ref_b["meas"], made], [ref_c["meas"], ref_c["points"], ref_c["sources"]]),
    }
    refs = {"apply_outliers": (ref_a, ("bad", "meas", "never", "failure")), "handle_bad_points": (ref_b, ("new_index", "kept", "meas", "never",
                                                                                                         "new_queue", "failure")),
            "add_points": (ref_c, ("meas", "points", "sources"))}
    ctx = None
    if a.only != "host":
        from ptam_cg_amd._lib import load
        ctx = host.Context(lib=load())
        raws = raw_calls(ctx, K, N, t, ref_a, ref_b, outliers, made, points3, src_kf, target_kf)
    hostms = {}
    if a.only != "device":
        tmp = tempfile.mkdtemp()
        exe = os.path.join(tmp, "map_edit_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "mapmaker", "map_edit_host.cc"), "-o", exe])
        path = os.path.join(tmp, "tables.bin")
        with open(path, "wb") as f:
            f.write(np.array([K, N, len(meas), len(never), len(nq), len(failure), len(outliers), len(made), src_kf, target_kf,
                              _abi.SRC_EPIPOLAR, 0], np.int32).tobytes())
            for x in (t["bad"], t["outlier_count"], t["inlier_count"], meas, never, nq, failure, outliers, made):
                f.write(np.ascontiguousarray(x).tobytes())
        h = subprocess.check_output([exe, path, str(max(a.reps // 3, 3))], text=True).split()
        hostms = dict(zip(calls, map(float, h[1:4])))
        assert int(h[4]) == ref_b["n_removed"] and int(h[5]) == len(ref_c["meas"]), h
    for name, (np_fn, dev_fn, up, down) in calls.items():
        line = f"{name:18s}"
        if ctx is not None:
            got = dev_fn(ctx)
            E.assert_same(got, refs[name][0], (), refs[name][1])
            prep, raw = raws[name]
            call = median_ms(raw, a.reps, prep)
            run, free = copies(ctx, [np.ascontiguousarray(x) for x in up], [np.ascontiguousarray(x).copy() for x in down])
            cp = median_ms(run, a.reps)
            free()
            mb = (sum(x.nbytes for x in up) + sum(x.nbytes for x in down)) / 1e6
            line += f" device call {call:8.3f} ms | copies alone {cp:8.3f} ms ({mb:.1f} MB, {100 * cp / call:.0f} %) | rest {call - cp:8.3f} ms"
        if a.only != "device":
            line += f" | numpy {median_ms(np_fn, max(a.reps // 3, 3)):8.3f} ms | C++ std::map loop {hostms[name]:8.3f} ms"
        print(line, flush=True)
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
