"""Times ptam_map_refind (MapMaker::ReFindNewlyMade / ReFindInSingleKeyFrame as one device call on the map tables) against the
path it replaces: the callers' loops with the reference's std::set tests filling one ptam_refind_pair per pair
(tools/mapmaker/map_refind_host.cc, g++ -O2, one thread), ptam_refind_pairs on that list, then the results folded back into the
sets and the sorted table rebuilt.

    python tools/mapmaker/time_map_refind.py [--reps 20] [--only device|composed] [--cases new200x2000,keyframe50000]
                                             [--pass-sizes 16384,65536]

new200x2000: 200 keyframe entries x 2 000 new points (400 000 pairs) on a map of 20 000 points, every old point measured by ~16
consecutive keyframes; keyframe50000: the newest of 200 keyframes against 50 000 points.  Per case one JSON line: medians (and
minima) of --reps after 3 warm-ups, host clock around synchronous calls, the tables made before the clock starts.  Per-kernel
times come from a run of `--only device` under rocprofv3 --kernel-trace --stats (docs/LOG_mapmaker.md)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import map_refind_ref as R  # noqa: E402

CASES = {   # name: (mode, keyframe entries, points in the map, work)
    "new200x2000": (_abi.MAP_REFIND_NEW_POINTS, 200, 20000, 2000),
    "keyframe50000": (_abi.MAP_REFIND_KEYFRAME, 200, 50000, 1),
}
WARMUP = 3


def build_host_lib(out_dir):
    so = os.path.join(out_dir, "libmap_refind_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "mapmaker", "map_refind_host.cc"), "-o", so])
    lib = C.CDLL(so)
    lib.mrh_create.restype = C.c_void_p
    lib.mrh_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.mrh_destroy.argtypes = [C.c_void_p]
    lib.mrh_pairs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.mrh_pair_data.restype = C.c_void_p
    lib.mrh_fold.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def make_map(ctx, mode, n_kf, n_points, n_work, seed=3):
    """the test scene's keyframes and points, the points repeated up to n_points; old points measured by 16 consecutive
    keyframes (a window that slides with the point index), the new points (the last n_work of the table, NEW_POINTS) by their
    source keyframe and one more, two never entries per hundred points"""
    scene = R.make_scene(ctx, n_kf=n_kf, meas_share=0.0, never_share=0.0)
    base = scene["points"]
    points = base[np.arange(n_points) % len(base)].copy()
    rng = np.random.default_rng(seed)
    n_new = n_work if mode == _abi.MAP_REFIND_NEW_POINTS else 0
    n_old = n_points - n_new
    first = (np.arange(n_old) * (n_kf - 16)) // max(n_old - 1, 1)
    kf = (first[:, None] + np.arange(16)[None, :]).reshape(-1)
    pt = np.repeat(np.arange(n_old), 16)
    kf = np.concatenate([kf, np.tile([1, n_kf - 1], n_new)])
    pt = np.concatenate([pt, np.repeat(np.arange(n_old, n_points), 2)])
    meas = np.zeros(len(kf), R.MEAS_DT)
    meas["kf"], meas["point"] = kf, pt
    meas["level"], meas["source"] = rng.integers(0, 4, len(kf)), rng.integers(0, 5, len(kf))
    meas["root_pos"] = rng.random((len(kf), 2)) * 600
    meas = R.sort_table(meas)
    nv = np.zeros(n_points // 50, R.PAIR_DT)
    nv["point"] = rng.choice(n_points, size=len(nv), replace=False)
    k_work = ((n_kf - 1) // 12) * 12                                     # (frame B at the scene's true pose)
    nv["kf"] = 0 if mode == _abi.MAP_REFIND_NEW_POINTS else k_work
    nv = R.sort_table(nv[~np.isin(nv["point"].astype(np.int64) + nv["kf"].astype(np.int64) * n_points,
                                  meas["point"].astype(np.int64) + meas["kf"].astype(np.int64) * n_points)])
    work = np.arange(n_old, n_points, dtype=np.int32) if n_new else np.array([k_work], np.int32)
    return scene, points, meas, nv, work


def stats(t):
    t = np.array(t[WARMUP:]) * 1e3
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3)}


def time_device(ctx, mode, scene, points, meas, never, work, reps, per_pass=0):
    handles = np.array([k.h.value for k in scene["kfs"]], np.uint64)
    p = host._ptr
    cap = host.map_refind_pair_count(mode, len(handles), len(points), len(work))
    found, subpix, nev = np.zeros(cap, R.MEAS_DT), np.zeros(cap, np.int32), np.zeros(cap, R.PAIR_DT)
    mm, nm = np.zeros(len(meas) + cap, R.MEAS_DT), np.zeros(len(never) + cap, R.PAIR_DT)
    res = _abi.MapRefindResult()
    opts = _abi.MapRefindOpts(int(per_pass), 0)
    rf = host.ReFinder(ctx)
    t = []
    for _ in range(reps + WARMUP):
        t0 = time.perf_counter()
        rc = ctx.lib.map_refind(ctx.h, rf.h, C.byref(opts), mode, len(handles), p(handles), p(scene["poses"]), len(points), p(points), len(meas),
                                p(meas), len(never), p(never), len(work), p(work), None, C.byref(res), p(found), p(subpix), p(nev), cap,
                                p(mm), p(nm))
        t.append(time.perf_counter() - t0)
        assert rc == 0, rc
    rf.close()
    r = {f: getattr(res, f) for f, _ in _abi.MapRefindResult._fields_}
    r["meas_merged"] = mm[:len(meas) + res.n_found]
    return stats(t), r


def time_composed(ctx, hl, mode, scene, points, meas, never, work, reps):
    handles = np.array([k.h.value for k in scene["kfs"]], np.uint64)
    p = host._ptr
    rf = host.ReFinder(ctx)
    tl, tc, tf = [], [], []
    table = np.zeros(len(meas) + host.map_refind_pair_count(mode, len(handles), len(points), len(work)), R.MEAS_DT)
    for _ in range(reps + WARMUP):
        m = hl.mrh_create(len(handles), p(handles), p(scene["poses"]), len(points), p(points), len(meas), p(meas), len(never), p(never))
        t0 = time.perf_counter()
        n = hl.mrh_pairs(m, mode, len(work), p(work))
        t1 = time.perf_counter()
        out, kept = np.zeros(n, host.REFIND_RESULT_DT), np.zeros(n, np.int32)
        t2 = time.perf_counter()
        ctx._check(ctx.lib.refind_pairs(ctx.h, rf.h, n, hl.mrh_pair_data(), p(out), p(kept)), "refind_pairs")
        t3 = time.perf_counter()
        rows = hl.mrh_fold(m, n, p(out), p(table))
        t4 = time.perf_counter()
        hl.mrh_destroy(m)
        tl.append(t1 - t0)
        tc.append(t3 - t2)
        tf.append(t4 - t3)
    rf.close()
    total = [a + b + c for a, b, c in zip(tl, tc, tf)]
    return {"host_loop": stats(tl), "refind_pairs": stats(tc), "fold_and_table": stats(tf), "total": stats(total)}, out, table[:rows].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["device", "composed"])
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--pass-sizes", default="", help="also time the one call at these max_pairs_per_pass (comma separated)")
    a = ap.parse_args()
    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    hl = build_host_lib(tempfile.mkdtemp()) if a.only != "device" else None
    for name in a.cases.split(","):
        mode, n_kf, n_points, n_work = CASES[name]
        scene, points, meas, never, work = make_map(ctx, mode, n_kf, n_points, n_work)
        line = {"case": name, "keyframes": n_kf, "points": n_points, "meas_rows": len(meas), "never_rows": len(never)}
        dev = comp = None
        if a.only != "composed":
            line["one_call"], dev = time_device(ctx, mode, scene, points, meas, never, work, a.reps)
            line.update({f: dev[f] for f in ("n_pairs", "n_skipped", "n_found", "n_never", "n_template_kept")})
            for pp in [int(x) for x in a.pass_sizes.split(",") if x]:
                st, other = time_device(ctx, mode, scene, points, meas, never, work, a.reps, per_pass=pp)
                assert other["meas_merged"].tobytes() == dev["meas_merged"].tobytes()
                line["one_call_pass_%d" % pp] = st
        if hl is not None:
            line["composed"], comp, table = time_composed(ctx, hl, mode, scene, points, meas, never, work, a.reps)
        if dev is not None and comp is not None:   # the two paths computed the same thing
            assert int(comp["found"].sum()) == dev["n_found"] and int(comp["never_retry"].sum()) == dev["n_never"]
            assert table.tobytes() == dev["meas_merged"].tobytes()
            line["speedup"] = round(line["composed"]["total"]["median_ms"] / line["one_call"]["median_ms"], 2)
        print(json.dumps(line), flush=True)
        scene["close"]()
    ctx.close()


if __name__ == "__main__":
    main()
