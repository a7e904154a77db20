"""Times ptam_map_bundle_adjust (MapMaker::BundleAdjustRecent / BundleAdjustAll as one device call) against the host work it
replaces: the set choice and Add* marshalling of src/MapMaker.cc:768-882 restated in C++ with the reference's std::set / std::map
walk (tools/mapmaker/map_ba_host.cc, g++ -O2, one thread) over the same tables.

    python tools/mapmaker/time_map_ba.py [--reps 10] [--only device|host] [--cases recent200,all50,all200]

Per case: the whole call (host clock around the synchronous call, tables copied before the clock starts, median of --reps after
two warm-up calls) and the host restatement (median of --reps).  The device selection + marshal time alone comes from a kernel
trace of the same command (rocprofv3 --kernel-trace --stats: mba_select/mark/fixed/ids/compact_kernel), see docs/LOG_mapmaker.md.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host, synth  # noqa: E402
from tests import map_ba_ref as R  # noqa: E402

CASES = {   # name: (mode, keyframes, points, window)
    "recent200": (_abi.MAP_BA_RECENT, 200, 180000, 8),   # ~3 000 points in the local set
    "all50": (_abi.MAP_BA_ALL, 50, 5000, None),
    "all200": (_abi.MAP_BA_ALL, 200, 50000, 16),
}


def build_host_tool(out_dir):
    exe = os.path.join(out_dir, "map_ba_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "mapmaker", "map_ba_host.cc"), "-o", exe])
    return exe


def write_tables(path, mode, poses, fixed, points, meas):
    with open(path, "wb") as f:
        f.write(np.array([mode, len(poses), len(points), len(meas)], np.int32).tobytes())
        f.write(poses.tobytes() + fixed.tobytes() + points.tobytes() + np.ascontiguousarray(meas, host.MAP_MEAS_DT).tobytes())


def time_device(ctx, mode, poses, fixed, points, meas, reps):
    o = _abi.BaOpts()
    ctx.lib.ba_opts_default(C.byref(o))
    meas = np.ascontiguousarray(meas, host.MAP_MEAS_DT)
    out = np.zeros(len(meas), host.MAP_OUTLIER_DT)
    res = _abi.MapBaResult()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t = []
    for r in range(reps + 2):
        pw, xw = poses.copy(), points.copy()
        t0 = time.perf_counter()
        rc = ctx.lib.map_bundle_adjust(ctx.h, C.byref(o), mode, len(pw), p(pw), p(fixed), len(xw), p(xw), len(meas), p(meas), None,
                                       C.byref(res), p(out), len(meas), None, None)
        t1 = time.perf_counter()
        assert rc == 0, rc
        if r >= 2:
            t.append((t1 - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), {f: getattr(res, f) for f, _ in _abi.MapBaResult._fields_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["device", "host"])
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    exe = build_host_tool(tmp) if a.only != "device" else None
    ctx = None
    if a.only != "host":
        from ptam_cg_amd._lib import load
        ctx = host.Context(lib=load())
    for name in a.cases.split(","):
        mode, K, P, w = CASES[name]
        tabs = R.map_from_problem(synth.make_ba_problem(K, P, 7, window=w), seed=7, extra_fixed=(K // 2,))
        line = f"{name:10s} K={K} N={P} M={len(tabs[3])}"
        if ctx is not None:
            med, mn, res = time_device(ctx, mode, *tabs, a.reps)
            line += (f" | device call {med:.3f} ms (min {mn:.3f}) accepted {res['accepted']} cams {res['n_adjust']}+{res['n_fixed']}"
                     f" points {res['n_points']} meas {res['n_meas']} outliers {res['n_outliers']}")
        if exe is not None:
            path = os.path.join(tmp, name + ".bin")
            write_tables(path, mode, *tabs)
            h = subprocess.check_output([exe, path, str(a.reps)], text=True).split()
            line += f" | host set choice + Add* {float(h[2]):.3f} ms (min {float(h[3]):.3f}) cams {h[4]} points {h[5]} meas {h[6]}"
        print(line, flush=True)
    if ctx is not None:
        ctx.close()


if __name__ == "__main__":
    main()
