"""Times stages (8) and (5) of InitFromStereo on the device at 2 000 and 50 000 points x 200 keyframes with 100 trials, beside the
numpy restatement (tests/plane_ref.py), and prints one JSON line.  Per size:
  align_call_us     ptam_map_align_to_plane with a source table (synchronous: the tables up, three launches, everything down, one
                    wait), the C call alone on fresh copies of the tables
  align_upload_us   ptam_dev_upload of as many bytes as the call sends up (points, poses, sources), one synchronous copy
  align_download_us ptam_dev_download of as many bytes as it brings down (poses, points, pixel-vector rows, inlier bytes)
  align_rest_us     call - upload - download: the three kernels, their launches, the staging copies and the wait
  depth_call_us / depth_upload_us / depth_rest_us   the same for ptam_map_scene_depth (its result arrives through host-mapped
                    memory: nothing is downloaded); every keyframe measures --per-kf points
  numpy_align_s / numpy_depth_s   the restatement, once
Host clock around each synchronous call; the median of --reps runs after 3 warm-ups.
Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/mapmaker/time_plane_align.py`."""
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

from ptam_cg_amd import _abi, host  # noqa: E402
from ptam_cg_amd._lib import load  # noqa: E402
from tests import plane_ref as PR  # noqa: E402


def median_us(fn, reps, before=lambda: None):
    ts = []
    for _ in range(reps + 3):
        before()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(ts[3:]), 1)


def copy_us(ctx, nbytes, reps, up):
    buf, arr = host.DevBuf(ctx, nbytes), np.zeros(nbytes, np.uint8)
    fn = ctx.lib.dev_upload if up else ctx.lib.dev_download
    args = (ctx.h, buf.p, arr.ctypes.data, nbytes) if up else (ctx.h, arr.ctypes.data, buf.p, nbytes)
    t = median_us(lambda: fn(*args), reps)
    buf.free()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 50000])
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--per-kf", type=int, default=2000)
    ap.add_argument("--trials", type=int, default=100)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    lib = load()
    ctx = host.Context(lib=lib)
    p = host._ptr
    res = {"trials": a.trials, "keyframes": a.keyframes, "reps": a.reps}
    for n in a.sizes:
        K = a.keyframes
        points, poses, sources, _, _ = PR.make_map(n, 0, K, with_meas=False)
        rng = np.random.default_rng(1)
        per_kf = min(a.per_kf, n)
        meas = np.zeros(K * per_kf, host.MAP_MEAS_DT)
        meas["kf"] = np.repeat(np.arange(K), per_kf)
        meas["point"] = np.concatenate([np.sort(rng.permutation(n)[:per_kf]) for _ in range(K)])
        table = host.plane_samples(lib, 7, n, a.trials)
        opts = host._plane_opts(lib, 0.05, 0, table, a.trials)
        w_poses, w_points = poses.copy(), points.copy()
        out, inl = np.zeros(n, host.PVS_POINT_DT), np.zeros(n, np.uint8)
        se3, info = np.zeros(12), _abi.PlaneInfo()

        def restore():
            w_poses[:], w_points[:] = poses, points

        def align():
            assert lib.map_align_to_plane(ctx.h, C.byref(opts), K, p(w_poses), n, p(w_points), p(sources), p(out), host._pd(se3),
                                          C.byref(info), p(inl)) == 0 and info.status == _abi.PLANE_OK

        depth = np.zeros(K, host.SCENE_DEPTH_DT)

        def scene_depth():
            assert lib.map_scene_depth(ctx.h, K, p(w_poses), n, p(w_points), len(meas), p(meas), p(depth)) == 0

        r = {"measurements": len(meas)}
        r["align_call_us"] = median_us(align, a.reps, restore)
        r["inliers"] = info.n_inliers
        r["align_upload_us"] = copy_us(ctx, points.nbytes + poses.nbytes + sources.nbytes, a.reps, True)
        r["align_download_us"] = copy_us(ctx, points.nbytes + poses.nbytes + out.nbytes + inl.nbytes, a.reps, False)
        r["align_rest_us"] = round(r["align_call_us"] - r["align_upload_us"] - r["align_download_us"], 1)
        r["depth_call_us"] = median_us(scene_depth, a.reps)
        r["depth_upload_us"] = copy_us(ctx, points.nbytes + poses.nbytes + meas.nbytes, a.reps, True)
        r["depth_rest_us"] = round(r["depth_call_us"] - r["depth_upload_us"], 1)
        if not a.no_numpy:
            t0 = time.perf_counter()
            ref = PR.calc_plane_aligner(points, table, 0.05)
            PR.apply_global_transform(ref["se3"], poses, points, sources)
            r["numpy_align_s"] = round(time.perf_counter() - t0, 3)
            t0 = time.perf_counter()
            PR.scene_depth(w_poses, w_points, meas)
            r["numpy_depth_s"] = round(time.perf_counter() - t0, 3)
            r["same_trial_and_inliers"] = bool(ref["best_trial"] == info.best_trial and ref["n_inliers"] == info.n_inliers)
        res[str(n)] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
