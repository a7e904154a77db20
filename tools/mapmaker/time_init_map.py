"""Times ptam_rmap_init_from_stereo (host.ResidentMap.InitFromStereo) beside the composed host-table sequence of INTEGRATION.md —
stages 1-8 of MapMaker::InitFromStereo as host-table calls and a ResidentMap.upload at the end — on the trails of a rendered
sequence of the textured plane at 640 x 480.

    python tools/mapmaker/time_init_map.py [--reps 7] [--size 640x480] [--frames 11 --step 0.012] [--max-bundles 20]

Host clock around each whole path, median of --reps after two warm-up runs, both paths in one process on the same trails (the trail
tracking itself is outside the clock: it is the same for both).  Bytes over the host link: ptam_rmap_traffic for the one call; for
the composed sequence the sizes of the tables every call takes and returns (what its wrapper hands to and gets from the library),
plus ptam_rmap_traffic of the upload."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host  # noqa: E402
from tests import init_map_ref as IR  # noqa: E402


class Link:
    """the bytes a host-table call moves: its table arguments up, its table results down"""

    def __init__(self):
        self.up = self.down = 0

    def sent(self, *arrays):
        self.up += sum(np.asarray(a).nbytes for a in arrays)

    def got(self, *arrays):
        self.down += sum(np.asarray(a).nbytes for a in arrays if a is not None)


def composed_host_tables(ctx, first, second, trails, max_bundles, seeds, link):
    """INTEGRATION.md's InitFromStereo row, the pieces: every stage a host-table call, then the upload"""
    ok, se3, info, inl = trails.homography(seed=seeds[0])                                      # (1): on the device list; 256 + n down
    link.got(inl, np.zeros(32))
    assert ok
    _, se3 = IR.scaled(se3, 0.1)                                                               # (2)
    table = trails.read()                                                                      # the trail list down ...
    link.got(table)
    made, status = host.init_points_from_trails(ctx, first, second, se3, table)                # (3) ... and up again
    link.sent(table)
    link.got(made, status)
    N = len(made)
    add = host.map_add_points(ctx, 2, 0, np.zeros(0, host.MAP_MEAS_DT), 0, 1, made, _abi.SRC_TRAIL)
    link.sent(made)
    link.got(add["meas"], add["points"], add["sources"])
    t = dict(poses=np.stack([IR.IDENTITY, se3]), fixed=np.array([1, 0], np.uint8), points3=made["point"]["world"].copy(), points=add["points"],
             sources=add["sources"], bad=np.zeros(N, np.uint8), meas=add["meas"], never=np.zeros(0, host.MAP_PAIR_DT),
             failure=np.zeros(0, host.MAP_PAIR_DT), new_queue=add["new_queue"])
    n_bundles = 0

    def bundle():
        nonlocal n_bundles
        b = host.map_bundle_adjust(ctx, _abi.MAP_BA_ALL, t["poses"], t["fixed"], t["points3"], t["meas"], deterministic=1)
        link.sent(t["poses"], t["fixed"], t["points3"], t["meas"])
        link.got(b["poses"], b["points"], b["outliers"])
        t["poses"], t["points3"] = b["poses"], b["points"]
        t["points"]["pv"]["world"] = t["points3"]
        o = host.map_apply_outliers(ctx, 2, t["bad"], t["meas"], t["never"], t["failure"], b["outliers"])
        link.sent(t["bad"], t["meas"], t["never"], t["failure"], b["outliers"])
        link.got(o["bad"], o["meas"], o["never"], o["failure"])
        t.update(bad=o["bad"], meas=o["meas"], never=o["never"], failure=o["failure"])
        t["points"]["bad"] = t["bad"]
        n_bundles += 1
        return b["converged"]

    for _ in range(5):                                                                         # (4)
        bundle()
    depth = host.map_scene_depth(ctx, t["poses"], t["points3"], t["meas"])                     # (5)
    link.sent(t["poses"], t["points3"], t["meas"])
    link.got(depth)
    run = t["meas"][t["meas"]["kf"] == 1]                                                      # (6)
    mm = host.MapMaker(ctx)
    eo = mm.opts(levels=(0, 3, 1, 2), depth_mean=float(depth["depth_mean"][1]), depth_sigma=float(depth["depth_sigma"][1]))
    made2, stats = mm.AddSomeMapPoints(second, t["poses"][1], first, t["poses"][0], eo, busy_level=run["level"], busy_root=run["root_pos"])
    link.sent(run["level"], run["root_pos"])
    link.got(made2, stats)
    add = host.map_add_points(ctx, 2, len(t["points3"]), t["meas"], 1, 0, made2, _abi.SRC_EPIPOLAR)
    link.sent(t["meas"], made2)
    link.got(add["meas"], add["points"], add["sources"])
    A = len(made2)
    t.update(meas=add["meas"], points=np.concatenate([t["points"], add["points"]]), sources=np.concatenate([t["sources"], add["sources"]]),
             points3=np.concatenate([t["points3"], made2["point"]["world"]]), bad=np.concatenate([t["bad"], np.zeros(A, np.uint8)]),
             new_queue=np.concatenate([t["new_queue"], add["new_queue"]]))
    for _ in range(max_bundles):                                                               # (7)
        if bundle():
            break
    al = host.map_align_to_plane(ctx, t["poses"], t["points3"], t["sources"], seed=seeds[1])   # (8)
    link.sent(t["poses"], t["points3"], t["sources"])
    link.got(al["poses"], al["points"], al["pvs"], al["inliers"])
    t["poses"], t["points3"] = al["poses"].reshape(-1, 12), al["points"]
    t["points"]["pv"] = al["pvs"]
    m = host.ResidentMap(ctx)                                                                  # ... and the map becomes resident
    m.upload(kfs=[first, second], **t)
    up, down = m.traffic()
    link.up += up
    link.down += down
    return m, n_bundles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", default="640x480")
    ap.add_argument("--frames", type=int, default=11)
    ap.add_argument("--step", type=float, default=0.012, help="metres sideways per frame: about 5.5 px at 640 x 480")
    ap.add_argument("--max-bundles", type=int, default=20)
    a = ap.parse_args()
    size = tuple(int(x) for x in a.size.split("x"))
    seeds = (3, 5)
    frames, _ = IR.stereo_sequence(size, a.frames, step=a.step)
    ctx = host.Context(size=size)
    first, second, trails = IR.run_trails(ctx, frames)
    times = {"one call": [], "composed": []}
    note = {}
    for rep in range(a.reps + 2):
        m = host.ResidentMap(ctx)
        o = m.init_opts(max_bundles=a.max_bundles, ba=dict(deterministic=1), homography=dict(seed=seeds[0]), plane=dict(seed=seeds[1]))
        t0 = time.perf_counter()
        r = m.InitFromStereo(first, second, trails=trails, opts=o)
        t1 = time.perf_counter()
        note["one call"] = (m.traffic(), r["n_bundles"], m.counts()["n_points"], r["status"])
        m.close()
        link = Link()
        t2 = time.perf_counter()
        m2, nb = composed_host_tables(ctx, first, second, trails, a.max_bundles, seeds, link)
        t3 = time.perf_counter()
        note["composed"] = ((link.up, link.down), nb, m2.counts()["n_points"], 0)
        m2.close()
        if rep >= 2:
            times["one call"].append((t1 - t0) * 1e3)
            times["composed"].append((t3 - t2) * 1e3)
    print("%d x %d, %d frames, %d live trails, median of %d" % (size[0], size[1], a.frames, len(trails.read()), a.reps))
    print("%-10s %10s %12s %12s %8s %8s" % ("path", "ms", "bytes up", "bytes down", "bundles", "points"))
    for k in ("one call", "composed"):
        (up, down), nb, npts, status = note[k]
        print("%-10s %10.2f %12d %12d %8d %8d%s" % (k, float(np.median(times[k])), up, down, nb, npts, "" if status == 0 else "  status %d" % status))
    trails.close()
    ctx.close()


if __name__ == "__main__":
    main()
