"""Times the two device-planned calls of a MapMaker::run() iteration beside the host-composed sequences they stand for, in one
process, at 200 keyframes x 50 000 points x 800 000 rows:

    bundle      ptam_rmap_bundle_adjust_routed(ALL)            | ptam_rmap_bundle_adjust (outliers down) + ptam_rmap_apply_outliers (up)
                on maps whose bundle reports about 0, 100 and 10 000 outliers (the share of displaced measurements is chosen for it)
    refind      ptam_rmap_refind_queue(NEW_POINTS), 2 000 new points | ptam_rmap_refind(work = NULL)
                ptam_rmap_refind_queue(FAILURE_QUEUE), 2 000 pairs   | ptam_rmap_refind(work = NULL)
                on the map of tools/mapmaker/time_map_refind.py (200 keyframe entries x 20 000 points)

    step        ptam_mapmaker_step (host.MapMaker.Step)         | tests/mapmaker_run_ref.RefMapMaker.Step: the same iteration composed
                from ptam_rmap_bundle_adjust + ptam_rmap_apply_outliers, ptam_rmap_refind(work = NULL) and ptam_rmap_handle_bad_points,
                both through the Python wrappers, on the re-find map with its 2 000 new points queued and both flags down: the
                RECENT bundle, ReFindNewlyMade, the full bundle when the first converged, HandleBadPoints

    python tools/mapmaker/time_mapmaker_step.py [--reps 9] [--kf 200 --points 50000] [--bundle 0,100,10000|none] [--refind new,failure|none]
                                                [--step yes|no]

Method: host clock around the synchronous calls, everything allocated beforehand.  A call changes the map it runs on, so the map is
uploaded again before every timed call, outside the clock.  The two forms alternate, repetition by repetition, on one handle; two
warm-up rounds are dropped; the line gives each form's median, its lowest time and its quartile spread (q75 - q25), and the
host-link bytes of one call of each (ptam_rmap_traffic).  Both forms must end in the same counts."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ptam_cg_amd import _abi, host, synth  # noqa: E402
from tests import map_ba_ref as R  # noqa: E402
from tests import map_edit_ref as E  # noqa: E402
import time_map_refind as TR  # noqa: E402
from time_resident_map import UPLOAD_KEYS, whole_map  # noqa: E402


def alternate(forms, prep, reps, m):
    """forms: {name: call}.  -> {name: (median, min, q75 - q25) in ms, (bytes up, bytes down) of one call, the counts afterwards}"""
    t = {k: [] for k in forms}
    moved, counts = {}, {}
    for r in range(reps + 2):
        for name, call in forms.items():
            prep()
            before = m.traffic()
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            moved[name] = tuple(x - y for x, y in zip(m.traffic(), before))
            counts[name] = m.counts()
            if r >= 2:
                t[name].append((t1 - t0) * 1e3)
    out = {}
    for name, v in t.items():
        q25, q50, q75 = np.percentile(v, [25, 50, 75])
        out[name] = ((float(q50), float(min(v)), float(q75 - q25)), moved[name], counts[name])
    return out


def report(what, res):
    names = list(res)
    assert res[names[0]][2] == res[names[1]][2], (what, res[names[0]][2], res[names[1]][2])
    for name in names:
        (med, low, spread), (up, down), _ = res[name]
        print(f"{what:28s} {name:10s} median {med:9.3f} ms  min {low:9.3f} ms  spread {spread:7.3f} ms | up {up} B, down {down} B", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--bundle", default="0,100,10000")
    ap.add_argument("--refind", default="new,failure")
    ap.add_argument("--step", default="yes")
    a = ap.parse_args()
    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    p = lambda x: x.ctypes.data_as(C.c_void_p)

    def ok(rc):
        assert rc == 0, (rc, ctx.lib.last_error())

    if a.bundle != "none":
        K, N = a.kf, a.points
        o = _abi.BaOpts()
        ctx.lib.ba_opts_default(C.byref(o))
        for want in (int(x) for x in a.bundle.split(",")):
            rows = 16 * N
            prob = synth.make_ba_problem(K, N, 7, window=16, outlier_frac=want / rows, **({} if want else {"pose_noise": 0.0}))
            poses, fixed, points, meas = R.map_from_problem(prob, seed=7, extra_fixed=(K // 2,))
            h = whole_map(dict(n_kf=K, n_points=N, bad=np.zeros(N, np.uint8), meas=meas, never=np.zeros(0, E.PAIR_DT),
                               new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT), outlier_count=np.zeros(N, np.int32),
                               inlier_count=np.zeros(N, np.int32)))
            h.update(poses=poses, fixed=fixed, points3=points)
            h["points"]["pv"]["world"] = points
            m = host.ResidentMap(ctx)
            m.reserve(n_never=len(meas), n_failure=len(meas))
            out, rba, ro = np.zeros(len(meas), host.MAP_OUTLIER_DT), _abi.MapBaResult(), _abi.MapOutliersResult()

            def composed():
                ok(ctx.lib.rmap_bundle_adjust(m.h, C.byref(o), _abi.MAP_BA_ALL, None, C.byref(rba), p(out), len(meas), None, None))
                ok(ctx.lib.rmap_apply_outliers(m.h, rba.n_outliers, p(out), C.byref(ro)))

            def routed():
                ok(ctx.lib.rmap_bundle_adjust_routed(m.h, C.byref(o), _abi.MAP_BA_ALL, None, C.byref(rba), C.byref(ro)))
            res = alternate({"composed": composed, "routed": routed}, lambda: m.upload(**{k: h[k] for k in UPLOAD_KEYS}), a.reps, m)
            report(f"bundle ALL, {rba.n_outliers} outliers (M={len(meas)})", res)
            m.close()

    if a.refind != "none" or a.step == "yes":
        mode, Kr, Nr, Wr = TR.CASES["new200x2000"]
        scene, points, meas, never, work = TR.make_map(ctx, mode, Kr, Nr, Wr)
        h = whole_map(dict(n_kf=Kr, n_points=Nr, bad=np.zeros(Nr, np.uint8), meas=meas, never=never, new_queue=work,
                           failure=np.zeros(0, E.PAIR_DT), outlier_count=np.zeros(Nr, np.int32), inlier_count=np.zeros(Nr, np.int32)))
        h.update(poses=np.ascontiguousarray(scene["poses"]), points=points, points3=np.ascontiguousarray(points["pv"]["world"]))
        h["sources"]["src_kf"] = points["src_kf"]
        rng = np.random.default_rng(5)
        h["failure"] = np.zeros(Wr, E.PAIR_DT)
        h["failure"]["kf"], h["failure"]["point"] = rng.integers(0, Kr, Wr), rng.integers(0, Nr - Wr, Wr)
        m = host.ResidentMap(ctx)
        m.reserve(n_meas=len(meas) + Kr * Wr, n_never=len(never) + Kr * Wr)
        rf, rres = host.ReFinder(ctx), _abi.MapRefindResult()
        prep = lambda: m.upload(kfs=scene["kfs"], **{k: h[k] for k in UPLOAD_KEYS})
        for name in (a.refind.split(",") if a.refind != "none" else []):
            md = {"new": _abi.MAP_REFIND_NEW_POINTS, "failure": _abi.MAP_REFIND_FAILURE_QUEUE}[name]
            res = alternate({"host plan": lambda: ok(ctx.lib.rmap_refind(m.h, rf.h, None, md, 0, None, None, C.byref(rres), None, None, None, 0)),
                             "queue": lambda: ok(ctx.lib.rmap_refind_queue(m.h, rf.h, None, md, None, C.byref(rres)))}, prep, a.reps, m)
            report(f"refind {name}, {rres.n_pairs} pairs", res)
        if a.step == "yes":
            from tests.mapmaker_run_ref import RefMapMaker
            mm = host.MapMaker(ctx, m, rf, None, host.MapMaker.mapmaker_opts(ctx, ba=dict(deterministic=1)))
            ref = RefMapMaker(m, rf, ba=dict(deterministic=1))
            for flags in ((0, 0), (1, 0)):   # the RECENT bundle first | ReFindNewlyMade and the full bundle
                last = {}

                def one(which):
                    def call():
                        which.set_flags(*flags)
                        last[which] = which.Step()
                    return call
                res = alternate({"composed": one(ref), "step": one(mm)}, prep, a.reps, m)
                assert last[ref]["stages"] == last[mm]["stages"] and last[ref]["refind_new"] == last[mm]["refind_new"], (last[ref], last[mm])
                report(f"step from flags {flags}, stages {last[mm]['stages']}, {last[mm]['refind_new']['n_pairs']} pairs", res)
            mm.close()
        rf.close()
        m.close()
        scene["close"]()
    ctx.close()


if __name__ == "__main__":
    main()
