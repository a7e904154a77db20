"""Times the resident forms (ptam_rmap_*, host.ResidentMap) beside the host-table forms they stand for, in one process, on the
inputs of tools/mapmaker/time_map_edit.py: 200 keyframes x 50 000 points x 800 000 rows, 0.5 % of the points bad, 0.5 % of the rows
outliers, 2 000 new points; and the bundle on a case of tools/mapmaker/time_map_ba.py.

    python tools/mapmaker/time_resident_map.py [--reps 15] [--kf 200 --points 50000 --rows 800000] [--ba all200|all50|none]
                                               [--refind new200x2000,keyframe50000|none]

Method of time_map_edit.py: host clock around the synchronous call, output buffers allocated beforehand, median of --reps after two
warm-up calls.  A resident call changes the map it runs on, so before every repetition the map it starts from is uploaded again,
outside the clock.  `iteration`: apply_outliers, note_tracked, handle_bad_points, add_keyframe, add_points, scene_depth in a row on
one resident map, against the four of them that have a host-table form.  Re-find runs on the cases and maps of time_map_refind.py,
the resident call taking the resident queue and asking for no lists.
The last column is the host-link traffic of the resident call (ptam_rmap_traffic)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import _abi, host, synth  # noqa: E402
from tests import map_ba_ref as R  # noqa: E402
from tests import map_edit_ref as E  # noqa: E402

UPLOAD_KEYS = ("poses", "fixed", "points3", "points", "sources", "bad", "meas", "never", "new_queue", "failure", "outlier_count", "inlier_count")
BA_CASES = {"all50": (_abi.MAP_BA_ALL, 50, 5000, None), "all200": (_abi.MAP_BA_ALL, 200, 50000, 16)}


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


def whole_map(t, seed=9):
    """a keyframe side and a point side around the tables of tests/map_edit_ref.make_tables; the redundant columns agree"""
    rng = np.random.default_rng(seed)
    K, N = t["n_kf"], t["n_points"]
    _, pts, src = E.point_columns(seed, N)
    pts["src_kf"] = rng.integers(0, K, N)
    pts["bad"], src["src_kf"] = t["bad"], pts["src_kf"]
    poses = np.tile(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), (K, 1))
    poses[:, 9:] = rng.uniform(-0.2, 0.2, (K, 3))
    h = dict(poses=poses, fixed=(np.arange(K) == 0).astype(np.uint8), points3=pts["pv"]["world"].copy(), points=pts, sources=src)
    for k in ("bad", "meas", "never", "new_queue", "failure", "outlier_count", "inlier_count"):
        h[k] = t[k].copy()
    return h


def after(h, **tables):
    out = dict(h)
    out.update(tables)
    if "bad" in tables and "points" not in tables:
        out["points"] = h["points"].copy()
        out["points"]["bad"] = tables["bad"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    ap.add_argument("--made", type=int, default=2000)
    ap.add_argument("--ba", default="all200")
    ap.add_argument("--refind", default="new200x2000,keyframe50000")
    a = ap.parse_args()
    K, N = a.kf, a.points
    t = E.make_tables(7, K, N, a.rows, bad_share=0.005, count_share=0.005, lonely=0)
    outliers = E.make_outliers(8, K, N, t["meas"], len(t["meas"]) // 200)
    made = E.make_made(9, a.made)
    src_kf, target_kf = K - 1, K - 2
    h0 = whole_map(t)
    cols = ("points3", "points", "sources", "outlier_count", "inlier_count")
    ra = E.np_apply_outliers(K, h0["bad"], h0["meas"], h0["never"], h0["failure"], outliers)
    h1 = after(h0, bad=ra["bad"], meas=ra["meas"], never=ra["never"], failure=ra["failure"])
    rb = E.np_handle_bad_points(K, N, h1["meas"], h1["never"], h1["bad"], h1["outlier_count"], h1["inlier_count"], h1["new_queue"], h1["failure"],
                                [h1[c] for c in cols])
    nk = rb["n_kept"]
    h2 = after(h1, meas=rb["meas"], never=rb["never"], new_queue=rb["new_queue"], failure=rb["failure"], bad=np.zeros(nk, np.uint8),
               **{c: x[:nk].copy() for c, x in zip(cols, rb["columns"])})
    h2["points"]["bad"] = 0
    rng = np.random.default_rng(3)
    rows = np.zeros(len(t["meas"]) // K, host.MAP_KF_ROW_DT)
    rows["point"] = np.sort(rng.choice(nk, size=len(rows), replace=False))
    rows["level"], rows["root_pos"] = rng.integers(0, 4, len(rows)), rng.random((len(rows), 2)) * 600
    tracked, flags = rng.integers(0, nk, 1000).astype(np.int32), (rng.random(1000) < 0.1).astype(np.uint8)   # (of the compacted table)
    print(f"K={K} N={N} rows={len(t['meas'])} never={len(t['never'])} new queue={len(t['new_queue'])} failure queue={len(t['failure'])} "
          f"outliers={len(outliers)} made={len(made)} keyframe rows={len(rows)} tracked={len(tracked)}; removed {rb['n_removed']} points")

    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load())
    m = host.ResidentMap(ctx)
    m.reserve(n_kf=2 * K, n_points=2 * N, n_meas=2 * len(t["meas"]), n_never=2 * len(t["never"]) + len(outliers),
              n_new=2 * len(t["new_queue"]) + len(made), n_failure=2 * len(t["failure"]) + len(outliers))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    up = lambda h: (lambda: m.upload(**{k: h[k] for k in UPLOAD_KEYS}))

    # ---- the resident calls, through ctypes with everything allocated beforehand
    ro, rbr, depth = _abi.MapOutliersResult(), _abi.MapBadPointsResult(), np.zeros(K + 1, host.SCENE_DEPTH_DT)
    kept = np.zeros(N, np.int32)
    pose = np.ascontiguousarray(h0["poses"][0])

    def ok(rc):
        assert rc == 0, (rc, ctx.lib.last_error())
    res = {
        "apply_outliers": (up(h0), lambda: ok(ctx.lib.rmap_apply_outliers(m.h, len(outliers), p(outliers), C.byref(ro)))),
        "handle_bad_points": (up(h1), lambda: ok(ctx.lib.rmap_handle_bad_points(m.h, C.byref(rbr), p(kept), None))),
        "add_points": (up(h2), lambda: ok(ctx.lib.rmap_add_points(m.h, src_kf, target_kf, _abi.SRC_EPIPOLAR, len(made), p(made)))),
        "add_keyframe": (up(h2), lambda: ok(ctx.lib.rmap_add_keyframe(m.h, None, host._pd(pose), 0, len(rows), p(rows)))),
        "note_tracked": (up(h2), lambda: ok(ctx.lib.rmap_note_tracked(m.h, len(tracked), p(tracked), p(flags)))),
        "scene_depth": (up(h2), lambda: ok(ctx.lib.rmap_scene_depth(m.h, p(depth)))),
    }

    def iteration():
        for name in ("apply_outliers", "handle_bad_points", "note_tracked", "add_keyframe"):
            res[name][1]()
        ok(ctx.lib.rmap_add_points(m.h, K, target_kf, _abi.SRC_EPIPOLAR, len(made), p(made)))
        res["scene_depth"][1]()
    res["iteration"] = (up(h0), iteration)

    # ---- the host-table forms on the same tables
    M, V, F, O, A = len(h0["meas"]), len(h0["never"]), len(h0["failure"]), len(outliers), len(made)
    mo, no, fo = np.zeros(M + 2 * A + len(rows), E.MEAS_DT), np.zeros(V + O, E.PAIR_DT), np.zeros(F + O, E.PAIR_DT)
    ni, qo = np.zeros(N, np.int32), np.zeros(len(h0["new_queue"]), np.int32)
    pts_o, src_o = np.zeros(A, E.POINT_DT), np.zeros(A, E.SOURCE_DT)
    bad = h0["bad"].copy()
    wcols = [h1[c].copy() for c in cols]
    ctab, _ = host.map_columns(wcols)

    def reset_bad():
        bad[:] = h0["bad"]

    def reset():
        reset_bad()
        for w, c in zip(wcols, cols):
            w[:] = h1[c]
    tab = {
        "apply_outliers": (reset_bad, lambda: ok(ctx.lib.map_apply_outliers(ctx.h, K, N, M, p(h0["meas"]), V, p(h0["never"]), F, p(h0["failure"]), O,
                                                                        p(outliers), p(bad), C.byref(ro), p(mo), p(no), p(fo)))),
        "handle_bad_points": (reset, lambda: ok(ctx.lib.map_handle_bad_points(
            ctx.h, K, N, p(h1["bad"]), p(h1["outlier_count"]), p(h1["inlier_count"]), len(h1["meas"]), p(h1["meas"]), len(h1["never"]),
            p(h1["never"]), len(h1["new_queue"]), p(h1["new_queue"]), len(h1["failure"]), p(h1["failure"]), len(cols), C.cast(ctab, C.c_void_p),
            C.byref(rbr), p(ni), p(kept), p(mo), p(no), p(qo), p(fo)))),
        "add_points": (None, lambda: ok(ctx.lib.map_add_points(ctx.h, K, nk, len(h2["meas"]), p(h2["meas"]), src_kf, target_kf, _abi.SRC_EPIPOLAR, A,
                                                               p(made), p(mo), p(pts_o), p(src_o)))),
        "scene_depth": (None, lambda: ok(ctx.lib.map_scene_depth(ctx.h, K, p(h2["poses"]), nk, p(h2["points3"]), len(h2["meas"]), p(h2["meas"]),
                                                                 p(depth)))),
    }

    def table_iteration():
        for name in ("apply_outliers", "handle_bad_points", "add_points", "scene_depth"):
            tab[name][1]()
    tab["iteration"] = (reset, table_iteration)

    for name, (prep, call) in res.items():
        prep()
        before = m.traffic()
        call()
        moved = tuple(x - y for x, y in zip(m.traffic(), before))
        line = f"{name:18s} resident {median_ms(call, a.reps, prep):8.3f} ms"
        if name in tab:
            line += f" | host tables {median_ms(tab[name][1], a.reps, tab[name][0]):8.3f} ms"
        print(line + f" | resident traffic up {moved[0]} B, down {moved[1]} B", flush=True)
    # the resident iteration ends in the tables the references give
    up(h0)()
    iteration()
    got = m.download("meas")
    assert len(got) == len(h2["meas"]) + len(rows) + 2 * A and m.counts()["n_points"] == nk + A, (len(got), len(h2["meas"]))
    assert E.tables_valid(K + 1, nk + A, got, m.download("never"))
    m.close()

    if a.ba in BA_CASES:
        mode, Kb, Pb, w = BA_CASES[a.ba]
        poses, fixed, points, meas = R.map_from_problem(synth.make_ba_problem(Kb, Pb, 7, window=w), seed=7, extra_fixed=(Kb // 2,))
        hb = whole_map(dict(n_kf=Kb, n_points=Pb, bad=np.zeros(Pb, np.uint8), meas=meas, never=np.zeros(0, E.PAIR_DT),
                            new_queue=np.zeros(0, np.int32), failure=np.zeros(0, E.PAIR_DT), outlier_count=np.zeros(Pb, np.int32),
                            inlier_count=np.zeros(Pb, np.int32)))
        hb.update(poses=poses, fixed=fixed, points3=points)
        hb["points"]["pv"]["world"] = points
        mb = host.ResidentMap(ctx)
        o = _abi.BaOpts()
        ctx.lib.ba_opts_default(C.byref(o))
        out, rba = np.zeros(len(meas), host.MAP_OUTLIER_DT), _abi.MapBaResult()
        prep = lambda: mb.upload(**{k: hb[k] for k in UPLOAD_KEYS})
        call = lambda: ok(ctx.lib.rmap_bundle_adjust(mb.h, C.byref(o), mode, None, C.byref(rba), p(out), len(meas), None, None))
        prep()
        before = mb.traffic()
        call()
        moved = tuple(x - y for x, y in zip(mb.traffic(), before))
        r_ms = median_ms(call, a.reps, prep)
        pw, xw = poses.copy(), points.copy()

        def tprep():
            pw[:], xw[:] = poses, points
        t_ms = median_ms(lambda: ok(ctx.lib.map_bundle_adjust(ctx.h, C.byref(o), mode, Kb, p(pw), p(fixed), Pb, p(xw), len(meas), p(meas), None,
                                                              C.byref(rba), p(out), len(meas), None, None)), a.reps, tprep)
        print(f"bundle {a.ba:11s} resident {r_ms:8.3f} ms | host tables {t_ms:8.3f} ms | resident traffic up {moved[0]} B, down {moved[1]} B "
              f"(K={Kb} N={Pb} M={len(meas)}, accepted {rba.accepted}, outliers {rba.n_outliers})", flush=True)
        mb.close()

    if a.refind != "none":   # the cases and the maps of time_map_refind.py; the lists are not asked for, the merged tables stay
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import time_map_refind as TR
        for name in a.refind.split(","):
            mode, Kr, Nr, Wr = TR.CASES[name]
            scene, points, meas, never, work = TR.make_map(ctx, mode, Kr, Nr, Wr)
            hr = whole_map(dict(n_kf=Kr, n_points=Nr, bad=np.zeros(Nr, np.uint8), meas=meas, never=never, new_queue=np.zeros(0, np.int32),
                                failure=np.zeros(0, E.PAIR_DT), outlier_count=np.zeros(Nr, np.int32), inlier_count=np.zeros(Nr, np.int32)))
            hr.update(poses=np.ascontiguousarray(scene["poses"]), points=points, points3=np.ascontiguousarray(points["pv"]["world"]))
            hr["sources"]["src_kf"] = points["src_kf"]
            if mode == _abi.MAP_REFIND_NEW_POINTS:
                hr["new_queue"] = work
            mr = host.ResidentMap(ctx)
            mr.reserve(n_meas=len(meas) + Kr * max(Wr, 1) + Nr, n_never=len(never) + Kr * max(Wr, 1) + Nr)
            rf, rres = host.ReFinder(ctx), _abi.MapRefindResult()
            prep = lambda: mr.upload(kfs=scene["kfs"], **{k: hr[k] for k in UPLOAD_KEYS})
            from_queue = mode == _abi.MAP_REFIND_NEW_POINTS
            call = lambda: ok(ctx.lib.rmap_refind(mr.h, rf.h, None, mode, 0 if from_queue else len(work), None if from_queue else p(work), None,
                                                  C.byref(rres), None, None, None, 0))
            prep()
            before = mr.traffic()
            call()
            moved = tuple(x - y for x, y in zip(mr.traffic(), before))
            r_ms = median_ms(call, a.reps, prep)
            t_stats, t_res = TR.time_device(ctx, mode, scene, points, meas, never, work, a.reps)
            assert (rres.n_found, rres.n_never) == (t_res["n_found"], t_res["n_never"]), (rres.n_found, t_res["n_found"])
            print(f"refind {name:14s} resident {r_ms:8.3f} ms | host tables {t_stats['median_ms']:8.3f} ms | resident traffic up {moved[0]} B, "
                  f"down {moved[1]} B (K={Kr} N={Nr} M={len(meas)}, pairs {rres.n_pairs}, found {rres.n_found})", flush=True)
            rf.close()
            mr.close()
            scene["close"]()
    ctx.close()


if __name__ == "__main__":
    main()
