"""Times the keyframe section of the snapshot (ptam_snapshot_keyframes_enable: ptam_rmap_publish fills it,
ptam_sbi_bank_take_keyframes takes it) beside what it rides on and what it replaces, in one process, on the map of
tools/mapmaker/time_resident_map.py: 200 keyframes x 50 000 points, frames of 640x480.

    python tools/mapmaker/time_publish_keyframes.py [--reps 15] [--kf 200 --points 50000 --rows 800000]

Method of time_resident_map.py: host clock around the synchronous call, median of --reps after two warm-up calls; what a
repetition needs changed beforehand (a keyframe appended, the poses moved, a publish) happens outside the clock.
  (i)   ptam_rmap_publish into a snapshot without the section, into one with it in the steady state (nothing to make), and with one
        keyframe appended before every publish (the publishes alternate between two slots while no take holds one, so a slot lacks
        the two keyframes appended since it was last written: n_made is printed);
  (ii)  ptam_sbi_bank_take_keyframes after the poses moved and one keyframe was appended, against the composed path on a twin bank:
        ptam_rmap_download(KF_POSES) + ptam_sbi_bank_set_poses + one ptam_sbi_bank_add, and a wait for the twin's queue (the take is
        synchronous); the bytes over the host link on each side;
  (iii) the first publishes of the whole map into each slot of a fresh snapshot: every image is made."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ptam_cg_amd import host  # noqa: E402
from tests import map_edit_ref as E  # noqa: E402
from time_resident_map import UPLOAD_KEYS, median_ms, whole_map  # noqa: E402

SIZE = (640, 480)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--points", type=int, default=50000)
    ap.add_argument("--rows", type=int, default=800000)
    a = ap.parse_args()
    K, N, reps = a.kf, a.points, a.reps
    extra = 3 * (reps + 2) + 4                       # keyframes appended by (i) and by both sides of (ii)
    h = whole_map(E.make_tables(7, K, N, a.rows, bad_share=0.005, count_share=0.005, lonely=0))

    from ptam_cg_amd._lib import load
    ctx = host.Context(lib=load(), size=SIZE)
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, SIZE[::-1], dtype=np.uint8) for _ in range(8)]
    kfs = [host.KeyFrame(ctx).MakeKeyFrame_Lite(images[k % 8]) for k in range(K + extra)]
    m = host.ResidentMap(ctx)
    m.reserve(n_kf=K + extra, n_points=2 * N, n_meas=2 * len(h["meas"]))
    m.upload(kfs=kfs[:K], **{k: h[k] for k in UPLOAD_KEYS})
    ctx.sync()
    print(f"K={K} N={N} rows={len(h['meas'])} frames {SIZE[0]}x{SIZE[1]}, median of {reps}")
    appended = [K]
    row = np.zeros(1, host.MAP_KF_ROW_DT)
    shift = np.concatenate([np.eye(3).reshape(9), [1e-3, -2e-3, 5e-4]])

    def append():
        m.add_keyframe(h["poses"][0], 0, row, kf=kfs[appended[0]])
        appended[0] += 1

    def traffic(fn):
        up0, down0 = m.traffic()
        r = fn()
        up, down = m.traffic()
        return r, up - up0, down - down0

    # ---- (iii) first, on fresh snapshots: every image of the map is made, once per slot
    plain = host.MapSnapshot(ctx, N)
    snap = host.MapSnapshot(ctx, N)
    snap.enable_keyframes(K + extra)
    m.publish(plain)
    m.publish(plain)                                  # (both of its slots have been written: no growth, kernels loaded)
    first = []
    for _ in range(2):
        t0 = time.perf_counter()
        m.publish(snap)
        first.append(((time.perf_counter() - t0) * 1e3, snap.keyframes()["n_made"]))
    print("(iii) first publish into a slot: " + ", ".join(f"{ms:.3f} ms (made {n})" for ms, n in first))

    # ---- (i) publish
    t_plain = median_ms(lambda: m.publish(plain), reps)
    t_steady = median_ms(lambda: m.publish(snap), reps)
    _, up_p, _ = traffic(lambda: m.publish(plain))
    _, up_s, _ = traffic(lambda: m.publish(snap))
    made = []
    t_one = median_ms(lambda: (m.publish(snap), made.append(snap.keyframes()["n_made"])), reps, prep=append)
    print(f"(i) publish: plain {t_plain:.3f} ms ({up_p} B up) | with keyframes, steady {t_steady:.3f} ms ({up_s} B up) | "
          f"a keyframe appended before each {t_one:.3f} ms (made {sorted(set(made[2:]))} per publish)")

    # ---- (ii) take against the composed path
    rel = host.Relocaliser(ctx, K + extra, size=SIZE)
    twin = host.Relocaliser(ctx, K + extra, size=SIZE)
    rel.take_keyframes(snap)
    n0 = rel.count()
    twin.add_batch(kfs[:n0], m.download("poses"))
    ctx.sync()
    got = []

    def changed():
        append()
        m.apply_global_transform(shift, rows=False)
        m.publish(snap)

    def composed():
        n = twin.count()
        twin.add(kfs[n], h["poses"][0])
        twin.set_poses(0, m.download("poses"))
        ctx.sync()

    t_take = median_ms(lambda: got.append(rel.take_keyframes(snap)), reps, prep=changed)
    link_take = got[-1]["link_bytes"]
    n_kf = got[-1]["n_kf"]
    # the twin catches up with the keyframes (ii) appended so far, then one more per repetition, as the take saw them
    while twin.count() < rel.count():
        twin.add(kfs[twin.count()], h["poses"][0])
    down = []

    def composed_prep():
        append()
        m.apply_global_transform(shift, rows=False)

    def composed_counted():
        _, _, d = traffic(composed)
        down.append(d)

    t_comp = median_ms(composed_counted, reps, prep=composed_prep)
    k_now = twin.count()
    print(f"(ii) take after the poses moved and one keyframe came: {t_take:.3f} ms, {link_take} B down, 0 B up ({n_kf} keyframes, "
          f"{got[-1]['n_new']} new) | composed download + set_poses + one add: {t_comp:.3f} ms, {down[-1]} B down, {96 * k_now + 96} B up "
          f"({k_now} keyframes)")
    for o in [rel, twin, snap, plain, m] + kfs:
        o.close()
    ctx.close()


if __name__ == "__main__":
    main()
