"""Times the calibrator's optimiser on the device (ptam_calib_*): per problem the microseconds per step inside one 300-step call,
the microseconds of a call of one step (their difference is the price of a host round trip per step, which the reference's GUI
loop pays), the initial-pose call, and for the small problems one step of the numpy restatement (tests/calib_ref.py) on this node's
CPU.  Median of 7 with min-max, one visit.  Prints one JSON line per problem.

    python tools/calib/time_calib.py [--repeats 7] [--steps 300]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from ptam_cg_amd import host, synth   # noqa: E402

TRUTH = (0.62, 0.83, 0.48, 0.53, 0.9)
SIZE = (640, 480)
PROBLEMS = (("4 x 48", 4, 8, 6, (6.0, 10.0), True), ("40 x 48", 40, 8, 6, (6.0, 10.0), True), ("1000 x ~80", 1000, 10, 8, (8.0, 14.0), False))


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(us[0]), 2), "max_us": round(float(us[-1]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    ctx = host.Context(size=SIZE)
    for name, n_images, gw, gh, dist, with_numpy in PROBLEMS:
        grids = [c for c, _ in synth.make_calib_grids(TRUTH, SIZE, n_images, gw, gh, 11, distance=dist)]
        cal = host.CameraCalibrator(ctx, n_images, sum(len(c) for c in grids))
        guess, many, single = [], [], []
        for rep in range(a.repeats + 1):          # (the first repeat warms up and is dropped)
            cal.Reset()
            t0 = time.perf_counter()
            assert not cal.AddImages(grids).any()
            t1 = time.perf_counter()
            cal.Optimize(a.steps)
            t2 = time.perf_counter()
            for _ in range(20):
                cal.Optimize(1)
            t3 = time.perf_counter()
            if rep:
                guess.append((t1 - t0) * 1e6)
                many.append((t2 - t1) * 1e6 / a.steps)
                single.append((t3 - t2) * 1e6 / 20)
        out = {"problem": name, "images": n_images, "corners": int(sum(len(c) for c in grids)), "steps_per_call": a.steps,
               "step_in_call": stats(many), "call_of_one_step": stats(single), "add_images_call": stats(guess),
               "params_error_after_call": float(np.abs(cal.Params() - np.array(TRUTH)).max())}
        out["round_trip_us"] = round(out["call_of_one_step"]["median_us"] - out["step_in_call"]["median_us"], 2)
        if with_numpy:
            from tests import calib_ref as CR
            ref = CR.Calibrator(SIZE)
            for c in grids:
                ref.add_image(c)
            cpu = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                ref.optimize_one_step()
                cpu.append((time.perf_counter() - t0) * 1e6)
            out["numpy_step"] = stats(cpu)
        cal.close()
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
