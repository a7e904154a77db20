"""The point update (csrc/ba_update.inc, K10) rebuilds W_ij = A^T B in registers from the current pose and point
(ba_rebuild_w, csrc/ba_math.inc) instead of reading K7's W planes back.  Against the loading form (PTAM_UPDATE_LOADS_W=1, the
same library) and against the oracle, at the smallest shapes that reach each branch of the kernel.  Every case converges in a
few all-accepted trials on the oracle, so no trajectory hangs on last-bit noise."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from ptam_cg_amd import _abi, synth
from tests import util

pytestmark = pytest.mark.gpu

SWITCH = "PTAM_UPDATE_LOADS_W"
CAMS20 = dict(n_cams=20, n_pts=200, n_fixed=3, outlier_frac=0.1, seed=13)
# case -> (problem, options beside deterministic=1)
CASES = {
    # 8 measurements per point: a 256-measurement chunk holds more than 32 points, K10's later rounds (base != 0)
    "cams8_pts300": (dict(n_cams=8, n_pts=300, seed=11), {}),
    # 50 per point: points cut by K7's 64-measurement chunks (d.cut, V from pieces)
    "cams50_pts120": (dict(n_cams=50, n_pts=120, seed=12), {}),
    # fixed cameras (f < 0) and many measurements K7 turns MS_BAD inside a step: K10 must skip them exactly as the zero blocks did
    "cams20_pts200_fixed3_out10": (CAMS20, {}),
    # every point seen by 300 cameras: point_update_long (built as tests/test_gpu_parity.py::BA_UNBOUNDED_CASES builds it)
    "long_points_300x40": (dict(n_cams=300, n_pts=40, seed=31), dict(max_iterations=3)),
    # the general est_sqrt_weight path of the rebuilt weight
    "cams20_cauchy": (CAMS20, dict(estimator=_abi.EST_CAUCHY)),
    "cams20_huber": (CAMS20, dict(estimator=_abi.EST_HUBER)),
}


def _bit_equal(a, b):
    return (all(np.array_equal(a["trials"][k], b["trials"][k], equal_nan=True) for k in a["trials"].dtype.names)
            and np.array_equal(a["poses"], b["poses"], equal_nan=True) and np.array_equal(a["points"], b["points"], equal_nan=True))


@pytest.mark.parametrize("case", list(CASES))
def test_rebuilt_w_against_the_loaded_w_and_the_oracle(oracle, case, monkeypatch):
    """the default against PTAM_UPDATE_LOADS_W=1: the same discrete trajectory, every trial's numbers and the state to 1e-9 (the
    suite's bounds for "same trajectory, different arithmetic order"); against the oracle at the suite's 1e-6; no solve fell
    back; the default repeats to the last bit.  (The switch is read once per process: every run is a process of its own.)"""
    monkeypatch.delenv(SWITCH, raising=False)
    kw, extra = CASES[case]
    opts = dict(deterministic=1, **extra)
    a = util.run_ba_subprocess(kw, opts=opts)
    a2 = util.run_ba_subprocess(kw, opts=opts)
    old = util.run_ba_subprocess(kw, env={SWITCH: "1"}, opts=opts)
    ro = util.run_ba(oracle, synth.make_ba_problem(**kw), **extra)
    assert len(a["trials"]) > 0 and a["accepted"] > 0
    for r in (a, a2, old):
        assert r["solve_fallbacks"] == 0
    print(f"{case}: {len(a['trials'])} trials, {len(a['outliers'])} outliers, rebuilt and loaded W bit-identical: {_bit_equal(a, old)}")
    util.assert_ba_equal(a, old, rel=1e-9, abs_state=1e-9)
    util.assert_ba_equal(a, ro, rel=1e-6)
    assert _bit_equal(a, a2)


def _two_computes_subprocess(case, env=None):
    """Compute() twice on one bundle, in a process of its own -> the result dicts of the two calls"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tempfile.mktemp(suffix=".pkl")
    code = ("import sys, pickle; sys.path.insert(0, %r)\n"
            "from ptam_cg_amd._lib import load\nfrom tests import test_gpu_update_recompute as t\n"
            "pickle.dump(t._two_computes(load(), %r), open(%r, 'wb'))\n") % (root, case, out)
    e = dict(os.environ)
    e.update(env or {})
    subprocess.run([sys.executable, "-c", code], env=e, cwd=root, check=True, timeout=600)
    with open(out, "rb") as f:
        res = pickle.load(f)
    os.unlink(out)
    return res


def _two_computes(lib, case):
    from ptam_cg_amd import host
    ctx = host.Context(lib=lib)
    ba = synth.load_into(host.Bundle(ctx, deterministic=1), synth.make_ba_problem(**case))
    res = []
    for _ in range(2):
        acc = ba.Compute()
        poses, pts = ba.get_all()
        res.append({"accepted": acc, "converged": ba.Converged(), "trials": ba.trials().copy(), "poses": poses, "points": pts,
                    "outliers": ba.GetOutlierMeasurements().copy(), "solve_fallbacks": ba.solve_fallbacks()})
    ba.close()
    ctx.close()
    return res


def test_second_compute_after_a_purge(oracle, monkeypatch):
    """a second Compute() on the bundle whose first one purged its outliers: the purged measurements are MS_DEAD, K10 must leave
    them out of the rebuilt sums as it left their zero blocks out"""
    monkeypatch.delenv(SWITCH, raising=False)
    a = _two_computes_subprocess(CAMS20)
    old = _two_computes_subprocess(CAMS20, env={SWITCH: "1"})
    ro = _two_computes(oracle, CAMS20)
    assert len(ro[0]["outliers"]) > 100   # (a purge worth the name)
    for i in range(2):
        assert a[i]["solve_fallbacks"] == 0 and old[i]["solve_fallbacks"] == 0
        print(f"Compute {i + 1}: {len(a[i]['trials'])} trials, rebuilt and loaded W bit-identical: {_bit_equal(a[i], old[i])}")
        util.assert_ba_equal(a[i], old[i], rel=1e-9, abs_state=1e-9)
        util.assert_ba_equal(a[i], ro[i], rel=1e-6)
    assert len(a[1]["trials"]) > 0
