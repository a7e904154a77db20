"""-m gpu: bench.py's plain run on one GPU: one JSON line from the headline alone, exactly --steps timed trials, and
--dump-outputs holding what that timed Compute() returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ptam_cg_amd import synth
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_what_the_timed_compute_returned(hip, tmp_path):
    steps = 1000   # (far past convergence: lambda may overflow at the noise floor, the dumped state must stay finite)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cams", "24", "--points", "900", "--steps", str(steps),
           "--warmup", "1", "--deterministic", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == steps and rec["full"] is False and rec["ms_per_step"] > 0
    assert abs(rec["value"] * rec["ms_per_step"] - 1e3) <= 1e-9 * 1e3
    assert sum(rec["trial_mix"].values()) == steps
    assert not {"roofline", "kernel_ms_per_trial", "tracking", "cpu_baseline", "local_ba_config4"} & set(rec)   # --full's legs
    # deterministic mode: the same problem through the library in this process, to the last bit
    ref = util.run_ba(hip, synth.make_ba_problem(24, 900, synth.SEED_BA_HEADLINE), max_iterations=steps, update_sq_conv_limit=0.0,
                      deterministic=1)
    got = {k: np.load(tmp_path / f"{k}.npy") for k in ("cameras", "points", "outliers")}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["cameras"], ref["poses"]) and np.array_equal(got["points"], ref["points"])
    ol = ref["outliers"].astype(np.float64).reshape(-1, 2)
    assert np.array_equal(got["outliers"], ol[np.lexsort((ol[:, 1], ol[:, 0]))])
