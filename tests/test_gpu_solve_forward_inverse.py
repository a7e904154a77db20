"""The camera solve's forward-inverse form (csrc/ldlt_chain.inc, column workers): up to 13 block rows the persistent launch
builds L^-1 beside the factorisation and x = L^-T D^-1 z is a sum of products — no backward substitution.  Against the two
forms it replaces (the backward pass inside the launch, ldlt_backward_kernel behind it) and against the oracle, at the
smallest shapes at which it can go wrong."""
import threading

import numpy as np
import pytest

from ptam_cg_amd import synth
from tests import util

pytestmark = pytest.mark.gpu

# free cameras (+ 1 fixed) -> rows -> blocks of 32.  No covisibility window: every point is seen by every camera, the camera
# system is dense (band = blocks - 1 < 2 band + 8: one chain over the whole system), 3 .. 13 block rows — what ba_solve
# (csrc/solve.hip: ldlt_forward_inverse) gives to the forward-inverse form
SHAPES = {
    "13_cams_3_blocks_last_padded": dict(n_cams=14, n_pts=200, seed=131),      # 78 rows: the smallest persistent launch
    "16_cams_3_blocks_full": dict(n_cams=17, n_pts=200, seed=161),             # 96 rows: no identity padding at all
    "17_cams_4_blocks_last_6_rows": dict(n_cams=18, n_pts=200, seed=171),      # 102 rows: niter = 2 in the last block, a camera straddles every block boundary
    "49_cams_10_blocks": dict(n_cams=50, n_pts=300, seed=491),                 # 294 rows: the headline's role count without its run time
    "19_cams_4_blocks": dict(n_cams=20, n_pts=300, seed=191),                  # 114 rows: the local bundle's shape
    "69_cams_13_blocks": dict(n_cams=70, n_pts=300, seed=691),                 # 414 rows: the form's last size, 13 tiles fill a column worker's LDS
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_forward_inverse_solve_against_both_backward_forms_and_the_oracle(oracle, shape, monkeypatch):
    """the default (forward-inverse) form against PTAM_LDLT_SEPARATE_BACKWARD=1 and against PTAM_LDLT_BACKWARD_IN_LAUNCH=1: the
    same discrete trajectory, every trial's numbers and the state to 1e-9 (the bounds of
    test_backward_substitution_inside_the_launch_equals_the_separate_kernel); against the oracle at the suite's 1e-6; no wait
    gave up; deterministic mode repeats to the last bit.  (The switches are read once per process: every run is a process of
    its own, the default form's with every switch of the solve taken out of the environment.)"""
    for k in ("PTAM_LDLT_SEPARATE_BACKWARD", "PTAM_LDLT_BACKWARD_IN_LAUNCH", "PTAM_LDLT_NO_CHAIN", "PTAM_CH_SPIN_LIMIT"):
        monkeypatch.delenv(k, raising=False)
    case = SHAPES[shape]
    assert "window" not in case   # (dense: see SHAPES)
    n_free = case["n_cams"] - 1
    assert 3 <= (6 * n_free + 31) // 32 <= 13   # (the range of the form)
    det = dict(deterministic=1)
    prob = synth.make_ba_problem(**case)
    a = util.run_ba_subprocess(case, opts=det)
    a2 = util.run_ba_subprocess(case, opts=det)
    sep = util.run_ba_subprocess(case, env={"PTAM_LDLT_SEPARATE_BACKWARD": "1"}, opts=det)
    inl = util.run_ba_subprocess(case, env={"PTAM_LDLT_BACKWARD_IN_LAUNCH": "1"}, opts=det)
    ro = util.run_ba(oracle, prob)
    assert len(a["trials"]) > 0 and a["accepted"] > 0
    for r in (a, a2, sep, inl):
        assert r["solve_fallbacks"] == 0
    util.assert_ba_equal(a, sep, rel=1e-9, abs_state=1e-9)
    util.assert_ba_equal(a, inl, rel=1e-9, abs_state=1e-9)
    util.assert_ba_equal(a, ro, rel=1e-6)
    for k in a["trials"].dtype.names:
        assert np.array_equal(a["trials"][k], a2["trials"][k], equal_nan=True), k
    assert np.array_equal(a["poses"], a2["poses"]) and np.array_equal(a["points"], a2["points"])


def test_two_bundles_with_forward_inverse_solves_side_by_side(hip):
    """after test_two_bundles_with_persistent_solves_side_by_side: the form doubles the launch's working workgroups (20 at 49
    free cameras).  Two bundles adjusting at the same moment: each finds its XCD or repeats the trial per block column — both
    outcomes are right; both must finish with the results they have alone."""
    probs = [synth.make_ba_problem(n_cams=50, n_pts=300, seed=491), synth.make_ba_problem(n_cams=50, n_pts=300, seed=492)]
    alone = [util.run_ba(hip, p, max_iterations=6) for p in probs]
    got = {}

    def work(i):
        got[i] = [util.run_ba(hip, probs[i], max_iterations=6) for _ in range(4)]

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert all(not t.is_alive() for t in th)
    for i in range(2):
        assert len(got[i]) == 4
        for r in got[i]:
            util.assert_ba_equal(r, alone[i], rel=1e-8, abs_state=1e-8)
