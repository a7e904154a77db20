"""The camera solve alone (csrc/solve.hip), in every form ba_solve can choose, against an exact answer and an extended-precision
reference: ptam_ba_debug_solve runs ONE solve of a supplied system on a prepared bundle's own buffers.  One row of
tests/solve_ref.py's table per case: a bundle whose prepared counts give that (block rows, block band), then
  - the plan that ran is the table's;
  - class E (integer systems, exact in every summation order): da == x and |da|^2 == |x|^2 to the last bit, persistent and
    per-column forms, with and without NaN in the never-read upper triangles, a second system and the first one again;
  - classes W and I: error and residual against the longdouble reference at most 10 x the oracle's plain-double LDL^T (the
    project's referee rule: not the outlier), or 10 n 2^-53 where the oracle is better than that;
  - the trial poses exp(da) * pose and |da|^2 the same launch writes, from the DEVICE's da.
tests/test_solve_plan.py checks the table and the systems' preconditions without a GPU."""

import numpy as np
import pytest

from ptam_cg_amd import host, synth
from ptam_cg_amd._abi import BL_COUNTS
from tests import solve_ref as R
from tests import util

pytestmark = pytest.mark.gpu
ROWS = [pytest.param(r, id=R.row_id(r)) for r in R.TABLE]


def covisibility_problem(n_free, band):
    """cameras on synth's arc, camera 0 fixed and — from 20 free cameras on — a fixed one behind every 9th free one; one point per
    free camera f, seen by f, by the LAST free camera whose rows still lie within `band` blocks of f's, and by camera 0: the block
    bandwidth of the camera system is exactly `band`"""
    fixed = [1]
    for f in range(n_free):
        fixed.append(0)
        if n_free >= 20 and f % 9 == 8:
            fixed.append(1)
    fixed = np.array(fixed, dtype=np.uint8)
    n_cams = len(fixed)
    cam_of = np.flatnonzero(fixed == 0)
    rng = np.random.default_rng(7 * n_free + band)
    cam = synth.AtanCam(synth.DEFAULT_CAMERA, (640, 480))
    ang = np.linspace(-np.pi / 3, np.pi / 3, n_cams)
    poses = np.stack([synth.look_at([2 * np.sin(a), -2 * np.cos(a), 1.0], [0, 0, 0]) for a in ang])
    pts = np.column_stack([rng.uniform(-0.3, 0.3, n_free), rng.uniform(-0.3, 0.3, n_free), rng.uniform(-0.1, 0.1, n_free)])
    cam_idx, pt_idx = [], []
    for f in range(n_free):
        g = f
        while g + 1 < n_free and (6 * (g + 1) + 5) // R.NB - (6 * f) // R.NB <= band:
            g += 1
        for c in sorted({0, int(cam_of[f]), int(cam_of[g])}):
            cam_idx.append(c)
            pt_idx.append(f)
    cam_idx, pt_idx = np.array(cam_idx, dtype=np.int32), np.array(pt_idx, dtype=np.int32)
    order = np.lexsort((pt_idx, cam_idx))   # keyframe order, then point order
    cam_idx, pt_idx = cam_idx[order], pt_idx[order]
    found = np.zeros((len(cam_idx), 2))
    for c in range(n_cams):
        sel = cam_idx == c
        found[sel] = cam.visible(poses[c], pts)[1][pt_idx[sel]]
    return {"poses": poses.reshape(n_cams, 12), "fixed": fixed, "points": pts, "cam_idx": cam_idx, "pt_idx": pt_idx, "found": found,
            "sigma_sq": np.ones(len(cam_idx))}


class Solver:
    def __init__(self, hip, oracle, row):
        self.nblk, self.band, self.n_free = row[:3]
        self.want = {0: row[3], R.PER_COLUMN: row[4]}
        self.oracle = oracle
        self.prob = covisibility_problem(self.n_free, self.band)
        self.ctx = host.Context(lib=hip)
        self.ba = synth.load_into(host.Bundle(self.ctx), self.prob)
        self.ba.prepare()
        counts = self.ba.debug_lists(BL_COUNTS, np.int32)
        assert counts[0] == len(self.prob["fixed"]) and counts[1] == self.n_free and counts[4] == self.band, counts[:5]
        self.n = 6 * self.n_free
        self.plan = hip.ba_solve_plan

    def close(self):
        self.ba.close()
        self.ctx.close()

    def solve(self, system, flags):
        """one solve; the plan, the trial poses and |da|^2 are checked on every one"""
        da, sumsq, poses, plan = self.ba.debug_solve(system["S"], system["E"], flags)
        form = flags & R.PER_COLUMN
        assert plan == self.want[form] == self.plan(self.nblk, self.band, form), (R.plan_names(plan), R.plan_names(self.want[form]))
        assert np.all(np.isfinite(da)) and np.all(np.isfinite(poses)) and np.isfinite(sumsq)
        pin, fixed = self.prob["poses"], self.prob["fixed"]
        scale = float(np.max(np.abs(pin)))
        worst, f = 0.0, 0
        for c in range(len(fixed)):
            if fixed[c]:
                assert np.array_equal(poses[c], pin[c]), c   # a fixed camera's trial pose is its pose
                continue
            mu = np.ascontiguousarray(da[6 * f:6 * f + 6])
            ex, want = np.zeros(12), np.zeros(12)
            self.oracle.lib.ptamo_se3_exp(mu.ctypes.data, ex.ctypes.data)
            self.oracle.lib.ptamo_se3_mul(ex.ctypes.data, np.ascontiguousarray(pin[c]).ctypes.data, want.ctypes.data)
            worst = max(worst, float(np.max(np.abs(poses[c] - want))))
            f += 1
        assert f == self.n_free
        # a dozen dependent double operations on magnitudes of 1 to 10: 1e-12 is a thousandfold margin
        assert worst <= 1e-12 * scale, (worst, scale)
        ss = float(np.sum(da.astype(R.LD) ** 2))   # rows < n only: a padding row must not count
        assert abs(sumsq - ss) <= self.n * 2.0 ** -52 * ss, (sumsq, ss)
        return da, sumsq, poses


@pytest.fixture
def solver(hip, oracle, request):
    s = Solver(hip, oracle, request.param)
    yield s
    s.close()


@pytest.mark.parametrize("solver", ROWS, indirect=True)
def test_class_e_every_form_returns_x_bit_for_bit(solver):
    e1, e2 = R.class_e(solver.n_free, solver.band, 1), R.class_e(solver.n_free, solver.band, 2)
    assert not np.array_equal(e1["x"], e2["x"])
    for form in (0, R.PER_COLUMN):
        first = None
        for system, flags in ((e1, form), (e1, form | R.POISON_UPPER), (e2, form | R.POISON_UPPER), (e2, form), (e1, form)):
            da, sumsq, poses = solver.solve(system, flags)
            bad = np.flatnonzero(da != system["x"])
            assert len(bad) == 0, (R.plan_names(solver.want[form]), flags, len(bad), bad[:8], da[bad[:8]], system["x"][bad[:8]])
            assert sumsq == system["sumsq"], (sumsq, system["sumsq"])
            if first is None:
                first = (da, sumsq, poses)
        # (the last solve repeats the first: no sequence number, flag or stale vector of the solves between them leaks)
        assert np.array_equal(da, first[0]) and sumsq == first[1] and np.array_equal(poses, first[2])


@pytest.mark.parametrize("solver", ROWS, indirect=True)
def test_classes_w_and_i_no_worse_than_ten_times_the_oracle(solver):
    n = solver.n
    floor = n * 2.0 ** -53
    failures = []
    for name, make in (("W", R.class_w), ("I", R.class_i)):
        s = make(solver.n_free, solver.band, 3 if name == "W" else 4)
        x_ref = R.BandLDLT(s["S"], s["band"]).solve(s["E"])
        err_o, res_o = R.err_and_residual(s["S"], s["E"], s["band"], R.oracle_solve(solver.oracle, s["S"], s["E"]), x_ref)
        for form in (0, R.PER_COLUMN):
            a = solver.solve(s, form | R.POISON_UPPER)
            b = solver.solve(s, form | R.POISON_UPPER)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])   # two identical calls, identical bits
            err_d, res_d = R.err_and_residual(s["S"], s["E"], s["band"], a[0], x_ref)
            r_err, r_res = err_d / max(err_o, floor), res_d / max(res_o, floor)
            print("SOLVE_DIRECT %s class %s form %s: err device %.3e oracle %.3e ratio %.3f | res device %.3e oracle %.3e ratio %.3f"
                  % (R.row_id((solver.nblk, solver.band, solver.n_free)), name, R.plan_names(solver.want[form]), err_d, err_o, r_err,
                     res_d, res_o, r_res))
            if r_err > 10 or r_res > 10:
                failures.append((name, R.plan_names(solver.want[form]), err_d, err_o, res_d, res_o))
    assert not failures, failures


def test_compute_after_the_hook_equals_compute_without_it(hip, oracle):
    """the bundle stays usable: deterministic mode, the same bits with and without solves of foreign systems (both forms, NaN in
    the upper triangles) between prepare and Compute()"""
    case = dict(n_cams=14, n_pts=200, seed=131)   # 13 free cameras: 3 block rows, the smallest persistent launch
    prob = synth.make_ba_problem(**case)
    plain = util.run_ba(hip, prob, deterministic=1)
    ctx = host.Context(lib=hip)
    ba = synth.load_into(host.Bundle(ctx, deterministic=1), prob)
    ba.prepare()
    for seed, flags in ((3, R.POISON_UPPER), (5, R.PER_COLUMN | R.POISON_UPPER), (6, 0)):
        s = R.class_w(13, 2, seed)
        da = ba.debug_solve(s["S"], s["E"], flags)[0]
        assert np.all(np.isfinite(da))
    acc = ba.Compute()
    poses, pts = ba.get_all()
    trials = ba.trials()
    assert acc == plain["accepted"] and acc > 0 and ba.solve_fallbacks() == 0
    for k in trials.dtype.names:
        assert np.array_equal(trials[k], plain["trials"][k], equal_nan=True), k
    assert np.array_equal(poses, plain["poses"]) and np.array_equal(pts, plain["points"])
    assert np.array_equal(ba.GetOutlierMeasurements(), plain["outliers"])
    ba.close()
    ctx.close()
