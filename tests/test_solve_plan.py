"""CPU: which form of the camera solve runs for which system (csrc/solve.hip: ptam_ba_solve_plan, the function ba_solve takes its
decisions from) against the hand-derived table of tests/solve_ref.py, and the preconditions of the test systems that
tests/test_gpu_solve_direct.py feeds to every one of those forms."""
import ctypes
import os

import numpy as np
import pytest

from tests import solve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
SWITCHES = ("PTAM_LDLT_SEPARATE_BACKWARD", "PTAM_LDLT_BACKWARD_IN_LAUNCH", "PTAM_LDLT_NO_CHAIN", "PTAM_LDLT_ONE_ENDED",
            "PTAM_LDLT_NO_SMALL", "PTAM_LDLT_TWIN_LAUNCHES")
ROWS = [pytest.param(r, id=R.row_id(r)) for r in R.TABLE]


@pytest.fixture(scope="module")
def plan():
    for k in SWITCHES:   # (the library reads them once per process, at the first plan)
        assert k not in os.environ, k
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    lib.ptam_ba_solve_plan.restype = ctypes.c_int
    lib.ptam_ba_solve_plan.argtypes = [ctypes.c_int] * 3
    return lib.ptam_ba_solve_plan


@pytest.mark.parametrize("row", ROWS)
def test_plan_equals_the_table(plan, row):
    nblk, band, n_free, want, want_per_column = row
    assert R.nblk_of(n_free) == nblk and band <= nblk - 1
    got, got_pc = plan(nblk, band, 0), plan(nblk, band, R.PER_COLUMN)
    assert got == want, (R.plan_names(got), R.plan_names(want))
    assert got_pc == want_per_column, (R.plan_names(got_pc), R.plan_names(want_per_column))
    # flags bit 0: nothing persistent
    assert got_pc & (R.CHAIN_FWD_INV | R.CHAIN_BW_IN_LAUNCH | R.CHAIN_SEPARATE_BW | R.TWO_CHAINS | R.MID_CHAIN) == 0
    assert bool(got_pc & R.SMALL) + bool(got_pc & R.STEPS) + bool(got_pc & R.TWIN_STEPS) == 1
    assert got_pc & R.SMALL or nblk > 2
    # the elimination order the exact test systems are built for (solve_ref.twist_len) is the plan's
    assert (R.twist_len(nblk, band) > 0) == bool(got & R.BW_TWO_WG) == bool(got_pc & R.BW_TWO_WG)
    # a band wider than the system is the dense system
    assert plan(nblk, nblk + 40, 0) == plan(nblk, nblk - 1, 0)


def test_plan_refuses_nonsense(plan):
    assert plan(0, 0, 0) < 0 and plan(3, -1, 0) < 0 and plan(-2, 0, 1) < 0


def test_table_reaches_every_bit():
    seen = 0
    for row in R.TABLE:
        seen |= row[3] | row[4]
    assert seen == (1 << len(R.BIT_NAMES)) - 1, R.plan_names(((1 << len(R.BIT_NAMES)) - 1) & ~seen)


# threshold -> (nblk, band) below / at it, (nblk, band) beyond it, the bit the first has and the second has not, the bit the second has instead
THRESHOLDS = {
    "SM_USE_NB = 2": ((2, 1), (3, 2), R.SMALL, R.CHAIN_FWD_INV),
    "CH_FI_MAX_NB = 13": ((13, 3), (14, 4), R.CHAIN_FWD_INV, R.CHAIN_BW_IN_LAUNCH),
    "13 tiles of LDS, forward-inverse": ((13, 12), (14, 13), R.CHAIN_FWD_INV, R.STEPS),
    "nblk >= 2 band + 8": ((13, 3), (14, 3), R.CHAIN_FWD_INV, R.TWO_CHAINS),
    "CH_BW_MAXT = 9": ((25, 9), (24, 10), R.CHAIN_BW_IN_LAUNCH, R.CHAIN_SEPARATE_BW),
    "13 tiles of LDS, one chain": ((28, 12), (28, 13), R.CHAIN_SEPARATE_BW, R.STEPS),
    "CH_MAX_NB = 28, one chain": ((28, 12), (29, 11), R.CHAIN_SEPARATE_BW, R.STEPS),
    "13 tiles of LDS, two chains": ((32, 12), (34, 13), R.TWO_CHAINS, R.TWIN_STEPS),
    "13 tiles of LDS, the middle": ((32, 12), (34, 13), R.MID_CHAIN, R.MID_STEPS),
    "CH_MAX_NB = 28, rows of each of two chains": ((56, 2), (58, 2), R.TWO_CHAINS, R.TWIN_STEPS),
    "a middle of 3 blocks": ((11, 1), (10, 1), R.MID_CHAIN, R.MID_STEPS),
    "BW_LDS_MAX: npad > 3200": ((100, 2), (101, 2), 0, R.BW_GLOBAL),
}


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_every_threshold_is_bracketed_by_the_table(plan, name):
    a, b, bit_a, bit_b = THRESHOLDS[name]
    tabled = {(r[0], r[1]): r[3] for r in R.TABLE}
    assert a in tabled and b in tabled
    for want, got in ((tabled[a], plan(*a, 0)), (tabled[b], plan(*b, 0))):
        assert want == got
    pa, pb = tabled[a], tabled[b]
    assert pa & bit_a == bit_a and pb & bit_a == 0
    assert pb & bit_b == bit_b and pa & bit_b == 0


def elimination_rank(n, nblk, band):
    """position of every row in the solve's elimination order: the downward chain's, the upward chain's (bottom first), the middle"""
    t = R.twist_len(nblk, band)
    bot = (nblk - t) * R.NB
    order = list(range(min(t * R.NB, n))) + [i for i in range(n - 1, bot - 1, -1)] + list(range(t * R.NB, min(bot, n)))
    assert sorted(order) == list(range(n))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return rank, order


@pytest.mark.parametrize("row", ROWS)
def test_class_e_is_exact_in_every_form(row):
    """the stated precondition, in Python integers: every partial sum any summation order can meet stays below 2^53; M is unit
    lower triangular in the elimination order of this (nblk, band), so the pivots are D's powers of two and the multipliers M's
    integers; every in-band tile carries entries"""
    nblk, band, n_free = row[:3]
    for seed in (1, 2):   # (the two systems the GPU test solves)
        s = R.class_e(n_free, band, seed)
        n = s["n"]
        assert s["bound"] < 2 ** 53 // 4096, s["bound"]   # (with three decimal digits in hand)
        assert np.array_equal(s["S"], np.round(s["S"])) and np.array_equal(s["E"], np.array(s["E_int"], dtype=np.float64))
        assert np.array_equal(np.triu(s["S"], 1), np.zeros((n, n)))
        rank, order = elimination_rank(n, nblk, s["band"])
        tiles = set()
        for (i, j) in s["ent"]:
            assert rank[i] > rank[j] and abs(i // R.NB - j // R.NB) <= s["band"]
            tiles.add((max(i, j) // R.NB, min(i, j) // R.NB))
        want_tiles = {(bi, bj) for bi in range(nblk) for bj in range(max(0, bi - s["band"]), bi + 1)}
        assert want_tiles <= tiles, sorted(want_tiles - tiles)
        assert all(d > 0 and d & (d - 1) == 0 for d in s["D"])
        if nblk <= 13 and s["twist"] == 0:   # the forward-inverse form also builds M^-1
            assert R.class_e_inverse_bound(s) < 2 ** 53 // 4096
        # S x = E exactly, and (where that is cheap) plain double elimination in the solve's order meets D and x exactly
        assert np.array_equal(R.band_matvec(s["S"], s["x"], s["band"]), s["E"].astype(R.LD))
        if n <= 450:
            A = s["S"] + np.tril(s["S"], -1).T
            A = A[np.ix_(order, order)]
            z = s["E"][order].copy()
            piv = np.zeros(n)
            for k in range(n):
                piv[k] = A[k, k]
                l = A[k + 1:, k] / piv[k]
                A[k + 1:, k + 1:] -= np.outer(l, A[k, k + 1:])
                z[k + 1:] -= l * z[k]
                A[k + 1:, k] = l
            xs = z / piv
            for k in range(n - 1, -1, -1):
                xs[k] -= A[k + 1:, k] @ xs[k + 1:]
            assert np.array_equal(piv, np.array(s["D"], dtype=np.float64)[order])
            assert np.array_equal(xs, s["x"][order])


@pytest.mark.parametrize("row", ROWS)
def test_class_w_is_well_conditioned_and_not_diagonally_dominant(row):
    nblk, band, n_free = row[:3]
    s = R.class_w(n_free, band, 3)
    S, n = s["S"], s["n"]
    assert s["cond_bound"] < 1e4   # lambda_max <= |S|_inf, lambda_min >= the shift: see solve_ref
    assert np.array_equal(np.triu(S, 1), np.zeros((n, n)))
    i, k = np.nonzero(S)
    assert np.all(np.abs(i // R.NB - k // R.NB) <= s["band"])
    if n > 6:
        off = np.abs(S).sum(axis=1) + np.abs(S).sum(axis=0) - 2 * np.abs(np.diagonal(S))
        assert np.all(off > np.diagonal(S)), float((off / np.diagonal(S)).min())
    if n <= 450:
        R.BandLDLT(S, s["band"])   # (asserts its pivots positive; the larger shapes' are factored by the GPU test)


@pytest.mark.parametrize("row", ROWS)
def test_class_i_is_hard_but_not_hopeless_for_plain_double(oracle, row):
    """the oracle's plain-double LDL^T lands between 1e-12 and 1e-4 relative of the extended-precision reference: the comparison of
    tests/test_gpu_solve_direct.py against it is neither vacuous nor hopeless.  (The two rows of 3 200 rows are the slow ones: the
    oracle's LDL^T is dense, a third of n^3 strided operations whatever the band.)"""
    nblk, band, n_free = row[:3]
    s = R.class_i(n_free, band, 4)
    x_ref = R.BandLDLT(s["S"], s["band"]).solve(s["E"])
    err, res = R.err_and_residual(s["S"], s["E"], s["band"], R.oracle_solve(oracle, s["S"], s["E"]), x_ref)
    print("class I %s: oracle err %.3e res %.3e" % (R.row_id(row), err, res))
    assert 1e-12 <= err <= 1e-4, err
    assert float(np.max(np.abs(x_ref))) < 100   # (the trial poses exp(da) pose of the GPU test stay of order 1 to 10)
