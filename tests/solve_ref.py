"""The camera solve S da = E alone (csrc/solve.hip): the table of its forms, three classes of test systems and an
extended-precision reference.  numpy only; shared by tests/test_solve_plan.py (CPU) and tests/test_gpu_solve_direct.py.

The system is block-banded with 32x32 blocks: element (i, k) may be non-zero only if |i // 32 - k // 32| <= band.

Class E (exact): S = M D M^T with M unit "lower triangular in the solve's elimination order", small integer entries in every
    in-band tile, D powers of two, x small integers, E = S x in integer arithmetic.  Every pivot any form meets is then a power of
    two, every multiplier an entry of M, every Schur complement, partial sum and substituted vector an integer far below 2^53 —
    whatever the order of summation.  Every form must return x and |x|^2 bit for bit.
    (The elimination order is not always top-down: a system with nblk >= 2 band + 8 is eliminated from BOTH ends, twist_len
    below.  M follows that order — columns of the upward chain hold their entries ABOVE the diagonal — otherwise the upward chain's
    first pivot would be an arbitrary integer and its multipliers fractions.)
Class W (well conditioned): S = B B^T + s I with B block-lower-banded, uniform in (-1, 1): the product of such a B with its
    transpose lies inside the block band by itself (restricting it to the band is a no-op, so it stays positive semi-definite),
    lambda_min >= s, lambda_max <= |S|_inf, and with s = |B B^T|_inf / 500 the condition number is below 501 < 1e4 by
    construction.  Far from diagonally dominant: the off-diagonal row sums are several times the diagonal.
Class I (ill conditioned, as a lightly damped bundle's S): S = L0 D0 L0^T, L0 unit lower with real entries of order 1, D0
    log-uniform over eight decades.
"""
import numpy as np

from ptam_cg_amd import _abi

NB = 32
LD = np.longdouble

# ---- the plan bits (include/ptam_hip_bench.h) -----------------------------------------------------------------------------------
BIT_NAMES = ["SMALL", "CHAIN_FWD_INV", "CHAIN_BW_IN_LAUNCH", "CHAIN_SEPARATE_BW", "STEPS", "TWO_CHAINS", "TWIN_STEPS", "MID_CHAIN",
             "MID_STEPS", "BW_TWO_WG", "BW_GLOBAL"]
SMALL, CHAIN_FWD_INV, CHAIN_BW_IN_LAUNCH, CHAIN_SEPARATE_BW, STEPS, TWO_CHAINS, TWIN_STEPS, MID_CHAIN, MID_STEPS, BW_TWO_WG, BW_GLOBAL = (
    getattr(_abi, "SP_" + n) for n in BIT_NAMES)
PER_COLUMN, POISON_UPPER = _abi.SOLVE_PER_COLUMN, _abi.SOLVE_POISON_UPPER   # flags of ptam_ba_solve_plan / ptam_ba_debug_solve


def plan_names(mask):
    return "|".join(n for n in BIT_NAMES if mask & getattr(_abi, "SP_" + n)) or "0"


# (nblk, band) -> free cameras, the whole mask ba_solve must choose (persistent forms allowed), and with flags bit 0.
# Derived by hand from csrc/solve.hip and the sizes in csrc/ldlt_chain.inc: a CU's 160 KB of LDS hold 13 tiles beside ChainLds.
TABLE = [
    # nblk band  F    persistent                                  per column
    (1, 0, 1, SMALL, SMALL),
    (1, 0, 5, SMALL, SMALL),
    (2, 1, 10, SMALL, SMALL),
    (3, 2, 11, CHAIN_FWD_INV, STEPS),                                           # 2 real rows in the last block
    (13, 12, 65, CHAIN_FWD_INV, STEPS),                                         # the LDS limit; 6 real rows in the last block
    (13, 12, 69, CHAIN_FWD_INV, STEPS),                                         # ... 30
    (13, 3, 67, CHAIN_FWD_INV, STEPS),                                          # banded
    (14, 3, 72, TWO_CHAINS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),   # nblk = 2 band + 8
    (14, 13, 70, STEPS, STEPS),                                                 # dense, 14 tiles: nothing persistent fits
    (14, 4, 72, CHAIN_BW_IN_LAUNCH, STEPS),
    (25, 9, 131, CHAIN_BW_IN_LAUNCH, STEPS),                                    # band = CH_BW_MAXT, nblk = 2 band + 7
    (24, 10, 126, CHAIN_SEPARATE_BW, STEPS),
    (28, 12, 147, CHAIN_SEPARATE_BW, STEPS),                                    # CH_MAX_NB rows of 13 tiles
    (29, 11, 152, STEPS, STEPS),
    (28, 13, 147, STEPS, STEPS),
    (10, 1, 52, TWO_CHAINS | MID_STEPS | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),    # a middle of 2 blocks
    (11, 1, 57, TWO_CHAINS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),
    (32, 12, 168, TWO_CHAINS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),
    (34, 13, 179, TWIN_STEPS | MID_STEPS | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),  # 14 tiles per row
    (56, 2, 296, TWO_CHAINS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),   # each chain's rows = CH_MAX_NB
    (58, 2, 307, TWIN_STEPS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),   # ... + 1
    (100, 2, 533, TWIN_STEPS | MID_CHAIN | BW_TWO_WG, TWIN_STEPS | MID_STEPS | BW_TWO_WG),  # npad = 3200: the vectors' last fit in LDS
    (101, 2, 534, TWIN_STEPS | MID_CHAIN | BW_TWO_WG | BW_GLOBAL, TWIN_STEPS | MID_STEPS | BW_TWO_WG | BW_GLOBAL),
]


def row_id(row):
    return "nblk%d_band%d_F%d" % row[:3]


def nblk_of(n_free):
    return (6 * n_free + NB - 1) // NB


def twist_len(nblk, band):
    """block columns each end of a two-ended elimination takes (csrc/solve.hip: ldlt_twist_len); 0: top-down"""
    return 0 if band < 1 or nblk < 2 * band + 8 else (nblk - 2 * band) // 2


# ---- the extended-precision reference -------------------------------------------------------------------------------------------
def half_width(n, band):
    """largest |i - k| of an in-band element"""
    return min(n - 1, NB * band + NB - 1)


class BandLDLT:
    """unpivoted LDL^T of the banded S (dense n x n, lower triangle read) and both substitutions, in np.longdouble"""

    def __init__(self, S, band):
        n = S.shape[0]
        w = half_width(n, band)
        W = 2 * w + 1
        ab = np.zeros((n + 1) * W, dtype=LD)   # ab[i * W + k] = S[i, i - w + k]: the whole symmetric band, so that a trailing
        A = ab[:n * W].reshape(n, W)           # window [j+1, j+1+m)^2 is ONE strided view (row stride W - 1)
        for k in range(0, w + 1):
            dg = np.diagonal(S, -k).astype(LD)
            A[k:, w - k] = dg
            A[:n - k, w + k] = dg
        self.n, self.w = n, w
        self.d = np.zeros(n, dtype=LD)
        self.Lc = np.zeros((n, w), dtype=LD)   # Lc[j, a] = L[j + 1 + a, j]
        es = ab.itemsize
        for j in range(n):
            d = A[j, w]
            assert d > 0, ("pivot", j, float(d))
            self.d[j] = d
            m = min(w, n - 1 - j)
            if m == 0:
                continue
            col = A[j, w + 1:w + 1 + m].copy()   # row j right of the diagonal = column j below it
            l = col / d
            self.Lc[j, :m] = l
            win = np.lib.stride_tricks.as_strided(ab[(j + 1) * W + w:], shape=(m, m), strides=((W - 1) * es, es))
            win -= np.outer(l, col)

    def solve(self, b):
        n, w = self.n, self.w
        y = np.array(b, dtype=LD)
        for j in range(n):
            m = min(w, n - 1 - j)
            if m:
                y[j + 1:j + 1 + m] -= self.Lc[j, :m] * y[j]
        x = y / self.d
        for j in range(n - 1, -1, -1):
            m = min(w, n - 1 - j)
            if m:
                x[j] -= np.dot(self.Lc[j, :m], x[j + 1:j + 1 + m])
        return x


def band_matvec(S, x, band):
    """S x with the symmetric banded S given by its lower triangle, formed in longdouble"""
    n = S.shape[0]
    x = np.asarray(x, dtype=LD)
    r = np.diagonal(S).astype(LD) * x
    for k in range(1, half_width(n, band) + 1):
        dg = np.diagonal(S, -k).astype(LD)
        r[k:] += dg * x[:n - k]
        r[:n - k] += dg * x[k:]
    return r


def norm_inf(S, band):
    n = S.shape[0]
    r = np.abs(np.diagonal(S)).astype(np.float64)
    for k in range(1, half_width(n, band) + 1):
        dg = np.abs(np.diagonal(S, -k))
        r[k:] += dg
        r[:n - k] += dg
    return float(r.max())


def err_and_residual(S, E, band, da, x_ref):
    """err = max |da - x_ref| / max |x_ref|;  res = |S da - E|_inf / (|S|_inf |da|_inf + |E|_inf), the product in longdouble"""
    da = np.asarray(da, dtype=np.float64)
    if not np.all(np.isfinite(da)):
        return float("inf"), float("inf")
    err = float(np.max(np.abs(da.astype(LD) - x_ref)) / np.max(np.abs(x_ref)))
    r = band_matvec(S, da, band) - np.asarray(E, dtype=LD)
    res = float(np.max(np.abs(r)) / (LD(norm_inf(S, band)) * np.max(np.abs(da)) + np.max(np.abs(E))))
    return err, res


# ---- class E --------------------------------------------------------------------------------------------------------------------
LEVELS = 4       # an entry M[i, j] needs level(i) > level(j), level = (index in its block) % LEVELS: M - I is nilpotent of order LEVELS, so
PER_TILE = 40    # M^-1 = I - N + N^2 - N^3 has small integer entries as well (the forward-inverse form computes them)


def class_e(n_free, band, seed):
    """-> dict(S, E, x, sumsq, M entries (i, j, v), D) — S, E float64 holding exact integers"""
    n, nblk = 6 * n_free, nblk_of(n_free)
    band = min(band, nblk - 1)
    rng = np.random.default_rng(seed)
    t = twist_len(nblk, band)
    bot = (nblk - t) * NB   # t > 0: indices >= bot belong to the upward chain
    ent = {}

    def level(idx):   # (counted from the end each chain starts at, so that a thin last block of the upward chain gets entries too)
        return ((NB - 1 - idx % NB) if (t > 0 and idx >= bot) else idx % NB) % LEVELS

    for bi in range(nblk):
        for bj in range(max(0, bi - band), bi + 1):
            for _ in range(PER_TILE):
                r, c = int(rng.integers(0, min(NB, n - bi * NB))), int(rng.integers(0, min(NB, n - bj * NB)))
                p, q = bi * NB + r, bj * NB + c   # natural row > natural column
                if p <= q or p >= n:
                    continue
                # the pair's column is whichever of the two is eliminated FIRST: q, unless p belongs to the upward chain (then q
                # lies in that chain above p, or in the middle — the downward chain is out of the band's reach)
                i, j = (q, p) if (t > 0 and p >= bot) else (p, q)
                if level(i) <= level(j):
                    continue
                ent[(i, j)] = int(rng.choice([-2, -1, 1, 2], p=[0.1, 0.4, 0.4, 0.1]))
    D = [1 << int(k) for k in rng.integers(0, 7, n)]
    x = [int(v) for v in rng.choice([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], n)]
    cols = [[(j, 1)] for j in range(n)]   # column j of M: (row, value), the unit diagonal first
    for (i, j), v in ent.items():
        cols[j].append((i, v))
    Sd, Sabs = {}, {}
    for j in range(n):
        for (i, vi) in cols[j]:
            for (k, vk) in cols[j]:
                if k <= i:
                    Sd[(i, k)] = Sd.get((i, k), 0) + vi * D[j] * vk
                    Sabs[(i, k)] = Sabs.get((i, k), 0) + abs(vi) * D[j] * abs(vk)
    S = np.zeros((n, n))
    E, Eabs = [0] * n, [0] * n
    for (i, k), v in Sd.items():
        assert i // NB - k // NB <= band
        S[i, k] = v
        a = Sabs[(i, k)]
        E[i] += v * x[k]
        Eabs[i] += a * abs(x[k])
        if i != k:
            E[k] += v * x[i]
            Eabs[k] += a * abs(x[i])
    bound = max(max(Sabs.values()), max(Eabs))   # every partial sum of every Schur complement / substituted vector is below this
    return dict(S=S, E=np.array(E, dtype=np.float64), x=np.array(x, dtype=np.float64), sumsq=float(sum(v * v for v in x)),
                ent=ent, D=D, x_int=x, E_int=E, bound=bound, n=n, nblk=nblk, band=band, twist=t)


def class_e_inverse_bound(sys):
    """for the forward-inverse form (one-ended, nblk <= 13): the largest partial sum it can meet while it builds Y = M^-1 column
    block by column block and x = Y^T w, in Python integers"""
    n, ent, D, x = sys["n"], sys["ent"], sys["D"], sys["x_int"]
    assert sys["twist"] == 0
    rows = [[] for _ in range(n)]
    for (i, j), v in ent.items():
        assert i > j
        rows[i].append((j, v))
    Y = np.zeros((n, n), dtype=object)
    Yabs = np.zeros((n, n), dtype=object)
    for i in range(n):
        Y[i, i] = Yabs[i, i] = 1
        for (j, v) in rows[i]:
            Y[i, :] = Y[i, :] - v * Y[j, :]
            Yabs[i, :] = Yabs[i, :] + abs(v) * Yabs[j, :]
    w = [0] * n   # w = D^-1 z = M^T x
    for j in range(n):
        w[j] = x[j]
    for (i, j), v in ent.items():
        w[j] += v * x[i]
    wabs = np.array([abs(v) for v in w], dtype=object)
    # Y (M - I) Y-type products inside a block step are bounded by |Y| |M| |Y|; x_j = sum_m Y(m, j)^T w_m by |Y|^T |w|
    y_max = int(Yabs.max())
    m_row = max(1 + sum(abs(v) for _, v in r) for r in rows)
    y_row = int(max(Yabs[i, :].sum() for i in range(n)))
    return max(y_max * m_row * y_row, int((Yabs.T.dot(wabs)).max()), int(np.abs(Y).max()))


# ---- classes W and I ------------------------------------------------------------------------------------------------------------
def _tiles(nblk, band):
    return [(bi, bj) for bi in range(nblk) for bj in range(max(0, bi - band), bi + 1)]


def _dense_from_tiles(n, tiles):
    S = np.zeros((n, n))
    for (bi, bj), T in tiles.items():
        r0, c0 = bi * NB, bj * NB
        r1, c1 = min(n, r0 + NB), min(n, c0 + NB)
        S[r0:r1, c0:c1] = T[:r1 - r0, :c1 - c0]
    return np.tril(S)


def _banded_gram(nblk, band, Bt, Dt=None):
    """tiles (bi, bk), bk <= bi, of B diag(D) B^T for the block-lower-banded B given by its tiles"""
    out = {}
    for (bi, bk) in _tiles(nblk, band):
        acc = np.zeros((NB, NB))
        for bj in range(max(0, bi - band), bk + 1):
            left = Bt[(bi, bj)] if Dt is None else Bt[(bi, bj)] * Dt[bj][None, :]
            acc += left @ Bt[(bk, bj)].T
        out[(bi, bk)] = acc
    return out


def class_w(n_free, band, seed):
    n, nblk = 6 * n_free, nblk_of(n_free)
    band = min(band, nblk - 1)
    rng = np.random.default_rng(seed)
    Bt = {}
    for (bi, bj) in _tiles(nblk, band):
        T = rng.uniform(-1, 1, (NB, NB))
        T[max(0, n - bi * NB):, :] = 0   # rows / columns past n do not exist
        T[:, max(0, n - bj * NB):] = 0
        Bt[(bi, bj)] = T
    G = _dense_from_tiles(n, _banded_gram(nblk, band, Bt))
    g_inf = norm_inf(G, band)
    shift = g_inf / 500.0
    S = G + shift * np.eye(n)
    E = rng.uniform(-1, 1, n)
    return dict(S=S, E=E, n=n, nblk=nblk, band=band, shift=shift, cond_bound=(norm_inf(S, band)) / shift)


I_ROW = 1.5   # class I: off-diagonal entries of L0 per row, on average — uniform in (-1, 1), spread over the row's in-band tiles.
              # (A row's squared entries sum to ~0.5: with a sum above 1, |L0^-1| grows exponentially with n and no plain-double
              # solve, the oracle's included, has a digit left at 3 000 rows.)


def class_i(n_free, band, seed):
    n, nblk = 6 * n_free, nblk_of(n_free)
    band = min(band, nblk - 1)
    rng = np.random.default_rng(seed)
    Lt = {}
    for (bi, bj) in _tiles(nblk, band):
        avail = np.maximum(1, np.arange(NB) + NB * min(bi, band))[:, None]   # in-band columns left of the diagonal, per row
        keep = (rng.uniform(0, 1, (NB, NB)) < I_ROW / avail) | (avail <= 8)   # (the first rows dense: one camera alone is hard too)
        T = np.where(keep, rng.uniform(-1, 1, (NB, NB)), 0.0)
        if bi == bj:
            T = np.tril(T, -1) + np.eye(NB)
        T[max(0, n - bi * NB):, :] = 0
        T[:, max(0, n - bj * NB):] = 0
        Lt[(bi, bj)] = T
    Dv = 10.0 ** rng.uniform(-4, 4, nblk * NB)
    # (the whole range already inside the first camera, the large pivots first: the small ones are what cancellation leaves of
    #  entries 10^8 times their size — an ascending D would be solved to the last digit by anybody)
    Dv[:6] = 10.0 ** np.array([4.0, 2.4, 0.8, -0.8, -2.4, -4.0])
    Dt = [Dv[b * NB:(b + 1) * NB] for b in range(nblk)]
    S = _dense_from_tiles(n, _banded_gram(nblk, band, Lt, Dt))
    E = band_matvec(S, rng.uniform(-1, 1, n), band).astype(np.float64)   # (a solution of order 1, as a camera update is)
    return dict(S=S, E=E, n=n, nblk=nblk, band=band)


def oracle_solve(oracle, S, E):
    """the oracle's plain-double LDL^T (TooN's Cholesky<> restated) on the dense system"""
    n = S.shape[0]
    A = np.ascontiguousarray(S)
    b = np.ascontiguousarray(E, dtype=np.float64)
    x = np.zeros(n)
    oracle.lib.ptamo_ldlt_solve(n, A.ctypes.data, b.ctypes.data, x.ctypes.data)
    return x
