"""HomographyInit::Compute (src/HomographyInit.cc) restated in numpy, function by function, as the yardstick of
ptam_homography_init / ptam_trails_homography: the DLT (:65-115), the MLESAC loop (:179-230) on a given sample table, the inlier
test and the score (:14-33), RefineHomographyWithInliers (:120-177) with Tukey's sigma and weights (include/Tools.h) and the prior
of 1.0, DecomposeHomography (:232-339, Faugeras & Lustman's eight solutions in the reference's push order) and
ChooseBestDecomposition (:363-435).  The SVDs are numpy.linalg.svd, the 9x9 solve numpy.linalg.solve.  The reference draws its
quadruples with rand(); here the draw is a table (samples(): splitmix64 on a seed), as in the C ABI.

compute() also returns what the tests' fixture guards look at: every trial's score, every match's squared pixel error under the
winning homography, and every visibility value that was compared with zero."""
import numpy as np

MATCH_DT = np.dtype([("first", "<f8", (2,)), ("second", "<f8", (2,)), ("jac", "<f8", (4,))])
OK, DEGENERATE, NO_INLIERS = 0, 1, 2
_M64 = (1 << 64) - 1


def splitmix64(state):
    """one step: (new state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def samples(seed, n_matches, trials):
    """the quadruples of :198-211 with rand() replaced by splitmix64(seed): index = next() % n_matches, a repeat inside a
    quadruple is drawn again"""
    assert n_matches >= 4 and trials >= 1
    out = np.zeros((trials, 4), np.int32)
    state = seed & _M64
    for r in range(trials):
        for i in range(4):
            while True:
                state, z = splitmix64(state)
                k = z % n_matches
                if k not in out[r, :i]:
                    break
            out[r, i] = k
    return out


def _unproject(v):
    return np.concatenate([v, np.ones(v.shape[:-1] + (1,))], axis=-1)


def pixel_error_sq(H, m):
    """dSquaredError of IsHomographyInlier / MLESACScore for every match"""
    p = _unproject(m["first"]) @ H.T
    err = m["second"] - p[:, :2] / p[:, 2:3]
    J = m["jac"].reshape(-1, 2, 2)
    pe = np.einsum("nij,nj->ni", J, err)
    return (pe * pe).sum(1)


def mlesac_score(H, m, max_sq):
    e2 = pixel_error_sq(H, m)
    return float(np.where(e2 > max_sq, max_sq, e2).sum())


def homography_from_matches(m):
    n = len(m)
    assert n >= 4
    A = np.zeros((max(2 * n, 9), 9))
    x, y, u, v = m["first"][:, 0], m["first"][:, 1], m["second"][:, 0], m["second"][:, 1]
    one, zero = np.ones(n), np.zeros(n)
    A[0:2 * n:2] = np.stack([x, y, one, zero, zero, zero, -x * u, -y * u, -u], 1)
    A[1:2 * n:2] = np.stack([zero, zero, zero, x, y, one, -x * v, -y * v, -v], 1)
    vt = np.linalg.svd(A, full_matrices=False)[2]      # (a 9-row matrix whose last row is zero when 2n < 9)
    return vt[8].reshape(3, 3)


def tukey_sigma_sq(e2):
    """Tukey::FindSigmaSquared: the median is sorted[n / 2]; 2n - 6 in size_t arithmetic"""
    n = len(e2)
    assert n > 0
    med = np.sort(e2)[n // 2]
    den = (2 * n - 6) % (1 << 64)
    with np.errstate(divide="ignore"):
        sigma = 1.4826 * (1 + np.float64(5.0) / np.float64(den)) * np.sqrt(med)
    sigma = 4.6851 * sigma
    return sigma * sigma


def tukey_weight(e2, s2):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(e2 > s2, 0.0, 1.0 - e2 / s2)
    return np.where(e2 == 0.0, 1.0, r * r)        # (0 / 0 under a zero median: defined as the full weight, as in the C ABI)


def refine(H, inl):
    """one RefineHomographyWithInliers on the inlier matches"""
    f3 = _unproject(inl["first"])
    s3 = f3 @ H.T
    J2 = inl["jac"].reshape(-1, 2, 2)
    err = np.einsum("nij,nj->ni", J2, inl["second"] - s3[:, :2] / s3[:, 2:3])
    e2 = (err * err).sum(1)
    den = s3[:, 2]
    J = np.zeros((len(inl), 2, 9))
    J[:, 0, 0:3] = f3 / den[:, None]
    J[:, 0, 6:9] = -f3 * s3[:, 0:1] / (den * den)[:, None]
    J[:, 1, 3:6] = f3 / den[:, None]
    J[:, 1, 6:9] = -f3 * s3[:, 1:2] / (den * den)[:, None]
    J = np.einsum("nij,njk->nik", J2, J)
    w = tukey_weight(e2, tukey_sigma_sq(e2))
    C = np.eye(9) + np.einsum("n,nri,nrj->ij", w, J, J)          # WLS<9>::add_prior(1.0) + add_mJ
    vec = np.einsum("n,nr,nri->i", w, err, J)
    return H + np.linalg.solve(C, vec).reshape(3, 3)


def decompose(H):
    """DecomposeHomography: the eight (d, R', t', n, R, t) in push order, or None where nCase != 1"""
    U, dg, Vt = np.linalg.svd(H)
    d1, d2, d3 = np.abs(dg)
    V = Vt.T
    s = np.linalg.det(U) * np.linalg.det(V)
    if not (d1 != d2 and d2 != d3):
        return None
    x1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    x3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    e1, e3 = [1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]
    out = []
    for k in range(4):      # d' > 0
        sin = (d1 - d3) * x1 * x3 * e1[k] * e3[k] / d2
        cos = (d1 * x3 * x3 + d3 * x1 * x1) / d2
        Rp = np.array([[cos, 0, -sin], [0, 1, 0], [sin, 0, cos]])
        tp = np.array([(d1 - d3) * x1 * e1[k], 0.0, (d1 - d3) * -x3 * e3[k]])
        out.append(dict(d=s * d2, Rp=Rp, tp=tp, n=V @ np.array([x1 * e1[k], 0.0, x3 * e3[k]])))
    for k in range(4):      # d' < 0
        sin = (d1 + d3) * x1 * x3 * e1[k] * e3[k] / d2
        cos = (d3 * x1 * x1 - d1 * x3 * x3) / d2
        Rp = np.array([[cos, 0, sin], [0, -1, 0], [sin, 0, -cos]])
        tp = np.array([(d1 + d3) * x1 * e1[k], 0.0, (d1 + d3) * x3 * e3[k]])
        out.append(dict(d=s * -d2, Rp=Rp, tp=tp, n=V @ np.array([x1 * e1[k], 0.0, x3 * e3[k]])))
    for i, dec in enumerate(out):
        dec["index"] = i
        dec["R"] = s * U @ dec["Rp"] @ V.T
        dec["t"] = U @ dec["tp"]
    return out


def sampson_sum(R, t, m, limit):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R                                                    # column j = t ^ (column j of R)
    a, b = _unproject(m["second"]), _unproject(m["first"])
    err = np.einsum("ni,ij,nj->n", a, E, b)
    f, ft = b @ E.T, a @ E
    d = err * err / ((f[:, :2] ** 2).sum(1) + (ft[:, :2] ** 2).sum(1))
    return float(np.where(d > limit, limit, d).sum())


def choose_best(decs, H, inl, m, max_sq):
    """ChooseBestDecomposition -> (the chosen decomposition, ambiguous, the two Sampson sums, the visibility values compared
    with zero).  std::sort on eight elements is an insertion sort: equal scores keep their order, like sorted()."""
    vis = []
    for dec in decs:
        v = (_unproject(inl["first"]) @ H[2]) / dec["d"]
        vis.append(v)
        dec["score"] = -int((v > 0.0).sum())
    decs = sorted(decs, key=lambda q: q["score"])[:4]
    for dec in decs:
        v = (_unproject(inl["first"]) @ dec["n"]) / dec["d"]
        vis.append(v)
        dec["score"] = -int((v > 0.0).sum())
    decs = sorted(decs, key=lambda q: q["score"])[:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.float64(decs[1]["score"]) / np.float64(decs[0]["score"])
    vis = np.concatenate(vis)
    if ratio < 0.9:
        return decs[0], False, (0.0, 0.0), vis, decs
    sums = tuple(sampson_sum(q["R"], q["t"], m, 4.0 * max_sq) for q in decs)
    return (decs[0] if sums[0] <= sums[1] else decs[1]), True, sums, vis, decs


def compute(m, max_pixel_error, table, flip_sign=False):
    """HomographyInit::Compute on the sample table (trials x 4; unused below ten matches).  flip_sign: the best homography is
    negated before the refinements (the tests' check that the result does not depend on the SVD's sign)."""
    m = np.ascontiguousarray(m, dtype=MATCH_DT)
    n, max_sq = len(m), max_pixel_error * max_pixel_error
    r = dict(status=OK, n_matches=n, best_trial=-1, best_score=0.0, ambiguous=False, sampson=(0.0, 0.0), se3=None, scores=None)
    if n < 10:
        H = homography_from_matches(m)
    else:
        H, best = np.eye(3), 999999999999999999.9
        r["scores"], r["table"] = np.zeros(len(table)), np.asarray(table)
        for k, quad in enumerate(table):
            Hk = homography_from_matches(m[quad])
            r["scores"][k] = sc = mlesac_score(Hk, m, max_sq)
            if sc < best:
                H, best, r["best_trial"] = Hk, sc, k
        r["best_score"] = best
    if flip_sign:
        H = -H
    r["first_error_sq"] = e2 = pixel_error_sq(H, m)
    r["inliers"] = flags = e2 < max_sq
    r["n_inliers"] = int(flags.sum())
    r["homography"] = H
    if r["n_inliers"] == 0:
        r["status"] = NO_INLIERS
        return r
    inl = m[flags]
    for _ in range(5):
        H = refine(H, inl)
    r["homography"] = H
    decs = decompose(H)
    if decs is None:
        r["status"] = DEGENERATE
        return r
    best, r["ambiguous"], r["sampson"], r["visibility"], r["last_two"] = choose_best(decs, H, inl, m, max_sq)
    r["se3"] = np.concatenate([best["R"].reshape(9), best["t"]])
    return r


# ---- scenes for the tests ------------------------------------------------------------------------------------------------------
def rodrigues(w):
    w = np.asarray(w, float)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(kind, n, seed, noise_px=0.5, outliers=0, focal=300.0):
    """n matches between two views -> (matches MATCH_DT, R, t second-from-first, is-on-plane flags).
    "tilted": a plane at 3 m tilted by ~0.5 rad, a 0.3 m sideways baseline and a 0.08 rad rotation, a 0.5 x 0.4 field of view;
              `outliers` matches get a second position anywhere in the field (gross outliers).
    "facing": a plane at 3 m that nearly faces the camera (tilted by ~0.4 rad), seen as a narrow bundle (+-0.08), with a mostly
              forward motion tilted the other way: the second solution roughly swaps normal and translation, and both normals
              are in front of every point — the case the Sampson scores decide; `outliers` matches are
              real points off the plane (1.2 m - 2.4 m deep), which obey the true epipolar geometry only.
    jac is a pinhole's derivative with a mild radial term, so that all four entries are used."""
    rng = np.random.default_rng(seed)
    if kind == "tilted":
        R, t = rodrigues([0.02, -0.07, 0.03]), np.array([-0.3, 0.02, 0.03])
        nrm, half = np.array([0.45, -0.15, -1.0]), np.array([0.5, 0.4])
    else:
        R, t = rodrigues([0.01, 0.015, -0.02]), np.array([-0.16, 0.03, -0.3])
        nrm, half = np.array([0.45, 0.1, -1.0]), np.array([0.08, 0.08])
    nrm = nrm / np.linalg.norm(nrm)
    first = rng.uniform(-half, half, (n, 2))
    rays = _unproject(first)
    depth = (nrm @ np.array([0, 0, 3.0])) / (rays @ nrm)             # the plane passes through (0, 0, 3)
    on_plane = np.ones(n, bool)
    bad = rng.permutation(n)[:outliers]
    if kind == "facing":
        depth[bad] = rng.uniform(1.2, 2.4, len(bad))
        on_plane[bad] = False
    P = rays * depth[:, None] @ R.T + t
    second = P[:, :2] / P[:, 2:3]
    second += rng.normal(0, noise_px / focal, (n, 2)) if noise_px else 0.0
    if kind == "tilted" and outliers:
        second[bad] = rng.uniform(-half, half, (len(bad), 2))
        on_plane[bad] = False
    m = np.zeros(n, MATCH_DT)
    m["first"], m["second"] = first, second
    r2 = (second * second).sum(1)
    k = -0.2                                                          # u = f x (1 + k r^2): du/dx = f (1 + k r^2 + 2 k x^2), ...
    m["jac"][:, 0] = focal * (1 + k * r2 + 2 * k * second[:, 0] ** 2)
    m["jac"][:, 1] = m["jac"][:, 2] = focal * 2 * k * second[:, 0] * second[:, 1]
    m["jac"][:, 3] = focal * (1 + k * r2 + 2 * k * second[:, 1] ** 2)
    return m, R, t, on_plane


def guards(r, max_pixel_error):
    """what a fixture must satisfy so that rounding cannot flip a discrete decision (the tests assert every entry):
    score_gap: best vs second-best MLESAC score, relative (inf below ten matches); threshold_gap: the nearest squared pixel error
    to the threshold, relative; visibility: the smallest |visibility value|; sampson_gap: relative, inf unless ambiguous"""
    max_sq = max_pixel_error ** 2
    g = dict(score_gap=np.inf, sampson_gap=np.inf)
    if r["scores"] is not None:                     # (a trial with the winner's quadruple in the winner's order computes the winner's bits:
        other = (r["table"] != r["table"][r["best_trial"]]).any(1)   #  a tie, which the lowest index wins everywhere)
        if other.any():
            g["score_gap"] = (r["scores"][other].min() - r["best_score"]) / r["best_score"]
    g["threshold_gap"] = float(np.abs(r["first_error_sq"] - max_sq).min() / max_sq)
    g["visibility"] = float(np.abs(r["visibility"]).min())
    if r["ambiguous"]:
        a, b = r["sampson"]
        g["sampson_gap"] = abs(a - b) / max(a, b)
    return g
