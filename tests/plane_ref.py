"""The last two host stages of MapMaker::InitFromStereo restated in numpy (fp64, sums over points sequential in index order, as
the reference's loops run), as the yardstick of ptam_calc_plane_aligner / ptam_map_apply_global_transform /
ptam_map_align_to_plane / ptam_map_scene_depth:
  calc_plane_aligner()       MapMaker::CalcPlaneAligner (src/MapMaker.cc:1100-1195) on a given table of sample triples;
  samples()                  the draw of :1113-1119 with rand() replaced by splitmix64 on a seed, as in the C ABI;
  apply_global_transform()   MapMaker::ApplyGlobalTransformationToMap (:463-472) with MapPoint::RefreshPixelVectors
                             (src/Map.cc:40-65, v3Normal_NC = (0, 0, -1));
  scene_depth()              MapMaker::RefreshSceneDepth (:1202-1219) per keyframe of a measurement table.
The eigenvectors are numpy.linalg.eigh (LAPACK, as TooN's SymEigen).  guards() returns what a test looks at before it trusts a
fixture: how far every discrete decision is from its threshold.  make_map() builds the synthetic maps of the tests."""
import numpy as np

OK, TOO_FEW, DEGENERATE = 0, 1, 2
MEAS_DT = np.dtype([("kf", "<i4"), ("point", "<i4"), ("level", "<i4"), ("source", "<i4"), ("root_pos", "<f8", (2,))])
SOURCE_DT = np.dtype([("src_kf", "<i4"), ("pad_", "<i4"), ("center_nc", "<f8", (3,)), ("one_right_nc", "<f8", (3,)),
                      ("one_down_nc", "<f8", (3,))])
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
_M64 = (1 << 64) - 1


def splitmix64(state):
    """one step: (new state, output)"""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def samples(seed, n_points, trials):
    """nA = next() % n; nB drawn again while it equals nA; nC drawn again while it equals nA or nB"""
    assert n_points >= 3 and trials >= 1
    out = np.zeros((trials, 3), np.int32)
    state = seed & _M64
    for r in range(trials):
        for i in range(3):
            while True:
                state, z = splitmix64(state)
                k = z % n_points
                if k not in out[r, :i]:
                    break
            out[r, i] = k
    return out


def _seq_sum(v):
    """the sum of a loop that adds one element after the other (numpy.sum adds pairwise)"""
    return float(np.cumsum(v)[-1]) if len(v) else 0.0


def _dot(a, b):
    """TooN's a * b for 3-vectors (rows of a against b): left to right"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def trial_plane(points, triple):
    """(v3Mean, unit v3Normal) of :1121-1130, or None where the normal's squared length is exactly 0"""
    A, B, C = (points[i] for i in triple)
    mean = 0.33333333 * ((A + B) + C)
    nrm = _cross(C - A, B - A)
    nn = _dot(nrm, nrm)
    if nn == 0.0:
        return None
    return mean, nrm / np.sqrt(nn)


def plane_distances(points, mean, nrm):
    """|v3Diff * v3Normal| per point; NaN marks the points with dDistSq == 0.0, which both loops skip"""
    diff = points - mean
    d = np.abs(_dot(diff, nrm))
    d[_dot(diff, diff) == 0.0] = np.nan
    return d


def calc_plane_aligner(points, table, max_dist=0.05):
    points = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(points)
    r = dict(status=OK, se3=IDENTITY.copy(), n_points=n, n_inliers=0, best_trial=-1, best_score=0.0, trials_skipped=0,
             inliers=np.zeros(n, bool), mean=np.zeros(3), normal=np.zeros(3), eigenvalues=np.zeros(3))
    if n < 10:
        r["status"] = TOO_FEW
        return r
    table = np.asarray(table).reshape(-1, 3)
    scores = np.full(len(table), np.inf)
    best, best_plane = 9999999999999999.9, None
    for t, triple in enumerate(table):
        plane = trial_plane(points, triple)
        if plane is None:
            r["trials_skipped"] += 1
            continue
        d = plane_distances(points, *plane)
        d = d[~np.isnan(d)]
        scores[t] = _seq_sum(np.where(d > max_dist, max_dist, d))
        if scores[t] < best:
            best, best_plane, r["best_trial"] = scores[t], plane, t
    r["scores"] = scores
    if best_plane is None:
        r["status"] = DEGENERATE
        return r
    r["best_score"] = best
    d = plane_distances(points, *best_plane)
    r["dists"] = d
    inl = d < max_dist                                  # (NaN compares false)
    r["inliers"], r["n_inliers"] = inl, int(inl.sum())
    if not inl.any():
        r["status"] = DEGENERATE
        return r
    P = points[inl]
    mean = np.array([_seq_sum(P[:, k]) for k in range(3)]) * (1.0 / len(P))
    D = P - mean
    cov = np.array([[_seq_sum(D[:, i] * D[:, j]) for j in range(3)] for i in range(3)])
    ev, vec = np.linalg.eigh(cov)
    nrm = vec[:, 0].copy()
    if nrm[2] > 0:
        nrm *= -1.0
    r.update(mean=mean, normal=nrm, eigenvalues=ev)
    row0 = np.array([1.0, 0.0, 0.0])
    row0 = row0 - nrm * _dot(row0, nrm)
    if _dot(row0, row0) == 0.0:
        r["status"] = DEGENERATE
        return r
    row0 = row0 / np.sqrt(_dot(row0, row0))
    R = np.stack([row0, _cross(nrm, row0), nrm])
    r["se3"] = np.concatenate([R.reshape(9), -_dot(R, mean)])
    return r


def guards(points, table, opts):
    """for a fixture whose status is OK: dict(score_gap, threshold_gap, eigen_gap, normal_z, one_minus_normal_x); opts: max_dist or a
    mapping that holds it"""
    max_dist = opts["max_dist"] if hasattr(opts, "__getitem__") else float(opts)
    r = calc_plane_aligner(points, table, max_dist)
    assert r["status"] == OK
    table = np.asarray(table).reshape(-1, 3)
    win = frozenset(table[r["best_trial"]].tolist())
    others = [s for t, s in zip(table, r["scores"]) if frozenset(t.tolist()) != win and np.isfinite(s)]
    ev = r["eigenvalues"]
    return dict(score_gap=(min(others) - r["best_score"]) / r["best_score"] if others else np.inf,
                threshold_gap=float(np.nanmin(np.abs(r["dists"] - max_dist))),
                eigen_gap=float((ev[1] - ev[0]) / ev[1]), normal_z=float(abs(r["normal"][2])),
                one_minus_normal_x=float(1.0 - abs(r["normal"][0])))


def se3_apply(T, v):
    """se3 * v for one vector or the rows of v: R v + t"""
    R = T[:9].reshape(3, 3)
    return np.stack([_dot(R[i], v) for i in range(3)], -1) + T[9:]


def pose_times_inverse(P, T):
    """se3CfromW * se3NewFromOld.inverse(): the inverse is (R^T, -(R^T t)), the product (Rl Rr, tl + Rl tr)"""
    Rp, Rt = P[:9].reshape(3, 3), T[:9].reshape(3, 3)
    it = -np.array([_dot(Rt[:, i], T[9:]) for i in range(3)])
    R = np.array([[_dot(Rp[r], Rt[c]) for c in range(3)] for r in range(3)])
    return np.concatenate([R.reshape(9), P[9:] + np.array([_dot(Rp[r], it) for r in range(3)])])


def refresh_pixel_vectors(pose, world, src):
    """MapPoint::RefreshPixelVectors for one point: (v3PixelRight_W, v3PixelDown_W)"""
    R = pose[:9].reshape(3, 3)
    cam_h = abs(se3_apply(pose, world)[2])              # |v3PlanePoint_C * (0, 0, -1)|
    on_plane = [np.asarray(src[f]) * cam_h / abs(src[f][2]) for f in ("center_nc", "one_right_nc", "one_down_nc")]
    return tuple(np.array([_dot(R[:, i], v - on_plane[0]) for i in range(3)]) for v in on_plane[1:])


def apply_global_transform(se3, poses, points, sources=None):
    """-> (poses, points, (right, down) or None); the inputs are not modified"""
    se3 = np.asarray(se3, np.float64).reshape(12)
    poses = np.array([pose_times_inverse(p, se3) for p in np.asarray(poses, np.float64).reshape(-1, 12)]).reshape(-1, 12)
    points = se3_apply(se3, np.asarray(points, np.float64).reshape(-1, 3))
    if sources is None:
        return poses, points, None
    pv = [refresh_pixel_vectors(poses[s["src_kf"]], w, s) for w, s in zip(points, sources)]
    return poses, points, (np.array([p[0] for p in pv]).reshape(-1, 3), np.array([p[1] for p in pv]).reshape(-1, 3))


def pixel_vectors(poses, points, sources):
    """RefreshPixelVectors of every point against the tables as they are"""
    return apply_global_transform(IDENTITY, poses, points, sources)[2]


def scene_depth(poses, points, meas):
    """per keyframe (mean, sigma, n): 0 / 0 / 0 without a row, sigma 0 where rounding made the radicand negative"""
    poses, points = np.asarray(poses, np.float64).reshape(-1, 12), np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros((len(poses), 3))
    for k, P in enumerate(poses):
        rows = meas["point"][meas["kf"] == k]
        if len(rows) == 0:
            continue
        z = se3_apply(P, points[rows])[:, 2]
        mean = _seq_sum(z) / len(z)
        rad = _seq_sum(z * z) / len(z) - mean * mean
        out[k] = mean, (np.sqrt(rad) if rad >= 0 else 0.0), len(z)
    return out


# ---- synthetic maps ---------------------------------------------------------------------------------------------------------------
def _small_pose(rng, scale):
    """a camera near the origin that looks down +z: a rotation of up to ~scale radians, a translation of that size"""
    w = rng.uniform(-scale, scale, 3)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    return np.concatenate([R.reshape(9), rng.uniform(-scale, scale, 3)])


def make_map(n, seed, n_kf=2, outlier_fraction=0.3, noise=0.02, with_meas=True):
    """n points about a tilted plane two units in front of the cameras, a fraction of them 0.1 .. 1 off it; n_kf keyframes; a
    source row per point (src_kf = point % n_kf); a measurement table in which keyframe k sees the points with (point + k) % 3 != 0
    (with_meas = False: an empty one)
    -> (points (n, 3), poses (n_kf, 12), sources, meas, on_plane (n,) bool)"""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.2, 0.3, -0.93])
    nrm /= np.linalg.norm(nrm)
    a = np.cross(nrm, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    uv = rng.uniform(-1.0, 1.0, (n, 2))
    off = rng.uniform(-noise, noise, n)
    on_plane = np.ones(n, bool)
    on_plane[rng.permutation(n)[:int(round(outlier_fraction * n))]] = False
    far = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)
    off = np.where(on_plane, off, far)
    points = np.array([0.1, -0.2, 2.0]) + uv[:, :1] * a + uv[:, 1:] * b + off[:, None] * nrm
    poses = np.array([_small_pose(rng, 0.1) for _ in range(n_kf)])
    sources = np.zeros(n, SOURCE_DT)
    sources["src_kf"] = np.arange(n) % n_kf
    xy = rng.uniform(-0.4, 0.4, (n, 2))
    for f, d in (("center_nc", (0, 0)), ("one_right_nc", (0.002, 0)), ("one_down_nc", (0, 0.002))):
        v = np.concatenate([xy + d, np.ones((n, 1))], 1)
        sources[f] = v / np.linalg.norm(v, axis=1)[:, None]
    seen = [np.flatnonzero((np.arange(n) + k) % 3 != 0) for k in range(n_kf)] if with_meas else []
    meas = np.zeros(sum(len(p) for p in seen), MEAS_DT)
    if len(meas):
        meas["kf"], meas["point"] = np.repeat(np.arange(n_kf), [len(p) for p in seen]), np.concatenate(seen)
    meas["source"] = 2
    return points, poses, sources, meas, on_plane
