"""CPU: the numpy restatement of HomographyInit::Compute (tests/homography_ref.py) is a sound yardstick — it recovers known poses,
takes the ambiguous branch where the scene asks for it and resolves it to the true pose, handles the sizes at which the code
changes path, and does not depend on the sign of the homography it refines."""
import numpy as np
import pytest

from tests import homography_ref as HR


def _pose_errors(se3, R, t):
    """(Frobenius distance of the rotations, distance of the unit translations)"""
    return (float(np.linalg.norm(se3[:9].reshape(3, 3) - R)),
            float(np.linalg.norm(se3[9:] / np.linalg.norm(se3[9:]) - t / np.linalg.norm(t))))


@pytest.mark.parametrize("n", [12, 65, 200])
def test_noise_free_plane_gives_the_pose(n):
    m, R, t, _ = HR.make_scene("tilted", n, 0, noise_px=0.0)
    r = HR.compute(m, 5.0, HR.samples(7, n, 300))
    assert r["status"] == HR.OK and r["n_inliers"] == n and r["inliers"].all() and not r["ambiguous"]
    dr, dt = _pose_errors(r["se3"], R, t)
    assert dr < 1e-9 and dt < 1e-9, (dr, dt)
    assert abs(np.linalg.det(r["se3"][:9].reshape(3, 3)) - 1.0) < 1e-12


@pytest.mark.parametrize("n,extra,seed", [(64, 14, 0), (200, 40, 1)])
def test_facing_plane_takes_the_sampson_branch_and_finds_the_true_pose(n, extra, seed):
    """a plane facing a narrow bundle of points, the camera moving mostly forwards: both surviving normals are in front of every
    inlier, the second visibility counts are equal, and the Sampson sums over all matches — the off-plane points among them —
    decide"""
    m, R, t, on_plane = HR.make_scene("facing", n, seed, noise_px=0.3, outliers=extra)
    r = HR.compute(m, 5.0, HR.samples(8 if n == 64 else 7, n, 300))
    assert r["status"] == HR.OK and r["ambiguous"]
    s0, s1 = (q["score"] for q in r["last_two"])
    assert s1 / s0 >= 0.9 and r["sampson"][0] != r["sampson"][1]
    errs = [_pose_errors(np.concatenate([q["R"].reshape(9), q["t"]]), R, t) for q in r["last_two"]]
    chosen = 0 if r["sampson"][0] <= r["sampson"][1] else 1
    assert np.array_equal(r["se3"][:9], r["last_two"][chosen]["R"].reshape(9))
    print(errs, r["sampson"])
    assert errs[chosen][1] < 0.5 * errs[1 - chosen][1] and errs[chosen][0] < errs[1 - chosen][0]   # nearer the truth than the other one
    assert errs[chosen][0] < 0.06 and errs[chosen][1] < 0.3
    assert r["inliers"][on_plane].mean() > 0.9


@pytest.mark.parametrize("n", [4, 9, 10])
def test_sizes_where_the_path_changes(n):
    """n = 4: a nine-row matrix whose last row is zero; n = 9: the last size without trials; n = 10: the first with"""
    m, R, t, _ = HR.make_scene("tilted", n, 2, noise_px=0.0)
    r = HR.compute(m, 5.0, HR.samples(3, n, 300))
    assert r["status"] == HR.OK and r["n_inliers"] == n
    assert (r["best_trial"] == -1 and r["best_score"] == 0.0) if n < 10 else (0 <= r["best_trial"] < 300 and r["scores"].shape == (300,))
    dr, dt = _pose_errors(r["se3"], R, t)
    assert dr < 1e-7 and dt < 1e-7, (dr, dt)
    assert np.abs(HR.homography_from_matches(m[:4]) @ np.append(m["first"][0], 1.0)).max() > 0   # (the 4-match DLT alone)


@pytest.mark.parametrize("kind,n,extra", [("tilted", 64, 8), ("facing", 64, 14), ("tilted", 9, 0)])
def test_negated_homography_gives_the_same_pose(kind, n, extra):
    m = HR.make_scene(kind, n, 1, 0.3, extra)[0]
    table = HR.samples(8, n, 300)
    a, b = HR.compute(m, 5.0, table), HR.compute(m, 5.0, table, flip_sign=True)
    assert a["status"] == b["status"] == HR.OK and a["ambiguous"] == b["ambiguous"] and np.array_equal(a["inliers"], b["inliers"])
    assert np.allclose(a["homography"], -b["homography"], rtol=0, atol=1e-12 * np.abs(a["homography"]).max())
    assert np.allclose(a["se3"], b["se3"], rtol=0, atol=1e-11)


def test_gross_outliers_are_rejected():
    m, R, t, on_plane = HR.make_scene("tilted", 200, 0, 0.5, 30)
    r = HR.compute(m, 5.0, HR.samples(7, 200, 300))
    assert r["status"] == HR.OK and r["inliers"][on_plane].all() and r["inliers"][~on_plane].sum() <= 3
    dr, dt = _pose_errors(r["se3"], R, t)
    assert dr < 0.02 and dt < 0.1


def test_no_inliers_and_degenerate_are_reported():
    m = HR.make_scene("tilted", 9, 3, 0.5, 0)[0]
    assert HR.compute(m, 1e-9, None)["status"] == HR.NO_INLIERS
    assert HR.decompose(np.eye(3)) is None and HR.decompose(np.diag([2.0, 2.0, 1.0])) is None


def test_generator():
    for seed, n, trials in ((0, 4, 50), (99, 10, 300), (2 ** 64 - 1, 1000, 100)):
        t = HR.samples(seed, n, trials)
        assert t.shape == (trials, 4) and t.dtype == np.int32 and (t >= 0).all() and (t < n).all()
        assert all(len(set(q)) == 4 for q in t.tolist())
        assert np.array_equal(t, HR.samples(seed, n, trials)) and not np.array_equal(t, HR.samples(seed + 1, n, trials))
    assert (np.sort(HR.samples(3, 4, 20), axis=1) == np.arange(4)).all()            # four matches: every quadruple is all of them
    # splitmix64's published first outputs for the state 0 (Vigna's reference implementation)
    s, z0 = HR.splitmix64(0)
    s, z1 = HR.splitmix64(s)
    assert (z0, z1) == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
