"""CPU: the numpy restatement of the calibrator's optimiser (tests/calib_ref.py) does what the reference's does — it recovers a
known ATAN camera from grid corners, with and without distortion, and GuessInitialPose with the true camera returns the true
pose — and the two ways of solving a step's system that the GPU tests' tolerance rests on agree."""
import numpy as np
import pytest

from tests import calib_cases as CC, calib_ref as CR


@pytest.fixture(scope="module")
def recovered():
    """the 4 x 48 case from the default parameters and the guessed poses, 300 steps"""
    grids = CC.recover_case()
    assert [len(c) for c, _ in grids] == [48] * 4
    ref = CC.reference_from(grids)
    steps = [ref.optimize_one_step() for _ in range(300)]
    return ref, steps


def test_restatement_recovers_the_known_camera(recovered):
    ref, steps = recovered
    rms = np.array([s["rms"] for s in steps])
    cond = max(CR.condition_number(s["sv"]) for s in steps)
    err = float(np.abs(ref.cam.params - np.array(CC.TRUTH)).max())
    print("rms at step 0 %.3f px, after 300 steps %.3g; parameter error %.3g; largest condition number %.3g" % (rms[0], rms[-1], err, cond))
    assert rms[0] > 5.0                     # the default camera is far from the truth
    assert all(s["n_meas"] == 4 * 48 for s in steps)
    assert cond < 1e7                       # the bar of every test that compares the device with this restatement
    assert (np.diff(rms[rms > 1e-9]) < 0).all()   # decreasing until it is rounding noise
    assert err < 1e-9 and rms[-1] < 1e-9    # the fixed point, not its last digits


def test_restatement_recovers_a_camera_without_distortion():
    grids = CC.recover_case(CC.TRUTH_NO_DISTORTION)
    ref = CC.reference_from(grids, None, disable=True)
    for _ in range(250):
        r = ref.optimize_one_step()
        assert ref.cam.params[4] == 0.0
    err = float(np.abs(ref.cam.params - np.array(CC.TRUTH_NO_DISTORTION)).max())
    print("rms after 250 steps %.3g, parameter error %.3g" % (r["rms"], err))
    assert r["rms"] < 1e-8 and err < 1e-9


@pytest.mark.parametrize("truth", [CC.TRUTH, CC.TRUTH_NO_DISTORTION])
def test_guess_with_the_true_camera_is_the_true_pose(truth):
    cam = CR.Camera(truth, CC.SIZE)
    for c, pose in CC.recover_case(truth):
        st, guess = CR.guess_initial_pose(cam, c)
        assert st == CR.GUESS_OK and guess[11] > 0
        assert np.abs(guess - pose).max() < 1e-12   # (1e-14 measured; the model is exact on these grids)


def test_guess_refuses_what_it_cannot_use():
    c = CC.recover_case()[0][0].copy()
    c["u"][3] = np.nan
    assert CR.guess_initial_pose(CR.Camera(CC.TRUTH, CC.SIZE), c)[0] == CR.GUESS_REFUSED


def test_the_two_solves_agree_on_the_gpu_tests_systems():
    """the SVD back-substitution and block elimination in longdouble: their difference is the solver noise the GPU tests allow 16x of"""
    for name, imgs, size in (("1 x 12", CC.small_images(1, 12, 3), CC.SIZE), ("3 x 12", CC.small_images(3, 12, 3), CC.SIZE),
                             ("65 mixed", CC.images_with_counts(CC.mixed_counts_65(), size=CC.SMALL_SIZE), CC.SMALL_SIZE)):
        noise, cond = CC.solver_noise(CC.reference_from(imgs, size=size))
        print("%s: relative difference %.3g, condition number %.3g" % (name, noise, cond))
        assert cond < 1e7 and noise < 1e-8   # (eps x condition number is 2e-9 at the bar)


def test_nothing_to_adjust_changes_nothing():
    ref = CC.reference_from(CC.small_images(2, 12, 3))
    behind = [np.concatenate([p[:9], [p[9], p[10], -abs(p[11])]]) for p in ref.poses]
    ref.poses = [b.copy() for b in behind]
    before = ref.cam.params.copy()
    r = ref.optimize_one_step()
    assert r["n_meas"] == 0 and np.array_equal(ref.cam.params, before) and all(np.array_equal(a, b) for a, b in zip(ref.poses, behind))
