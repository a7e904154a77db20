"""-m gpu: the camera calibrator's optimiser on the device (ptam_calib_*, host.CameraCalibrator) against the numpy restatement of
the reference (tests/calib_ref.py): the initial pose, one step, the skip tests, the recovery of a known camera in one call, call
splitting, adding images later, residuals and every refusal.

Every test that compares with the restatement first asserts that the restatement's own matrix has a condition number below 1e7:
the device solves the arrowhead system by block elimination, the reference by an SVD with a cut at 1e9 (ptam_hip.h).  The
tolerance of a step is 16 x the largest relative difference, over the one-step shapes, between the restatement's SVD solve and
block elimination in longdouble — solver noise at this conditioning, measured on the CPU (docs/LOG_calib.md)."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import calib_cases as CC, calib_ref as CR

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
COND_BAR = 1e7


@pytest.fixture(scope="module")
def ctx(hip):
    c = host.Context(lib=hip, size=CC.SIZE)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_small(hip):
    c = host.Context(lib=hip, size=CC.SMALL_SIZE)
    yield c
    c.close()


@pytest.fixture(scope="module")
def step_cases():
    """name -> (images, image size); computed once"""
    return {"1x12": (CC.small_images(1, 12, 3), CC.SIZE), "3x12": (CC.small_images(3, 12, 3), CC.SIZE),
            "65 mixed": (CC.images_with_counts(CC.mixed_counts_65(), size=CC.SMALL_SIZE), CC.SMALL_SIZE)}


@pytest.fixture(scope="module")
def step_tolerance(step_cases):
    noise = {}
    for name, (imgs, size) in step_cases.items():
        noise[name], cond = CC.solver_noise(CC.reference_from(imgs, size=size))
        assert cond < COND_BAR, (name, cond)
    tol = 16.0 * max(noise.values())
    print("solver noise per shape %s -> relative tolerance of a step %.3g" % ({k: "%.3g" % v for k, v in noise.items()}, tol))
    return tol


def calibrator(c, images, params=None, disable=False, poses=None, max_images=None):
    cal = host.CameraCalibrator(c, max_images or max(len(images), 1), sum(len(x) for x, _ in images) + 64)
    cal.Reset(params, disable)
    assert (cal.AddImages([x for x, _ in images]) == _abi.CALIB_GUESS_OK).all()
    if poses is not None:
        cal.SetPoses(np.array(poses))
    return cal


def snapshot(cal):
    return cal.counts(), cal.Params().tobytes(), cal.Poses().tobytes()


def assert_step_equal(cal, ref, tol, what):
    """one OptimizeOneStep on both, from the same state: count exactly, RMS, the parameter update and every pose within tol"""
    p0 = cal.Params()
    assert np.array_equal(p0, ref.cam.params) and np.array_equal(cal.Poses(), np.array(ref.poses))
    r = cal.OptimizeOneStep()
    rr = ref.optimize_one_step()
    assert CR.condition_number(rr["sv"]) < COND_BAR
    assert r["status"] == _abi.CALIB_OK and r["n_measurements"] == rr["n_meas"] and r["steps"] == 1
    scale = float(np.abs(rr["update"]).max())
    d_upd = float(np.abs((r["params"] - p0) - rr["update"][-5:]).max())
    poses_ref = np.array(ref.poses)
    d_pose = float(np.abs(cal.Poses() - poses_ref).max())
    d_rms = abs(r["rms"] - rr["rms"])
    # a pose is exp(update) * pose: an error d in the update moves an entry by at most d (1 + |pose|); the subtraction
    # params - p0 and the products of exp * pose round at a few eps of the values themselves
    pose_bound = tol * scale * (1.0 + float(np.abs(poses_ref).max())) + 16 * EPS * float(np.abs(poses_ref).max())
    print("%s: update off by %.3g (bound %.3g), poses by %.3g (bound %.3g), rms by %.3g of %.6g" %
          (what, d_upd, tol * scale + 4 * EPS, d_pose, pose_bound, d_rms, rr["rms"]))
    assert d_upd <= tol * scale + 4 * EPS
    assert d_pose <= pose_bound
    assert d_rms <= 64 * EPS * rr["rms"]   # a sum of n squares in another order: n eps at the very most, n <= 1426; half of it after the root
    assert np.array_equal(r["params"], cal.Params()) and r["history"][0] == r["rms"]
    assert r["pixel_aspect_ratio"] == (ref.size[1] * r["params"][1]) / (ref.size[0] * r["params"][0])


# ---- the initial pose ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 257])
def test_initial_pose_is_the_true_pose(ctx, n):
    (c, truth), = CC.images_with_counts([n], seed=5 + n)
    assert len(c) == n
    st, guess = CR.guess_initial_pose(CR.Camera(CC.TRUTH, CC.SIZE), c)
    assert st == CR.GUESS_OK and np.isfinite(guess).all() and guess[11] > 0
    ref_err = float(np.abs(guess - truth).max())
    cal = calibrator(ctx, [(c, truth)], CC.TRUTH)
    err = float(np.abs(cal.Poses()[0] - truth).max())
    print("%d corners: device %.3g, restatement %.3g" % (n, err, ref_err))
    assert cal.counts() == (1, n) and cal.Poses()[0][11] > 0
    assert err <= max(64.0 * ref_err, 1e-12)
    cal.close()


# ---- one step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x12", "3x12", "65 mixed"])
def test_one_step_is_the_restatements_step(ctx, ctx_small, step_cases, step_tolerance, name):
    imgs, size = step_cases[name]
    if name == "65 mixed":
        assert len(imgs) == 65 and {63, 64, 65, 255, 256, 257} <= set(len(c) for c, _ in imgs)
    ref = CC.reference_from(imgs, size=size)
    cal = calibrator(ctx if size == CC.SIZE else ctx_small, imgs, poses=ref.poses)
    assert_step_equal(cal, ref, step_tolerance, name)
    assert_step_equal(cal_resync(cal, ref), ref, step_tolerance, name + ", second step")
    cal.close()


def cal_resync(cal, ref):
    """the restatement takes over the device's state, so that the next step starts from the same bits"""
    ref.cam.params = cal.Params()
    ref.cam.refresh()
    ref.poses = [p.copy() for p in cal.Poses()]
    return cal


# ---- the skip tests -------------------------------------------------------------------------------------------------------------------
def tilted_pose(deg, t):
    a = np.deg2rad(deg)
    R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return np.concatenate([R.ravel(), np.asarray(t, float)])


def behind(pose):
    return np.concatenate([pose[:9], [pose[9], pose[10], -abs(pose[11]) - 1.0]])


def test_skipped_corners_count_and_sums(ctx, step_tolerance):
    imgs = CC.small_images(3, 12, 3)                       # (12 corners an image: 24 put the condition number at 1.8e7)
    ref = CC.reference_from(imgs)
    ref.poses[0] = tilted_pose(75, (-3.5, -1.0, -0.6))   # the grid crosses the camera's plane: both skip tests fire
    ref.poses[2] = behind(ref.poses[2])                    # every corner skipped
    c = imgs[0][0]
    z = (np.stack([c["gx"], c["gy"], 0 * c["gx"]], 1).astype(float) @ ref.poses[0][:9].reshape(3, 3).T + ref.poses[0][9:])[:, 2]
    valid = CR.project_image(ref.cam, ref.poses[0], c)[5]
    assert (z <= 0.001).sum() == 4 and ((z > 0.001) & ~valid).sum() == 2 and valid.sum() == 6
    assert not CR.project_image(ref.cam, ref.poses[2], imgs[2][0])[5].any()
    cal = calibrator(ctx, imgs, poses=ref.poses)
    uv, dev_valid = cal.Residuals(0)
    assert np.array_equal(dev_valid, valid) and not cal.Residuals(2)[1].any()
    skipped_pose = cal.Poses()[2].tobytes()
    assert_step_equal(cal, ref, step_tolerance, "skips")
    assert cal.last["n_measurements"] == 6 + 12
    assert cal.Poses()[2].tobytes() == skipped_pose           # its block is the prior alone: the update is exactly zero
    cal.close()


def test_all_skipped_is_no_measurements(ctx):
    imgs = CC.small_images(2, 12, 3)
    ref = CC.reference_from(imgs)
    cal = calibrator(ctx, imgs, poses=[behind(p) for p in ref.poses])
    before = snapshot(cal)
    for steps in (1, 3):
        r = cal.Optimize(steps)
        assert r["status"] == _abi.CALIB_NO_MEASUREMENTS and r["n_measurements"] == 0 and r["history"] is None
        assert snapshot(cal) == before and np.array_equal(r["params"], np.array(CR.DEFAULT_PARAMS))
    cal.SetPoses(np.array(ref.poses))                          # and the handle still works
    assert cal.OptimizeOneStep()["status"] == _abi.CALIB_OK
    cal.close()


# ---- the known camera, from corners alone ---------------------------------------------------------------------------------------------
def test_one_call_recovers_the_known_camera(ctx):
    grids = CC.recover_case()
    assert [len(c) for c, _ in grids] == [48] * 4
    cal = calibrator(ctx, grids)
    assert np.array_equal(cal.Params(), np.array(CR.DEFAULT_PARAMS))
    r = cal.Optimize(300)
    err = float(np.abs(r["params"] - np.array(CC.TRUTH)).max())
    h = r["history"]
    print("rms %.3f -> %.3g px, parameter error %.3g, pose error %.3g" % (h[0], h[-1], err, max(np.abs(p - t).max() for p, (_, t) in zip(cal.Poses(), grids))))
    assert r["status"] == _abi.CALIB_OK and r["n_measurements"] == 192 and r["steps"] == 300 and len(h) == 300
    assert err < 1e-9
    assert h[0] > 5.0 and (np.diff(h) < 0).all()
    assert r["rms"] == h[-1] == cal.MeanPixelError()
    cal.close()


def test_recovery_with_distortion_disabled_keeps_w_at_zero(ctx):
    grids = CC.recover_case(CC.TRUTH_NO_DISTORTION)
    cal = calibrator(ctx, grids, disable=True)
    assert cal.Params()[4] == 0.0
    for _ in range(300):
        r = cal.OptimizeOneStep()
        assert r["params"][4] == 0.0 and not np.signbit(r["params"][4])
    err = float(np.abs(r["params"] - np.array(CC.TRUTH_NO_DISTORTION)).max())
    print("without distortion: rms %.3g px, parameter error %.3g" % (r["rms"], err))
    assert err < 1e-9
    one = calibrator(ctx, grids, disable=True)
    assert np.array_equal(one.Optimize(300)["params"], r["params"])
    cal.close()
    one.close()


# ---- call splitting -------------------------------------------------------------------------------------------------------------------
def test_split_calls_and_repeated_runs_give_the_same_bits(ctx):
    grids = CC.recover_case()
    runs = []
    for _ in range(2):
        cal = calibrator(ctx, grids)
        r = cal.Optimize(300)
        runs.append((r["params"].tobytes(), r["history"].tobytes(), cal.Poses().tobytes()))
        cal.close()
    assert runs[0] == runs[1]
    cal = calibrator(ctx, grids)
    hist = np.array([cal.OptimizeOneStep()["rms"] for _ in range(300)])
    assert (cal.Params().tobytes(), hist.tobytes(), cal.Poses().tobytes()) == runs[0]
    cal.close()


# ---- adding images later ----------------------------------------------------------------------------------------------------------------
def test_an_image_added_later_is_guessed_with_the_camera_of_that_moment(ctx):
    grids = CC.recover_case()
    (extra, _), = CC.small_images(1, 30, 21)
    cal = calibrator(ctx, grids, max_images=8)
    cal.Optimize(50)
    now = cal.Params()
    poses_before = cal.Poses()
    assert cal.AddImage(extra) == _abi.CALIB_GUESS_OK and cal.counts() == (5, 4 * 48 + 30)
    poses = cal.Poses()
    assert np.array_equal(poses[:4], poses_before) and np.array_equal(cal.Params(), now)
    st, guess = CR.guess_initial_pose(CR.Camera(now, CC.SIZE), extra)            # the restatement doing the same
    st0, guess0 = CR.guess_initial_pose(CR.Camera(CR.DEFAULT_PARAMS, CC.SIZE), extra)
    assert st == st0 == CR.GUESS_OK
    # the DLT's null vector is known to eps x (s_0 / s_7) of its matrix, in LAPACK's SVD as in the device's Jacobi
    un = CR.Camera(now, CC.SIZE).unproject(np.stack([extra["u"], extra["v"]], 1))
    M = np.zeros((60, 9))
    x, y = extra["gx"].astype(float), extra["gy"].astype(float)
    M[0::2, 0], M[0::2, 1], M[0::2, 2], M[0::2, 6], M[0::2, 7], M[0::2, 8] = x, y, 1, -x * un[:, 0], -y * un[:, 0], -un[:, 0]
    M[1::2, 3], M[1::2, 4], M[1::2, 5], M[1::2, 6], M[1::2, 7], M[1::2, 8] = x, y, 1, -x * un[:, 1], -y * un[:, 1], -un[:, 1]
    sv = np.linalg.svd(M, compute_uv=False)
    bound = max(64.0 * EPS * sv[0] / sv[7] * float(np.abs(guess).max()), 1e-12)
    d = float(np.abs(poses[4] - guess).max())
    print("added later: off the restatement by %.3g (bound %.3g); the default camera's guess is %.3g away" % (d, bound, np.abs(guess0 - guess).max()))
    assert d <= bound and np.abs(guess0 - guess).max() > 1e3 * bound
    # and the restatement's own 50 steps lead to the same camera (50 steps of solver noise at most)
    ref = CC.reference_from(grids)
    for _ in range(50):
        assert CR.condition_number(ref.optimize_one_step()["sv"]) < COND_BAR
    assert np.abs(ref.cam.params - now).max() < 1e-9
    assert cal.Optimize(250)["status"] == _abi.CALIB_OK and np.abs(cal.Params() - np.array(CC.TRUTH)).max() < 1e-9
    cal.close()


def test_a_refused_image_is_not_added(ctx):
    grids = CC.recover_case()
    far = grids[1][0].copy()
    far["u"], far["v"] = 1e300, 1e300        # finite, so the host lets it through; UnProject overflows and the guess is not finite
    assert CR.guess_initial_pose(CR.Camera(CR.DEFAULT_PARAMS, CC.SIZE), far)[0] == CR.GUESS_REFUSED
    cal = host.CameraCalibrator(ctx, 8, 1024)
    status = cal.AddImages([grids[0][0], far, grids[2][0], far, grids[3][0]])
    assert status.tolist() == [0, 1, 0, 1, 0] and cal.counts() == (3, 144)
    only = calibrator(ctx, [grids[0], grids[2], grids[3]])
    assert np.array_equal(cal.Poses(), only.Poses())
    a, b = cal.Optimize(20), only.Optimize(20)
    assert a["status"] == _abi.CALIB_OK and np.array_equal(a["params"], b["params"]) and np.array_equal(cal.Poses(), only.Poses())
    assert np.array_equal(cal.Residuals(1)[0], only.Residuals(1)[0])
    assert cal.AddImages([far]).tolist() == [1] and cal.counts() == (3, 144)     # nothing kept at all
    cal.close()
    only.close()


# ---- residuals and refusals -----------------------------------------------------------------------------------------------------------
def test_residuals_are_the_restatements_projections(ctx):
    grids = CC.recover_case()
    ref = CC.reference_from(grids)
    cal = calibrator(ctx, grids, poses=ref.poses)
    for i in range(4):
        uv, valid = cal.Residuals(i)
        ruv, rvalid = ref.residuals(i)
        assert valid.all() and np.array_equal(valid, rvalid)
        # cx + fx (f x): a handful of roundings of numbers below the image's width, and an atan that is correctly rounded on one side only
        assert np.abs(uv - ruv).max() <= 64 * EPS * 640
    cal.close()


def test_refusals_leave_the_handle_as_it_was(ctx, hip):
    import ctypes as C
    grids = CC.recover_case()
    cal = calibrator(ctx, grids[:3], max_images=4)
    cal.Optimize(5)
    before = snapshot(cal)
    good = grids[3][0]

    def refused(fn, code=-1):
        with pytest.raises(host.PtamError) as e:
            fn()
        assert "(%d)" % code in str(e.value)
        assert snapshot(cal) == before

    refused(lambda: cal.AddImage(good[:3]))                                   # fewer than 4 corners
    twice = good.copy()
    twice["gx"][5], twice["gy"][5] = twice["gx"][9], twice["gy"][9]
    refused(lambda: cal.AddImage(twice))                                      # a grid position twice
    for bad in (np.nan, np.inf):
        nf = good.copy()
        nf["v"][7] = bad
        refused(lambda: cal.AddImage(nf))                                     # non-finite input
    refused(lambda: cal.AddImages([good, good]))                              # more images than the handle holds
    big = np.zeros(65, CR.CORNER_DT)                                          # more corners than the handle holds (64 are left)
    big["gx"], big["u"], big["v"] = np.arange(len(big)), 10.0, 10.0
    refused(lambda: cal.AddImage(big))
    refused(lambda: cal.Optimize(0))                                          # steps < 1
    refused(lambda: cal.Optimize(_abi.CALIB_MAX_STEPS + 1))
    refused(lambda: cal.Reset((0.0, 0.75, 0.5, 0.5, 0.1)))                    # fx of 0
    refused(lambda: cal.Reset((0.5, 0.0, 0.5, 0.5, 0.1)))                     # fy of 0
    refused(lambda: cal.Reset((0.5, 0.75, np.nan, 0.5, 0.1)))
    poses = cal.Poses()
    poses[1, 4] = np.nan
    refused(lambda: cal.SetPoses(poses))
    refused(lambda: cal.Residuals(3))                                         # an image the handle does not have
    refused(lambda: cal.Residuals(-1))
    res = _abi.CalibResult()
    res.steps = -7
    assert hip.calib_optimize(cal.h, 0, C.byref(res), None) == -1 and res.steps == -7   # nothing written
    assert cal.AddImage(good) == _abi.CALIB_GUESS_OK and cal.counts() == (4, 192)        # and the handle still works
    cal.close()
    h = C.c_void_p()
    for mi, mc in ((0, 64), (_abi.CALIB_MAX_IMAGES + 1, 64), (4, 3), (4, _abi.CALIB_MAX_CORNERS + 1)):
        assert hip.calib_create(ctx.h, mi, mc, C.byref(h)) == -1 and not h.value
    empty = host.CameraCalibrator(ctx, 2, 64)
    assert np.array_equal(empty.Params(), np.array(CR.DEFAULT_PARAMS)) and empty.counts() == (0, 0)
    with pytest.raises(host.PtamError) as e:
        empty.Optimize(1)                                                     # PTAM_E_STATE: no images
    assert "(-3)" in str(e.value)
    empty.close()
