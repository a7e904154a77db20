"""CPU: known answers for tests/sbi_ref.py, the numpy restatement of the SmallBlurryImage the device is compared against
(tests/test_gpu_sbi.py) — so that the restatement is not its own judge —, the guards of the shared fixtures (tests/sbi_cases.py),
and the library's new symbols."""
import ctypes
import os

import numpy as np
import pytest

from ptam_cg_amd import _abi, synth
from tests import sbi_cases as SC
from tests import sbi_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sbi_create", "sbi_destroy", "sbi_make", "sbi_size", "sbi_read", "sbi_calc_rotation", "sbi_bank_create",
               "sbi_bank_destroy", "sbi_bank_add", "sbi_bank_add_batch", "sbi_bank_count", "relocalise", "rotation_estimator_create",
               "rotation_estimator_destroy", "rotation_estimator_reset", "motion_predict_sbi", "motion_recover", "track_frame_sbi"]


def test_library_exports_the_sbi_symbols():
    path = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(path)
    assert [n for n in NEW_SYMBOLS if not hasattr(lib, "ptam_" + n) or n not in _abi.DECLARED] == []
    assert ctypes.sizeof(_abi.SbiAlignment) == 17 * 8 + 16 and ctypes.sizeof(_abi.RelocResult) == 8 + 8 + 96 + 152


@pytest.mark.parametrize("sigma", [0.75, 2.5, 5.0])
def test_blurred_delta(sigma):
    wt, k = S.gaussian_weights(sigma)
    assert k == int(np.ceil(3 * sigma)) and len(wt) == 2 * k + 1 and abs(wt.sum() - 1.0) < 1e-15 and np.array_equal(wt, wt[::-1])
    im = np.zeros((30, 40), np.float32)
    im[15, 20] = 1.0
    out = S.convolve_gaussian(im, sigma)
    full = np.zeros((30 + 2 * k, 40 + 2 * k))
    full[15:15 + 2 * k + 1, 20:20 + 2 * k + 1] = np.outer(wt, wt)      # the outer product of the taps around (20, 15)
    inside = full[k:k + 30, k:k + 40]
    assert np.array_equal(out, inside.astype(np.float32))
    if 15 + k < 30:
        assert abs(float(out.astype(np.float64).sum()) - 1.0) < 1e-6      # all of it inside: sums to 1 (float32 rounding of 1 200 values)
    im = np.zeros((30, 40), np.float32)
    im[0, 0] = 1.0
    corner = S.convolve_gaussian(im, sigma)
    kept = np.outer(wt[k:], wt[k:])                                       # the quadrant that stays inside; the rest is lost, not folded back
    hh, ww = min(k + 1, 30), min(k + 1, 40)
    assert np.array_equal(corner[:hh, :ww], kept[:hh, :ww].astype(np.float32)) and not corner[hh:].any() and not corner[:, ww:].any()
    assert abs(float(corner.astype(np.float64).sum()) - kept[:hh, :ww].sum()) < 1e-6
    assert abs(kept.sum() - wt[k:].sum() ** 2) < 1e-15 and kept.sum() < 0.6     # ((1 + w0) / 2)^2 of the weight stays


@pytest.mark.parametrize("blur", SC.BLURS)
def test_self_alignment_is_the_identity(blur):
    a = SC.reference("work", blur, "R")["cur"]
    r = S.calc_rotation(a, a, 6)
    assert np.array_equal(r["R"], np.eye(2)) and not r["t"].any() and r["score"] == 0.0 and r["mean_offset"] == 0.0
    assert len(r["updates"]) == 6 and not np.array(r["updates"]).any() and r["iterations_done"] == 6 and not r["degenerate"]
    assert r["n_used"] == (40 - 3) * (30 - 3)              # the identity walk puts the last row and column outside: p < w - 1
    assert np.array_equal(r["rotation"], np.eye(3))        # to the last bit


def test_synthetic_warp_is_recovered():
    """a template warped by a known SE2 with the restatement's own transform: the aligner finds the inverse motion"""
    tgt = SC.reference("work", 2.5, "R")["tgt"]
    th, tr = 0.03, np.array([0.7, -0.4])
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([20.0, 15.0])
    warped, _, _ = S.transform(tgt["tmpl"], R, (c + tr) - R @ c)    # W * (R, tr) * W^-1
    keep = warped > -1e20
    cur = np.where(keep, warped, np.float32(0))
    # current(x) = target(A x): aligning current to the target needs A^-1
    r = S.iterate(cur, tgt, 6)
    Ri, ti = R.T, -R.T @ tr
    print("SE2 recovered:", np.abs(r["R"] - Ri).max(), np.abs(r["t"] - ti).max())
    assert np.abs(r["R"] - Ri).max() < 2e-3 and np.abs(r["t"] - ti).max() < 0.05 and not r["degenerate"]


def test_se3_from_se2():
    assert np.array_equal(S.se3_from_se2(np.eye(2), np.zeros(2), (40, 30)), np.eye(3))
    for th in (0.01, 0.05, -0.1):
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        # an in-plane turn about the CENTRE pixel: se2CtoC is applied to offsets from the centre, so its translation is zero
        w = S.so3_ln(S.se3_from_se2(R, np.zeros(2), (40, 30)))
        print(th, w)
        # the default camera's principal point is 0.8 / 1.5 pixels from the SBI's centre: the axis leans by that much over the focal length
        assert abs(np.linalg.norm(w) - abs(th)) < 0.01 * abs(th) and abs(w[2] - th) < 0.01 * abs(th)
        assert np.linalg.norm(w[:2]) < 0.05 * abs(th)


# Rotation-vector error of the estimator (sigma 0.75, 6 iterations) as a fraction of |w| on the views below, measured with this file:
# 0.021, 0.018, 0.026, 0.020, 0.036, 0.064 — the largest 0.064 (the smallest turn, 0.025 rad about y: sensor noise and the 16-pixel
# cells of the SBI weigh most there).  The bound is twice the largest.
TRUTH_W = [(0.02, 0.012, 0.01), (0.0, 0.0, 0.05), (0.03, -0.04, 0.06), (-0.05, 0.02, -0.1), (0.06, 0.05, 0.0), (0.0, -0.025, 0.0)]
TRUTH_BOUND = 0.128


def test_truth_on_rendered_views():
    """two 640x480 views from one camera centre, a pure rotation w apart, sensor noise on both"""
    pose = synth.sequence_pose(3, 64)
    last = S.make_sbi_from_frame(SC.render((640, 480), pose, 5), 0.75)
    worst = 0.0
    for i, w in enumerate(TRUTH_W):
        w = np.array(w)
        assert 0.025 <= np.linalg.norm(w) <= 0.12
        this = S.make_sbi_from_frame(SC.render((640, 480), SC.rotated(pose, w), 50 + i), 0.75)
        r = S.calc_rotation(this, last, 6)
        frac = np.linalg.norm(S.so3_ln(r["rotation"] @ S.so3_exp(w).T)) / np.linalg.norm(w)
        worst = max(worst, frac)
        print(w, "error / |w| = %.4f" % frac, "n_used", r["n_used"])
        assert r["edge_gap"] >= 1e-9 and r["pivot_ratio"] >= 1e-6
        # the prediction from a standing start: without the estimator it is the last pose, off by w itself
        true = SC.rotated(pose, w)
        pred = S.predict_sbi(pose, np.zeros(6), r["rotation"])
        err = lambda p: np.linalg.norm(S.so3_ln(p[:9].reshape(3, 3) @ true[:9].reshape(3, 3).T))
        assert abs(err(pose) - np.linalg.norm(w)) < 1e-9 and err(pred) < 0.25 * err(pose)
        assert np.abs(pred[9:] - true[9:]).max() < 0.25 * np.abs(pose[9:] - true[9:]).max()
    assert worst <= TRUTH_BOUND


@pytest.mark.parametrize("name", list(SC.CASES))
@pytest.mark.parametrize("blur", SC.BLURS)
@pytest.mark.parametrize("variant", SC.VARIANTS)
def test_fixture_guards(name, blur, variant):
    """what the device comparison relies on, on the restatement alone: no in / out decision of the warp and no pivot near its threshold"""
    size = SC.CASES[name][0]
    w, h = S.sbi_size(*size)
    r = SC.reference(name, blur, variant)
    a = r["align"]
    assert r["cur"]["small"].shape == (h, w) and np.isfinite(a["score"]) and np.isfinite(a["rotation"]).all()
    if name == "blank":
        assert a["degenerate"] == 1 and a["iterations_done"] == 0 and a["n_used"] == (w - 3) * (h - 3) and a["score"] == 0.0
        assert np.array_equal(a["R"], np.eye(2)) and not a["t"].any() and np.array_equal(a["rotation"], np.eye(3))
        return
    assert a["degenerate"] == 0 and a["iterations_done"] == 6
    assert a["edge_gap"] >= 1e-9 and a["pivot_ratio"] >= 1e-6
    if name == "far":
        assert a["n_used"] < (w - 3) * (h - 3) - 40          # warped samples left the image: the -9e20 path
    if name in ("work", "far"):                              # the fixtures are alignments that work, not noise
        assert np.linalg.norm(S.so3_ln(a["rotation"]) - np.array(SC.CASES[name][1])) < 0.1 * np.linalg.norm(SC.CASES[name][1])


def test_bank_nearest_keyframe_has_the_lowest_ssd():
    kfs, poses, cur = SC.bank_views()
    r = SC.bank_reference()
    true = synth.sequence_pose(SC.BANK_CURRENT_FRAME, 64)
    centre = lambda p: -p[:9].reshape(3, 3).T @ p[9:]
    dist = [np.linalg.norm(centre(p) - centre(true)) + np.linalg.norm(S.so3_ln(p[:9].reshape(3, 3) @ true[:9].reshape(3, 3).T)) for p in poses]
    assert int(np.argmin(dist)) == SC.BANK_NEAREST == r["best"] and r["good"]
    assert r["align"]["edge_gap"] >= 1e-9 and r["align"]["pivot_ratio"] >= 1e-6 and not r["align"]["degenerate"]
    s = np.sort(r["ssd"])
    print("runner-up margin", s[1] / s[0])
    assert s[1] >= 1.01 * s[0]
    # the recovered pose is nearer to the truth than the keyframe's own
    rot_err = lambda p: np.linalg.norm(S.so3_ln(p[:9].reshape(3, 3) @ true[:9].reshape(3, 3).T))
    assert rot_err(r["pose"]) < rot_err(poses[r["best"]])
    # sub-banks the device test uses: one entry; two entries
    assert SC.bank_reference("R", 1, 5)["best"] == 0 and SC.bank_reference("R", 2, 4)["best"] == 1


def test_closed_loop_composition_keeps_tracking(oracle):
    """the expectation of tests/test_gpu_sbi_track.py's closed loop — the restatement's rotation, the prediction with it, the
    checker's TrackMap — stays on the trajectory on every one of the 8 frames (n_meas >= 50 is the bench's mark of a lost frame)"""
    poses = SC.tracking_sequence()[1]
    loop = SC.closed_loop_on_oracle(oracle)
    assert len(loop) == SC.TRACK_FRAMES
    for k, f in enumerate(loop):
        print(k, f["result"]["n_meas"], int(f["result"]["did_coarse"]), "%.2e" % np.abs(f["result"]["pose"] - poses[k]).max())
        assert f["result"]["n_meas"] >= 50 and np.abs(f["result"]["pose"] - poses[k]).max() < 3e-3
    assert np.array_equal(SC.sequence_rotations()[0], np.eye(3))             # frame 0 is aligned against itself
