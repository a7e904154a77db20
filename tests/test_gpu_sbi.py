"""-m gpu: the SmallBlurryImage on the device (ptam_sbi_*, ptam_relocalise) against its numpy restatement (tests/sbi_ref.py) on the
fixtures of tests/sbi_cases.py, whose guards tests/test_sbi_ref.py checks on the restatement alone.  Discrete results (mimSmall, the
pixels used, the iterations done, the nearest keyframe) are compared exactly, continuous ones under the tolerances below; every
figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import sbi_cases as SC
from tests import sbi_ref as S

pytestmark = pytest.mark.gpu

# Device against restatement, max |a - b| / max |b| per quantity, measured on an MI355X over every case, both blurs and both halfSample
# variants (docs/LOG_sbi.md has the table).  The tolerance is ten times the largest figure, the margin the plane-aligner and
# homography tests use.
# Template and Jacobians: 0 in every case — the device's blur is the restatement's operation by operation (the same tap order, no
# contraction, the weights from the same libm) — so they are compared exactly, like mimSmall.
# TOL_ALIGN: SE2 rotation <= 3.6e-16, translation <= 2.11e-14 (the largest: tiny at sigma 2.5, 34 pixels, a pivot ratio of 0.08),
# score <= 1.6e-15, mean offset <= 3.1e-15, rotation <= 5.6e-16; the relocaliser's pose <= 9.0e-17.  The device sums per thread with
# stride 256, then lanes, then waves, its products contracted into FMAs; the restatement sums in raster order without.  The float32
# rounding of the warped image, expected to dominate, did not show: no warped pixel sat on a rounding boundary in these fixtures.
# TOL_SSD: the bank's SSDs <= 8.2e-15 (1 200 squares, tree against sequential order).
# All far below 1e-6, the project's bundle tolerance: nothing to explain.
TOL_ALIGN = 2.2e-13
TOL_SSD = 8.2e-14

FRAME = {"R": _abi.HALFSAMPLE_R, "T": _abi.HALFSAMPLE_T}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / (scale if scale > 0 else 1.0))


@pytest.fixture(scope="module")
def ctxs(hip):
    made = {}

    def get(size, variant):
        if (size, variant) not in made:
            made[size, variant] = host.Context(lib=hip, size=size, halfsample=FRAME[variant])
        return made[size, variant]

    yield get
    for c in made.values():
        c.close()


def _run(ctx, name, blur):
    """the device's MakeFromKF of both views and CalcSBIRotation(current, target) -> (cur, tgt, align, align again)"""
    cur_im, tgt_im = SC.views(name)
    kf = host.KeyFrame(ctx)
    cur, tgt = host.SmallBlurryImage(ctx), host.SmallBlurryImage(ctx)
    cur.MakeFromKF(kf.MakeKeyFrame_Lite(cur_im), blur)
    tgt.MakeFromKF(kf.MakeKeyFrame_Lite(tgt_im), blur)
    out = cur.read(), tgt.read(), cur.CalcSBIRotation(tgt, 6), cur.CalcSBIRotation(tgt, 6)
    for o in (cur, tgt, kf):
        o.close()
    return out


@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("blur", SC.BLURS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_device_matches_restatement(ctxs, name, blur, variant):
    size = SC.CASES[name][0]
    ref = SC.reference(name, blur, variant)
    cur, tgt, al, again = _run(ctxs(size, variant), name, blur)
    ra = ref["align"]
    for d, r in ((cur, ref["cur"]), (tgt, ref["tgt"])):
        assert d["small"].shape == r["small"].shape == S.sbi_size(*size)[::-1] and np.array_equal(d["small"], r["small"])
    make = dict(tmpl=max(_rel(cur["tmpl"], ref["cur"]["tmpl"]), _rel(tgt["tmpl"], ref["tgt"]["tmpl"])),
                jacs=max(_rel(cur["jacs"], ref["cur"]["jacs"]), _rel(tgt["jacs"], ref["tgt"]["jacs"])))
    align = dict(R=_rel(al["R"], ra["R"]), t=_rel(al["t"], ra["t"]), score=_rel(al["score"], ra["score"]),
                 mean_offset=_rel(al["mean_offset"], ra["mean_offset"]), rotation=_rel(al["rotation"], ra["rotation"]))
    print(name, blur, variant, "n_used", al["n_used"], {k: "%.2e" % v for k, v in {**make, **align}.items()})
    assert np.isfinite([al["score"], al["mean_offset"]]).all() and np.isfinite(al["R"]).all() and np.isfinite(al["rotation"]).all()
    assert (al["n_used"], al["iterations_done"], al["degenerate"]) == (ra["n_used"], ra["iterations_done"], ra["degenerate"])
    assert max(make.values()) == 0.0, make
    assert max(align.values()) <= TOL_ALIGN, align
    if name == "blank":
        assert al["degenerate"] == 1 and np.array_equal(al["R"], np.eye(2)) and not al["t"].any() and al["score"] == 0.0
        assert np.array_equal(al["rotation"], np.eye(3))
    # a second run gives the same bits
    assert all(np.array_equal(np.asarray(al[k]), np.asarray(again[k])) for k in al)


def test_self_alignment_is_the_exact_identity(ctxs):
    ctx = ctxs((640, 480), "R")
    kf = host.KeyFrame(ctx).MakeKeyFrame_Lite(SC.views("work")[0])
    a = host.SmallBlurryImage(ctx).MakeFromKF(kf, 0.75)
    al = a.CalcSBIRotation(a, 6)
    assert np.array_equal(al["R"], np.eye(2)) and not al["t"].any() and al["score"] == 0.0 and np.array_equal(al["rotation"], np.eye(3))
    assert (al["n_used"], al["iterations_done"], al["degenerate"]) == (37 * 27, 6, 0)
    a.close()
    kf.close()


@functools.lru_cache(maxsize=None)
def _bank_case(which):
    """-> (keyframe indices into SC.bank_views(), the restatement's result); `which`: one, two_same, two, seventeen"""
    idx = {"one": [5], "two_same": [5, 5], "two": [4, 5], "seventeen": list(range(16)) + [5]}[which]
    kfs, poses, cur = SC.bank_views()
    bank = [S.make_sbi_from_frame(kfs[i], 2.5) for i in sorted(set(idx))]
    by = dict(zip(sorted(set(idx)), bank))
    ref = S.relocalise([by[i] for i in idx], poses[idx], S.make_sbi_from_frame(cur, 2.5))
    # the guards, on the restatement alone, before anything is compared: no in / out decision of the warp and no pivot near its
    # threshold, and a runner-up among the DIFFERENT keyframes that is clearly behind
    assert ref["align"]["edge_gap"] >= 1e-9 and ref["align"]["pivot_ratio"] >= 1e-6 and not ref["align"]["degenerate"]
    others = [v for i, v in zip(idx, ref["ssd"]) if i != idx[ref["best"]]]
    assert not others or min(others) >= 1.01 * ref["ssd"][ref["best"]]
    return idx, ref


def hip_refuses_overfull(rel, kfs):
    """a batch larger than the room left is refused with PTAM_E_LIMIT"""
    two = (C.c_void_p * 2)(kfs[0].h.value, kfs[0].h.value)
    return rel.lib.sbi_bank_add_batch(rel.h, 2, two, 2.5, None) == -4


@pytest.mark.parametrize("which", ["one", "two_same", "two", "seventeen"])
def test_relocalise_matches_restatement(ctxs, which):
    """banks of 1, 2 and 17 entries; equal entries (two_same, and keyframe 5 again as the seventeenth) give the first index"""
    ctx = ctxs((640, 480), "R")
    idx, ref = _bank_case(which)
    kfs, poses, cur = SC.bank_views()
    assert ref["best"] == {"one": 0, "two_same": 0, "two": 1, "seventeen": 5}[which]
    rel = host.Relocaliser(ctx, capacity=len(idx))
    kf = host.KeyFrame(ctx)
    for i in idx:
        assert rel.add(kf.MakeKeyFrame_Lite(kfs[i]), poses[i]) == rel.count() - 1
        ctx.sync()
    r = rel.AttemptRecovery(kf.MakeKeyFrame_Lite(cur))
    ra = ref["align"]
    figures = dict(ssd=_rel(r["ssd"], ref["ssd"]), best_ssd=_rel(r["best_ssd"], ref["ssd"][ref["best"]]), pose=_rel(r["pose"], ref["pose"]),
                   score=_rel(r["align"]["score"], ra["score"]), rotation=_rel(r["align"]["rotation"], ra["rotation"]))
    print(which, r["best"], {k: "%.2e" % v for k, v in figures.items()})
    assert r["best"] == ref["best"] and r["good"] == ref["good"] is True and r["best_ssd"] == r["ssd"][r["best"]]
    assert (r["align"]["n_used"], r["align"]["iterations_done"]) == (ra["n_used"], ra["iterations_done"])
    assert max(figures["ssd"], figures["best_ssd"]) <= TOL_SSD and max(figures["pose"], figures["score"], figures["rotation"]) <= TOL_ALIGN
    R = r["align"]["rotation"]
    K = poses[idx[r["best"]]]
    assert _rel(r["pose"], np.concatenate([(R @ K[:9].reshape(3, 3)).reshape(9), R @ K[9:]])) <= 1e-15    # pose = rotation * kf_pose
    # good follows max_score on both sides of the measured score
    s = r["align"]["score"]
    assert rel.AttemptRecovery(kf, max_score=s * 1.001)["good"] and not rel.AttemptRecovery(kf, max_score=s * 0.999)["good"]
    assert not rel.AttemptRecovery(kf, max_score=s)["good"]                       # strictly below
    again = rel.AttemptRecovery(kf)
    # the same bank filled by ONE make launch (ptam_sbi_bank_add_batch) holds the same images
    many = [host.KeyFrame(ctx).MakeKeyFrame_Lite(kfs[i]) for i in idx]
    rel2 = host.Relocaliser(ctx, capacity=len(idx) + 1)
    assert rel2.add_batch(many, poses[idx]) == 0 and rel2.count() == len(idx)
    r2 = rel2.AttemptRecovery(kf)
    assert r2["ssd"].tobytes() == r["ssd"].tobytes() and r2["pose"].tobytes() == r["pose"].tobytes() and r2["best"] == r["best"]
    assert hip_refuses_overfull(rel2, many) and rel2.count() == len(idx)
    rel2.close()
    for k in many:
        k.close()
    assert again["ssd"].tobytes() == r["ssd"].tobytes() and again["pose"].tobytes() == r["pose"].tobytes()
    rel.close()
    kf.close()


def test_refusals(hip, ctxs):
    ctx = ctxs((160, 128), "R")
    kf = host.KeyFrame(ctx).MakeKeyFrame_Lite(SC.views("tiny")[0])
    a, b = host.SmallBlurryImage(ctx), host.SmallBlurryImage(ctx)
    out = _abi.SbiAlignment()
    h = C.c_void_p()
    assert hip.sbi_create(ctx.h, 40, 40, C.byref(h)) == -1                        # a 2x2 image has no interior
    assert hip.sbi_create(ctx.h, 1 << 13, 1 << 13, C.byref(h)) == -4              # above 4096 pixels
    assert hip.sbi_read(a.h, None, None, None) == -3                              # nothing made yet
    assert hip.sbi_calc_rotation(a.h, b.h, 6, C.byref(out)) == -3
    for blur in (0.0, -1.0, 5.5, float("nan")):
        assert hip.sbi_make(a.h, kf.h, blur) == -1
    assert hip.sbi_make(a.h, None, 0.75) == -1 and hip.sbi_make(None, kf.h, 0.75) == -1
    big = host.Context(lib=hip, size=(336, 272))
    other = host.KeyFrame(big)
    assert hip.sbi_make(a.h, other.h, 0.75) == -1                                 # a keyframe of another frame size
    other.close()
    big.close()
    assert hip.sbi_make(a.h, kf.h, 5.0) == 0 and hip.sbi_make(b.h, kf.h, 5.0) == 0
    for its in (0, -1, 65):
        assert hip.sbi_calc_rotation(a.h, b.h, its, C.byref(out)) == -1
    assert hip.sbi_calc_rotation(a.h, b.h, 1, C.byref(out)) == 0 and out.iterations_done == 1 and out.score == 0.0
    bank = C.c_void_p()
    assert hip.sbi_bank_create(ctx.h, 160, 128, 0, C.byref(bank)) == -1
    assert hip.sbi_bank_create(ctx.h, 160, 128, 1, C.byref(bank)) == 0
    res, pose = _abi.RelocResult(), np.zeros(12)
    assert hip.relocalise(bank, a.h, kf.h, host._ptr(pose), 2.5, 9e6, C.byref(res), None) == -3      # an empty bank
    assert hip.sbi_bank_add(bank, kf.h, 2.5, None) == 0 and hip.sbi_bank_add(bank, kf.h, 2.5, None) == -4    # full
    assert hip.relocalise(bank, a.h, kf.h, None, 2.5, 9e6, C.byref(res), None) == -1
    assert hip.relocalise(bank, a.h, kf.h, host._ptr(pose), 2.5, 9e6, C.byref(res), None) == 0 and res.best == 0 and res.best_ssd == 0.0
    assert hip.sbi_bank_destroy(bank) == 0
    for o in (a, b, kf):
        o.close()
