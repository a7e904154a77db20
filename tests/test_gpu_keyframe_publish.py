"""-m gpu: the map's keyframes published to the relocaliser on the device — the keyframe section of a ptam_map_snapshot
(ptam_snapshot_keyframes_enable), filled by ptam_rmap_publish, taken by ptam_sbi_bank_take_keyframes — against the composed path it
replaces: a twin bank filled by ptam_sbi_bank_add_batch and ptam_sbi_bank_set_poses from ptam_rmap_download(KF_POSES), and against
tests/sbi_ref.py (the numpy SmallBlurryImage).  Images, poses and results by ==: the make kernel is the one tests/test_gpu_sbi.py
compares with tolerance 0, and everything else is a copy.
The map is the small synthetic one of tests/test_gpu_map_publish.py; the frames are rendered views of tests/sbi_cases.py's plane at
the sizes where the make kernel can go wrong: 160x128 (an SBI of 10x8: smaller than the blur kernel and than a workgroup) and
336x272 (21x17: odd, the stride loop's tail); 640x480 in one case only."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import sbi_cases as SC
from tests import sbi_ref as S
from tests.test_gpu_map_publish import KF_RECORD, moved, synthetic, uploaded
from tests.test_gpu_resident_map import UPLOAD_KEYS

pytestmark = pytest.mark.gpu
E_ARG, E_STATE, E_LIMIT = -1, -3, -4
FRAME = {"R": _abi.HALFSAMPLE_R, "T": _abi.HALFSAMPLE_T}
TINY, ODD, WORK = (160, 128), (336, 272), (640, 480)
N_POINTS = 9
POSE_BYTES = 96                      # se3CfromW of a keyframe: what a take brings down per keyframe
L3_BYTES = 8                         # what a publish sends up per SmallBlurryImage it makes: the level-3 address


@functools.lru_cache(maxsize=None)
def frame(size, k):
    """view k of the plane at `size`: every k another pose along the sequence and another noise seed"""
    return SC.render(size, synth.sequence_pose((5 * k) % 64, 64), 500 + k)


@functools.lru_cache(maxsize=None)
def ref_sbi(size, k, variant):
    return S.make_sbi_from_frame(frame(size, k), 2.5, variant)


@pytest.fixture(scope="module")
def ctxs(hip):
    made = {}

    def get(size, variant="R", tag=0):
        if (size, variant, tag) not in made:
            made[size, variant, tag] = host.Context(lib=hip, size=size, halfsample=FRAME[variant])
        return made[size, variant, tag]

    yield get
    for c in made.values():
        c.close()


class Scene:
    """a resident map of n_kf keyframes (frames 0 .. n_kf - 1 at `size`) on the synthetic tables, a snapshot with the keyframe section
    enabled, a bank that takes and a twin bank that is filled by hand"""

    def __init__(self, ctx, size, n_kf, max_kf=8, cap=8, enable=True):
        self.ctx, self.size = ctx, size
        self.frames = list(range(n_kf))
        self.kfs = [host.KeyFrame(ctx).MakeKeyFrame_Lite(frame(size, k)) for k in self.frames]
        self.map = uploaded(ctx, synthetic(N_POINTS, K=n_kf), kfs=self.kfs)
        self.snap = host.MapSnapshot(ctx, 64)
        if enable:
            self.snap.enable_keyframes(max_kf)
        self.rel = host.Relocaliser(ctx, cap, size=size)
        self.twin = None
        self.cap = cap
        self.closed = []

    def append(self, k, pose=None):
        """AddKeyFrameFromTopOfQueue's table side with a fresh image"""
        kf = host.KeyFrame(self.ctx).MakeKeyFrame_Lite(frame(self.size, k))
        rows = np.zeros(1, host.MAP_KF_ROW_DT)
        p = np.concatenate([np.eye(3).reshape(9), [0.02 * k, -0.01 * k, 0.005]]) if pose is None else pose
        self.map.add_keyframe(p, 0, rows, kf=kf)
        self.kfs.append(kf)
        self.frames.append(k)

    def move(self, t):
        """ApplyGlobalTransformationToMap with a translation: every pose changes"""
        self.map.apply_global_transform(np.concatenate([np.eye(3).reshape(9), np.asarray(t, np.float64)]), rows=False)

    def reupload(self, frames):
        old = self.kfs
        self.frames = list(frames)
        self.kfs = [host.KeyFrame(self.ctx).MakeKeyFrame_Lite(frame(self.size, k)) for k in self.frames]
        h = synthetic(N_POINTS, K=len(self.kfs), seed=11)
        self.map.upload(kfs=self.kfs, **{k: h[k] for k in UPLOAD_KEYS})
        self.closed += old

    def fill_twin(self):
        """the composed path: every keyframe handle and download(KF_POSES) into a fresh bank"""
        if self.twin is not None:
            self.twin.close()
        self.twin = host.Relocaliser(self.ctx, self.cap, size=self.size)
        if self.kfs:
            self.twin.add_batch(self.kfs, self.map.download("poses"))
        return self.twin

    def close(self):
        for o in [self.rel, self.twin, self.snap, self.map] + self.kfs + self.closed:
            if o is not None:
                o.close()


def bank_state(rel):
    """everything a bank holds, as bytes"""
    n = rel.count()
    entries = [rel.read(i) for i in range(n)]
    poses = rel.bank_poses(0, n) if n else np.zeros((0, 12))
    return n, poses.tobytes(), [tuple(e[f].tobytes() for f in ("small", "tmpl", "jacs")) for e in entries]


def assert_same_bank(sc, variant="R", tag=""):
    """the taking bank against the hand-filled twin and the numpy SmallBlurryImage of every keyframe's frame"""
    twin = sc.fill_twin()
    got, want = bank_state(sc.rel), bank_state(twin)
    assert got[0] == want[0] == len(sc.kfs), (tag, got[0], want[0])
    assert got[1] == want[1] == sc.map.download("poses").tobytes(), tag
    assert got[2] == want[2], tag
    assert len(sc.rel.poses) == got[0] and np.array(sc.rel.poses).tobytes() == got[1], tag          # AttemptRecovery's own table followed
    for i, k in enumerate(sc.frames):
        e, r = sc.rel.read(i), ref_sbi(sc.size, k, variant)
        for f in ("small", "tmpl", "jacs"):
            assert np.array_equal(e[f], r[f]), (tag, i, f)


def assert_same_recovery(sc, probe, tag=""):
    kf = host.KeyFrame(sc.ctx).MakeKeyFrame_Lite(probe)
    a, b = sc.rel.AttemptRecovery(kf), sc.twin.AttemptRecovery(kf)
    assert (a["best"], a["good"], a["best_ssd"]) == (b["best"], b["good"], b["best_ssd"]), (tag, a, b)
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["ssd"].tobytes() == b["ssd"].tobytes(), tag
    assert all(np.asarray(a["align"][f]).tobytes() == np.asarray(b["align"][f]).tobytes() for f in a["align"]), tag
    kf.close()


# ---- 1. take equals the composed path ---------------------------------------------------------------------------------------------------
CASES_1 = [(size, v, n) for size in (TINY, ODD) for v in ("R", "T") for n in (1, 2, 5)] + [(WORK, "R", 2)]


@pytest.mark.parametrize("size,variant,n_kf", CASES_1)
def test_take_equals_the_composed_path(ctxs, size, variant, n_kf):
    sc = Scene(ctxs(size, variant), size, n_kf)
    sc.move([0.03, -0.02, 0.01])                    # (poses that are not the upload's)
    pub = sc.map.publish(sc.snap)
    info = sc.snap.keyframes()
    assert (info["enabled"], info["n_kf"], info["n_made"], info["generation"]) == (1, n_kf, n_kf, pub["generation"])
    assert (info["sbi_w"], info["sbi_h"]) == S.sbi_size(*size) and info["blur"] == 2.5 and info["map_id"] == pub["map_id"]
    got = sc.rel.take_keyframes(sc.snap)
    assert (got["changed"], got["n_kf"], got["n_new"], got["generation"], got["map_id"]) == (1, n_kf, n_kf, pub["generation"], pub["map_id"])
    assert_same_bank(sc, variant)
    assert_same_recovery(sc, frame(size, 20))
    sc.close()


# ---- 2. slot rotation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("takes", [(1, 2, 3, 4, 5, 6), (2, 5, 6)])
@pytest.mark.parametrize("size", [TINY, ODD])
def test_slot_rotation(ctxs, size, takes):
    """six publishes, a keyframe appended and the poses moved before each.  A publish takes the first slot that is neither current
    nor being read (snapshot_slots.h); the takes here have returned before it, so the publishes alternate between two slots: from
    the third on a slot lacks the two keyframes appended since it was last written, and a bank that skips publishes appends more
    than one"""
    sc = Scene(ctxs(size), size, 1)
    held, current, slot_holds = 0, -1, [0, 0, 0]
    for p in range(1, 7):
        sc.append(p)
        sc.move([0.01 * p, 0.0, -0.02])
        n_kf = p + 1
        (pub, up, down) = moved(sc.map, lambda: sc.map.publish(sc.snap))
        made = sc.snap.keyframes()["n_made"]
        current = next(i for i in range(3) if i != current)
        assert made == n_kf - slot_holds[current] == (n_kf if p <= 2 else 2), (p, made)
        slot_holds[current] = n_kf
        assert (up, down) == (KF_RECORD * n_kf + L3_BYTES * made, 0), (p, up, down)
        if p in takes:
            got = sc.rel.take_keyframes(sc.snap)
            assert (got["changed"], got["n_kf"], got["n_new"], got["link_bytes"]) == (1, n_kf, n_kf - held, POSE_BYTES * n_kf), (p, got)
            held = n_kf
            assert_same_bank(sc, tag="publish %d" % p)
    assert_same_recovery(sc, frame(size, 20))
    sc.close()


# ---- 3. the unchanged poll --------------------------------------------------------------------------------------------------------------
def test_unchanged_poll(ctxs):
    sc = Scene(ctxs(ODD), ODD, 3)
    pub = sc.map.publish(sc.snap)
    sc.rel.take_keyframes(sc.snap)
    before = bank_state(sc.rel)
    sc.rel.set_poses(1, [np.arange(12.0)])            # set_poses stays allowed; an unchanged poll leaves it
    mine = bank_state(sc.rel)
    again = sc.rel.take_keyframes(sc.snap)
    assert (again["changed"], again["link_bytes"], again["n_new"], again["n_kf"], again["generation"]) == (0, 0, 0, 3, pub["generation"])
    assert bank_state(sc.rel) == mine != before
    sc.map.publish(sc.snap)                            # ... and the next changed take overwrites it
    got = sc.rel.take_keyframes(sc.snap)
    assert (got["changed"], got["n_new"], got["link_bytes"]) == (1, 0, 3 * POSE_BYTES) and bank_state(sc.rel) == before
    sc.close()


# ---- 4. a new epoch ---------------------------------------------------------------------------------------------------------------------
def test_new_epoch_refills_from_entry_zero(ctxs):
    sc = Scene(ctxs(ODD), ODD, 5)
    sc.map.publish(sc.snap)
    sc.rel.take_keyframes(sc.snap)
    epoch = sc.snap.keyframes()["epoch"]
    assert_same_bank(sc)
    sc.reupload([10, 11, 12])                           # fewer keyframes, other images, the same handle and map_id
    pub = sc.map.publish(sc.snap)
    info = sc.snap.keyframes()
    assert (info["n_kf"], info["n_made"], info["epoch"], info["map_id"]) == (3, 3, epoch + 1, pub["map_id"])
    got = sc.rel.take_keyframes(sc.snap)
    assert (got["changed"], got["n_kf"], got["n_new"]) == (1, 3, 3)
    assert_same_bank(sc, tag="after the re-upload")
    # the other slot still holds the old map's images and makes all of the new one's; then there is nothing left to make
    sc.map.publish(sc.snap)
    assert sc.snap.keyframes()["n_made"] == 3
    for _ in range(2):
        sc.map.publish(sc.snap)
        assert sc.snap.keyframes()["n_made"] == 0
    sc.rel.clear()
    assert sc.rel.take_keyframes(sc.snap)["n_new"] == 3
    assert_same_bank(sc, tag="after clear")
    sc.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(hip, ctxs):
    ctx = ctxs(TINY)
    sc = Scene(ctx, TINY, 3, max_kf=3, cap=3, enable=False)
    lib, snap, rel = sc.map.lib, sc.snap, sc.rel
    res = _abi.KeyframesTakeResult()

    def take(r=None, s=None):
        return lib.sbi_bank_take_keyframes((r or rel).h, (s or snap).h, C.byref(res))

    # enable
    assert take() == E_STATE                                                     # not enabled
    assert snap.keyframes()["enabled"] == 0
    assert snap.enable_keyframes(0, check=False) == E_ARG
    wide_ctx = host.Context(lib=hip, size=(4112, 48))                            # an SBI 257 wide: above the side limit
    wide = host.MapSnapshot(wide_ctx, 1)
    assert wide.enable_keyframes(4, check=False) == E_LIMIT and wide.keyframes()["enabled"] == 0
    wide.close()
    wide_ctx.close()
    sc.map.publish(snap)                                                         # generation 1 has no keyframe section
    snap.enable_keyframes(3)
    assert snap.enable_keyframes(3, check=False) == E_STATE                      # already enabled
    assert take() == E_ARG and rel.count() == 0                                  # nothing published since the enable
    fresh = host.MapSnapshot(ctx, 8)
    fresh.enable_keyframes(3)
    assert take(s=fresh) == E_ARG                                                # never published into
    fresh.close()
    # capacity edges: exactly n_kf passes on both sides
    sc.map.publish(snap)
    assert rel.take_keyframes(snap)["n_kf"] == 3
    assert_same_bank(sc)
    before, gen = bank_state(rel), snap.info()["generation"]
    sc.append(3)
    assert sc.map.publish(snap, check=False) == E_LIMIT                          # n_kf = max_keyframes + 1
    assert snap.info()["generation"] == gen and snap.keyframes()["n_kf"] == 3
    assert rel.take_keyframes(snap)["changed"] == 0 and bank_state(rel) == before
    big = host.MapSnapshot(ctx, 8)
    big.enable_keyframes(4)
    sc.map.publish(big)
    assert take(s=big) == E_LIMIT and bank_state(rel) == before                  # n_kf = capacity + 1
    assert rel.take_keyframes(snap)["changed"] == 0                              # ... and it still knows its last take
    roomy = host.Relocaliser(ctx, 4, size=TINY)
    assert roomy.take_keyframes(big)["n_kf"] == 4
    # another frame size; a bank used with another blur
    other = host.Relocaliser(ctxs(ODD), 4, size=ODD)
    assert take(r=other) == E_ARG and other.count() == 0
    other.close()
    hand = host.Relocaliser(ctx, 4, size=TINY)
    hand.add(sc.kfs[0], np.arange(12.0), blur=0.75)
    mine = bank_state(hand)
    assert take(r=hand, s=big) == E_ARG and bank_state(hand) == mine
    hand.clear()
    assert hand.take_keyframes(big)["n_new"] == 4 and bank_state(hand) == bank_state(roomy)
    # after a take the entries are the snapshot's: no adding by hand until clear
    hs = (C.c_void_p * 1)(sc.kfs[0].h.value if hasattr(sc.kfs[0].h, "value") else int(sc.kfs[0].h))
    assert lib.sbi_bank_add(hand.h, sc.kfs[0].h, C.c_double(2.5), None) == E_STATE
    assert lib.sbi_bank_add_batch(hand.h, 1, hs, C.c_double(2.5), None) == E_STATE
    assert bank_state(hand) == bank_state(roomy)
    hand.clear()
    assert hand.count() == 0 and hand.add(sc.kfs[1], np.arange(12.0)) == 0 and hand.count() == 1
    assert np.array_equal(hand.read(0)["tmpl"], ref_sbi(TINY, 1, "R")["tmpl"])
    assert lib.sbi_bank_read(hand.h, 1, None, None, None) == E_ARG and lib.sbi_bank_read(hand.h, -1, None, None, None) == E_ARG
    for o in (hand, roomy, big):
        o.close()
    sc.close()


# ---- 6. traffic -------------------------------------------------------------------------------------------------------------------------
def test_traffic_is_the_stated_formulas_at_both_sizes(ctxs):
    seen = []
    for size in (TINY, ODD):
        sc = Scene(ctxs(size), size, 4)
        plain = host.MapSnapshot(sc.ctx, 64)
        _, up0, down0 = moved(sc.map, lambda: sc.map.publish(plain))              # never enabled: what it is today
        assert (up0, down0) == (KF_RECORD * 4, 0)
        _, up1, down1 = moved(sc.map, lambda: sc.map.publish(sc.snap))            # four images to make
        _, up2, down2 = moved(sc.map, lambda: sc.map.publish(sc.snap))            # another slot: four again
        for _ in range(2):
            sc.map.publish(sc.snap)
        _, up3, down3 = moved(sc.map, lambda: sc.map.publish(sc.snap))            # steady state: nothing to make
        assert (up1, down1, up2, down2, up3, down3) == (KF_RECORD * 4 + L3_BYTES * 4, 0, KF_RECORD * 4 + L3_BYTES * 4, 0, KF_RECORD * 4, 0)
        up_t, down_t = sc.map.traffic()
        got = sc.rel.take_keyframes(sc.snap)
        assert sc.map.traffic() == (up_t, down_t)                                 # a take moves nothing on the map's side
        assert got["link_bytes"] == POSE_BYTES * 4
        seen.append((up1, up3, got["link_bytes"]))
        plain.close()
        sc.close()
    assert seen[0] == seen[1]                                                     # nothing SBI-sized crosses the link


# ---- 7. through the recover batch ---------------------------------------------------------------------------------------------------------
def test_through_the_recover_batch(hip):
    """a camera of tests/test_gpu_track_recover_batch.py, one tracked and one recovery frame: first with the hand-filled bank, then
    with a bank filled by a take from a resident map of the same keyframes"""
    from tests import track_state_ref as T
    from tests.test_gpu_track_recover_batch import RecCamera, _batch, _check_recovered, _check_tracked, _sequence_bank
    cam = RecCamera(hip)
    _sequence_bank(cam)
    n_kf = len(cam.bank_kfs)
    h = synthetic(N_POINTS, K=n_kf)
    h["poses"] = cam.kf_poses.copy()
    m = uploaded(cam.ctx, h, kfs=cam.bank_kfs)
    snap = host.MapSnapshot(cam.ctx, 64)
    snap.enable_keyframes(n_kf)
    m.publish(snap)
    taken = host.Relocaliser(cam.ctx, n_kf, size=cam.size)
    assert taken.take_keyframes(snap)["n_new"] == n_kf
    by_hand = cam.rel
    runs = []
    for rel in (by_hand, taken):
        cam.rel = rel
        cam.restart(cam.poses[0])
        out = []
        res, infos, before = _batch([cam], [0])
        _check_tracked(cam, 0, res[0], infos[0], before[0], "tracked")
        out.append((res[0].tobytes(), infos[0]))
        cam.lose()
        res, infos, before = _batch([cam], [4])
        assert _check_recovered(cam, 4, res[0], infos[0], before[0], "recovered") is not None and infos[0]["branch"] == T.RECOVERED
        out.append((res[0].tobytes(), infos[0]))
        runs.append(out)
    for (ra, ia), (rb, ib) in zip(*runs):
        assert ra == rb
        assert (ia["closest_kf"], ia["closest_kf_dist"], ia["need_new_keyframe"], ia["want_keyframe"]) == \
            (ib["closest_kf"], ib["closest_kf_dist"], ib["need_new_keyframe"], ib["want_keyframe"])
        ga, gb = ia["reloc"], ib["reloc"]
        assert (ga["best"], ga["good"], ga["best_ssd"]) == (gb["best"], gb["good"], gb["best_ssd"]) and ga["pose"].tobytes() == gb["pose"].tobytes()
        assert all(np.asarray(ga["align"][f]).tobytes() == np.asarray(gb["align"][f]).tobytes() for f in ga["align"])
    cam.rel = by_hand
    for o in (taken, snap, m):
        o.close()
    cam.close()


# ---- 8. two threads -----------------------------------------------------------------------------------------------------------------------
def test_two_threads(hip, ctxs):
    """the mapmaker's thread appends a keyframe or moves the poses and publishes, 30 times; the tracker's thread takes until it holds
    generation 30: every take is one whole generation"""
    ROUNDS = 30
    ctx_m, ctx_t = ctxs(TINY, tag="mapmaker"), ctxs(TINY, tag="tracker")
    sc = Scene(ctx_m, TINY, 1, max_kf=ROUNDS, cap=ROUNDS)
    rel = host.Relocaliser(ctx_t, ROUNDS, size=TINY)
    record, taken, errors = {}, [], []
    first_taken = threading.Event()

    def mapmaker():
        try:
            for r in range(1, ROUNDS + 1):
                if r % 2:
                    sc.append(r % 7)
                else:
                    sc.move([0.001 * r, 0.002, -0.001 * r])
                pub = sc.map.publish(sc.snap)
                record[pub["generation"]] = sc.map.download("poses").copy()
                if r == 1:      # the tracker holds a generation before the others come: it sees at least two, however the threads are scheduled
                    first_taken.wait(30)
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    def tracker():
        try:
            res = _abi.KeyframesTakeResult()
            gen = 0
            while gen < ROUNDS and not errors:
                rc = rel.lib.sbi_bank_take_keyframes(rel.h, sc.snap.h, C.byref(res))
                if rc == E_ARG and gen == 0:      # nothing published yet
                    continue
                rel.ctx._check(rc, "sbi_bank_take_keyframes")
                if res.changed:
                    gen = res.generation
                    taken.append((gen, res.n_kf, rel.bank_poses(0, res.n_kf).copy()))
                    first_taken.set()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
            first_taken.set()

    threads = [threading.Thread(target=f) for f in (mapmaker, tracker)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads)
    assert taken and taken[-1][0] == ROUNDS and len(taken) >= 2
    gens = [g for g, _, _ in taken]
    assert gens == sorted(set(gens))
    for gen, n_kf, poses in taken:
        assert n_kf == len(record[gen]) and poses.tobytes() == record[gen].tobytes(), gen
    # the bank the tracker ended with, image by image
    assert rel.count() == len(sc.kfs)
    for i, k in enumerate(sc.frames):
        assert np.array_equal(rel.read(i)["tmpl"], ref_sbi(TINY, k, "R")["tmpl"]), i
    rel.close()
    sc.close()
