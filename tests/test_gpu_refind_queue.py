"""-m gpu: ptam_rmap_refind_queue — the re-find of the resident queues with its work lists built on the device (the good new points
compacted and ranked, the failure pairs sorted) — against ptam_rmap_refind(work = NULL), whose lists the host builds, on a second
handle that holds the same map, each through a fresh finder.  Results and counts by ==, tables and the queue afterwards by
tobytes(), the bytes over the host link with the formula of the header.
Queue lengths: 0, 1, 2, the wave (63, 64, 65), the tile T of the compaction and of the sort (T - 1, T, T + 1) and 2 T + 3 (a second
merge pass).  Three keyframes, so that the longest new queue makes 6153 pairs."""
import threading

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import map_edit_ref as E
from tests import map_refind_ref as F
from tests.test_gpu_resident_map import check_invariants, same_tables
from tests.test_gpu_resident_map_refind import scene_map, uploaded

pytestmark = pytest.mark.gpu
NEW_POINTS, QUEUE = _abi.MAP_REFIND_NEW_POINTS, _abi.MAP_REFIND_FAILURE_QUEUE
T = 1024                                     # MT_TILE (ptam_cg_amd/csrc/maptables_internal.h)
LENGTHS = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
K = 3


@pytest.fixture(scope="module")
def dev(hip):
    ctx = host.Context(lib=hip)
    scene = F.make_scene(ctx, n_kf=K)
    # the scene's 1244 points twice: a new queue of 2 T + 3 entries names no point twice.  The copies are in no table
    scene["points"] = np.concatenate([scene["points"], scene["points"]])
    # before anything is compared: the reference path visits pairs and finds some on this scene, in both modes, so an empty visit
    # cannot pass for agreement (each case with good points asserts its own n_pairs > 0 in both_ways)
    points, q = new_queue_case(scene, 65, "random", "some", seed=1)
    m = uploaded(ctx, scene_map(scene, points, new_queue=q, failure=failure_case(scene, 65, "random", seed=2)), scene["kfs"])
    rf = host.ReFinder(ctx)
    for mode in (NEW_POINTS, QUEUE):
        r = m.refind(rf, mode, lists=False)
        assert r["n_pairs"] > 0 and r["n_found"] > 0, (mode, r)
    rf.close()
    m.close()
    yield ctx, scene
    scene["close"]()
    ctx.close()


def ordered(a, order, rng):
    if order == "ascending":
        return a
    if order == "reversed":
        return a[::-1].copy()
    return a[rng.permutation(len(a))]


def new_queue_case(scene, n, order, bad, seed):
    """n distinct points in the given order of their indices; bad: "some" (a seeded sixth), "none", "all" -> (points, queue)"""
    rng = np.random.default_rng(seed)
    N = len(scene["points"])
    q = ordered(np.sort(rng.choice(N, size=n, replace=False)).astype(np.int32), order, rng)
    points = scene["points"].copy()
    share = {"some": 1.0 / 6, "none": 0.0, "all": 1.0}[bad]
    points["bad"][q[rng.random(n) < share]] = 1
    if bad == "some" and n >= 2:               # (both kinds are there, at any length)
        points["bad"][q[0]], points["bad"][q[-1]] = 1, 0
    return points, q


def failure_case(scene, n, order, seed):
    """n pairs: sorted, reversed, random (no pair twice), all of one keyframe, or with every third pair repeated"""
    rng = np.random.default_rng(seed)
    N = len(scene["points"])
    q = np.zeros(n, E.PAIR_DT)
    flat = np.sort(rng.choice(K * N, size=n, replace=False))
    q["kf"], q["point"] = flat // N, flat % N
    if order == "one_keyframe":
        q["kf"] = 1
        return q[rng.permutation(n)]
    if order == "repeated":
        q[2::3] = q[0::3][:len(q[2::3])]
        return q[rng.permutation(n)]
    return ordered(q, {"sorted": "ascending"}.get(order, order), rng)


def both_ways(dev, h, mode, good, **kw):
    """the map of h on two handles: refind(work = NULL) on one, refind_queue on the other -> the reference's result"""
    ctx, scene = dev
    a, b = uploaded(ctx, h, scene["kfs"]), uploaded(ctx, h, scene["kfs"])
    fa, fb = host.ReFinder(ctx), host.ReFinder(ctx)
    ref = a.refind(fa, mode, lists=False, **kw)
    if good:
        assert ref["n_pairs"] > 0
    n_queue = len(h["new_queue"] if mode == NEW_POINTS else h["failure"])
    runs = (int((h["bad"][h["new_queue"]] == 0).sum()) if mode == NEW_POINTS else n_queue) > 0   # there is a pair to visit
    up0, down0 = b.traffic()
    got = b.refind_queue(fb, mode, **kw)
    up, down = b.traffic()
    assert got == ref
    ta, tb = a.tables(), b.tables()
    same_tables(tb, ta)
    check_invariants(tb)
    assert a.counts() == b.counts()
    # include/ptam_hip.h: the level records up; the count of good points and the counts down (no call here stops after a point)
    assert 0 < up - up0 <= _abi.RMAP_KF_RECORD_BYTES * K if runs else up == up0
    assert down - down0 == (4 if mode == NEW_POINTS and n_queue > 0 else 0) + (16 if runs else 0)
    for f in (fa, fb):
        f.close()
    a.close()
    b.close()
    return ref


@pytest.mark.parametrize("order", ["ascending", "reversed", "random"])
@pytest.mark.parametrize("n", LENGTHS)
def test_new_points_from_the_resident_queue(dev, n, order):
    points, q = new_queue_case(dev[1], n, order, "some", seed=n + 1)
    h = scene_map(dev[1], points, new_queue=q)
    ref = both_ways(dev, h, NEW_POINTS, good=n >= 2)
    n_bad = int(points["bad"][q].sum())
    assert ref["points_consumed"] == n and ref["n_bad_points"] == n_bad and ref["n_pairs"] == K * (n - n_bad) and ref["stopped"] == 0
    if n >= 2:
        assert 0 < n_bad < n


@pytest.mark.parametrize("bad", ["none", "all"])
@pytest.mark.parametrize("n", [1, 65, T + 1])
def test_new_points_none_bad_and_all_bad(dev, n, bad):
    points, q = new_queue_case(dev[1], n, "random", bad, seed=n + 7)
    ref = both_ways(dev, scene_map(dev[1], points, new_queue=q), NEW_POINTS, good=bad == "none")
    assert ref["n_bad_points"] == (n if bad == "all" else 0) and ref["points_consumed"] == n


@pytest.mark.parametrize("order", ["sorted", "reversed", "random", "one_keyframe", "repeated"])
@pytest.mark.parametrize("n", LENGTHS)
def test_failure_queue_from_the_resident_queue(dev, n, order):
    fq = failure_case(dev[1], n, order, seed=n + 3)
    ref = both_ways(dev, scene_map(dev[1], failure=fq), QUEUE, good=n > 0)
    assert ref["n_pairs"] == n
    if order == "repeated" and n >= 3:
        assert ref["n_skipped"] >= len(fq[2::3])


@pytest.mark.parametrize("mode", [NEW_POINTS, QUEUE])
@pytest.mark.parametrize("n", [0, 65])
def test_a_stop_flag_raised_before_the_call(dev, mode, n):
    points, q = new_queue_case(dev[1], n, "random", "some", seed=5)
    h = scene_map(dev[1], points, new_queue=q, failure=failure_case(dev[1], n, "random", seed=6))
    ref = both_ways(dev, h, mode, good=False, stop=np.ones(1, np.uint8))
    assert ref["n_pairs"] == 0 and ref["stopped"] == (1 if n else 0) and ref["points_consumed"] == 0


@pytest.mark.parametrize("mode", [NEW_POINTS, QUEUE])
def test_several_passes(dev, mode):
    points, q = new_queue_case(dev[1], 65, "random", "some", seed=8)
    h = scene_map(dev[1], points, new_queue=q, failure=failure_case(dev[1], 200, "repeated", seed=9))
    ref = both_ways(dev, h, mode, good=True, max_pairs_per_pass=32)
    assert ref["n_pairs"] > 3 * 32


def test_new_points_stopped_on_the_way(dev):
    """The flag goes up from a second thread while the passes, one point each, are being enqueued.  Wherever the walk ends, the
    result agrees with the queue: the entries up to the last visited point are popped, the bad ones among them counted, and the
    one word that says so came down.  Where it ends is the clock's: what is asserted holds for every end, and the branch that reads
    the visited point's entry number runs only when the flag lands between two of the 2 051 passes.  When it lands before the first
    or after the last, this test passes without that branch, which no other test reaches (a flag raised before the call visits no
    point)."""
    ctx, scene = dev
    points, q = new_queue_case(scene, 2 * T + 3, "random", "some", seed=4)
    m = uploaded(ctx, scene_map(scene, points, new_queue=q), scene["kfs"])
    rf = host.ReFinder(ctx)
    stop = np.zeros(1, np.uint8)
    timer = threading.Timer(0.001, stop.__setitem__, (0, 1))
    down0 = m.traffic()[1]
    timer.start()
    r = m.refind_queue(rf, NEW_POINTS, stop=stop, max_pairs_per_pass=K)
    timer.join()
    good = np.flatnonzero(points["bad"][q] == 0)
    wp = r["n_pairs"] // K
    assert r["n_pairs"] == wp * K and wp <= len(good)
    consumed = (int(good[wp - 1]) + 1 if wp else 0) if r["stopped"] else len(q)
    assert r["points_consumed"] == consumed and r["n_bad_points"] == consumed - (wp if r["stopped"] else len(good))
    assert m.traffic()[1] - down0 == 4 + 16 + (4 if r["stopped"] and wp else 0)
    tab = m.tables()
    assert tab["new_queue"].tobytes() == q[consumed:].tobytes()
    check_invariants(tab)
    rf.close()
    m.close()
