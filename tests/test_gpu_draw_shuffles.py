"""-m gpu: ptam_tracker_draw_shuffles — a tracked frame's two random orders drawn on the device — against its definition
ptam_shuffle_order_host, entry by entry, at every size where the kernel changes path; and a frame tracked behind the draw against
the frame of a twin that got the same two orders through ptam_tracker_set_shuffle, byte for byte."""
import numpy as np
import pytest

from ptam_cg_amd import host, synth
from tests.test_gpu_track_frames_batch import Camera

pytestmark = pytest.mark.gpu

# one wave, the sort tile, the register form's steps (1024 keys a thread-row: 1, 2, 4, 8 rows), the LDS limit and, beyond it, the sort
# in global memory up to its next merge pass (16384)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385)
SEED = 0x9E3779B97F4A7C15


def _orders(lib, seed, frame, n):
    return [host.shuffle_order(lib, seed, frame, w, n) for w in (0, 1)]


@pytest.fixture(scope="module")
def scene(hip):
    ctx = host.Context(lib=hip, size=(163, 121))
    a, _ = synth.make_frame_pair()
    kf = host.KeyFrame(ctx).MakeKeyFrame_Lite(np.ascontiguousarray(a[:121, :163]))
    yield ctx, kf
    kf.close()
    ctx.close()


def _set_points(tr, kf, n):
    rng = np.random.default_rng(n)
    world = rng.uniform(-1, 1, (n, 3))
    tr.set_map(world, rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)), kf, np.zeros(n, np.int32), np.full((n, 2), 40, np.int32))


@pytest.mark.parametrize("n", SIZES)
def test_the_device_draws_the_defined_orders(hip, scene, n):
    ctx, kf = scene
    tr = host.Tracker(ctx, max(n, 32))
    _set_points(tr, kf, n)
    for seed, frame in ((0, 0), (SEED, 2 ** 31), (SEED, 12345)):
        tr.draw_shuffles(seed, frame)
        got, want = tr.read_shuffle(), _orders(hip, seed, frame, n)
        for w in (0, 1):
            assert np.array_equal(got[w], want[w]), (seed, frame, w)
    tr.close()


def test_draw_and_set_replace_each_other_and_a_new_size_resets(hip, scene):
    ctx, kf = scene
    for n in (700, 9000):   # host-mapped and device-resident set_shuffle
        tr = host.Tracker(ctx, n + 100)
        _set_points(tr, kf, n)
        ident = np.arange(n, dtype=np.int32)
        assert all(np.array_equal(o, ident) for o in tr.read_shuffle())
        rng = np.random.default_rng(3)
        pa, pb = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
        want = _orders(hip, 9, 4, n)
        tr.draw_shuffles(9, 4)
        assert all(np.array_equal(g, w) for g, w in zip(tr.read_shuffle(), want))
        tr.set_shuffle(pa, pb)                                   # set behind a draw
        got = tr.read_shuffle()
        assert np.array_equal(got[0], pa) and np.array_equal(got[1], pb)
        tr.draw_shuffles(9, 4)                                   # a draw behind a set
        assert all(np.array_equal(g, w) for g, w in zip(tr.read_shuffle(), want))
        _set_points(tr, kf, n + 50)                              # a map of another size: the identity, as before
        assert all(np.array_equal(o, np.arange(n + 50)) for o in tr.read_shuffle())
        tr.draw_shuffles(9, 5)
        assert all(np.array_equal(g, w) for g, w in zip(tr.read_shuffle(), _orders(hip, 9, 5, n + 50)))
        tr.close()
    empty = host.Tracker(ctx, 32)                                # no map: nothing happens
    empty.draw_shuffles(1, 1)
    assert hip.tracker_draw_shuffles(None, 1, 1) == -1
    empty.close()


@pytest.fixture(scope="module")
def cam(hip):
    c = Camera(hip, estimator=False)
    yield c
    c.close()


@pytest.mark.parametrize("chop", [False, True], ids=["default_options", "fine_chop_cuts"])
def test_a_frame_behind_the_draw_equals_the_twin_with_set_shuffle(hip, cam, chop):
    """the 1 244-point scene.  chop: CoarseMax 30 and a patch budget of 400, so that the fine set is chopped (:597-600) and the second
    order is read at all — asserted, and asserted to matter: a third tracker with another second order tracks another set"""
    n = len(cam.map["world"])
    assert n == 1244
    opts = cam.tr.opts(coarse_max=30, max_patches=400) if chop else cam.tr.opts()
    frame, k = 7, 1
    lv, fi = _orders(hip, SEED, frame, n)
    trs = [cam._tracker() for _ in range(3)]
    trs[0].draw_shuffles(SEED, frame)
    trs[1].set_shuffle(lv, fi)
    trs[2].set_shuffle(lv, host.shuffle_order(hip, SEED, frame + 1, 1, n))
    res, sets = [], []
    for tr in trs:
        res.append(tr.TrackFrame(cam.kf, cam.d_frames[k], cam.poses[k], opts).copy())
        sets.append(tr.iteration_set().copy())
    for f in res[0].dtype.names:
        assert res[0][f].tobytes() == res[1][f].tobytes(), f
    assert sets[0].tobytes() == sets[1].tobytes() and len(sets[0]) > 100
    assert res[0]["n_meas"] > 100
    budget = int(opts["max_patches"][0])
    cut = res[0]["n_coarse"] + res[0]["n_top"] + res[0]["n_fine"] == budget and sum(res[0]["n_pvs"]) - int(opts["coarse_max"][0]) > budget
    if chop:
        assert cut
        assert sets[2]["point"].tobytes() != sets[0]["point"].tobytes()
    for tr in trs:
        tr.close()
