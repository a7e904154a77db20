"""CPU: ptam_shuffle_order_host — the definition of a tracked frame's two random orders (the stand-in for std::random_shuffle of
src/Tracker.cc:483-484 and :597-600) — against a numpy restatement: key(i) = hi32(splitmix64(seed, (2 frame + w) << 32 | i)) << 32 | i,
the order = the low words of the keys sorted ascending.  Host code: no device is touched."""
import numpy as np
import pytest

from ptam_cg_amd import host
from ptam_cg_amd._lib import load

M64 = (1 << 64) - 1
# one wave, one sort tile, the steps of the device's register form (1024 keys a thread-row) and its LDS limit
SIZES = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
SEEDS = (0, 0x9E3779B97F4A7C15)
FRAMES = (0, 2 ** 31)


def splitmix64(seed, n):
    """the n-th output of the splitmix64 generator whose state starts at seed (tests/test_mapmaker_plan.py), n an array"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.asarray(n, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def order(seed, frame, which, n):
    i = np.arange(n, dtype=np.uint64)
    base = np.uint64(((2 * frame + which) << 32) & M64)
    keys = (splitmix64(seed, base | i) >> np.uint64(32)) << np.uint64(32) | i
    return (np.sort(keys) & np.uint64(0xFFFFFFFF)).astype(np.int32)


@pytest.fixture(scope="module")
def lib():
    return load()


@pytest.mark.parametrize("n", SIZES)
def test_against_numpy(lib, n):
    # (the restatement itself is the published generator: its first outputs from the states 0 and 1234567)
    assert [int(splitmix64(0, k)) for k in (0, 1)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4] and int(splitmix64(1234567, 0)) == 6457827717110365317
    for seed in SEEDS:
        for frame in FRAMES:
            got = [host.shuffle_order(lib, seed, frame, w, n) for w in (0, 1)]
            for w in (0, 1):
                assert got[w].dtype == np.int32 and got[w].shape == (n,)
                assert np.array_equal(got[w], order(seed, frame, w, n)), (seed, frame, w)
                assert np.array_equal(np.sort(got[w]), np.arange(n))                       # a permutation
            if n >= 63:   # (two orders of one or two points coincide half of the time)
                assert not np.array_equal(got[0], got[1])
                nxt = host.shuffle_order(lib, seed, frame + 1, 0, n)
                assert not np.array_equal(got[0], nxt) and not np.array_equal(got[1], nxt)
                assert not np.array_equal(got[0], host.shuffle_order(lib, seed + 1, frame, 0, n))


def test_the_frame_counter_wraps_at_two_to_the_31(lib):
    """(2 frame + w) << 32 is taken in 64 bits: frames 2^31 apart draw alike, and nothing else about a large frame is special"""
    a, b = host.shuffle_order(lib, 5, 7, 1, 300), host.shuffle_order(lib, 5, 7 + 2 ** 31, 1, 300)
    assert np.array_equal(a, b)
    assert np.array_equal(host.shuffle_order(lib, 5, 2 ** 63 + 3, 0, 300), order(5, 2 ** 63 + 3, 0, 300))


def test_refusals(lib):
    out = np.full(8, -5, np.int32)
    assert lib.shuffle_order_host(1, 0, 2, 8, host._ptr(out)) == -1 and lib.shuffle_order_host(1, 0, -1, 8, host._ptr(out)) == -1
    assert lib.shuffle_order_host(1, 0, 0, -1, host._ptr(out)) == -1 and lib.shuffle_order_host(1, 0, 0, 8, None) == -1
    assert (out == -5).all()
    assert lib.shuffle_order_host(1, 0, 0, 0, None) == 0
