"""-m gpu: ptam_rmap_bundle_adjust_routed — the bundle with its outliers applied in place, the routed list never leaving the device —
against the two calls it stands for, ptam_rmap_bundle_adjust and ptam_rmap_apply_outliers, on a second handle that holds the same
map.  Tables are compared by tobytes(), counts by ==, the bytes over the host link with the formula of the header."""
import numpy as np
import pytest

from ptam_cg_amd import _abi, host, synth
from tests import map_ba_ref as R
from tests import map_edit_ref as E
from tests.test_gpu_resident_map import BA_COUNTS, check_invariants, same_tables, uploaded, with_ba_tables

pytestmark = pytest.mark.gpu
E_ARG = -1      # PTAM_E_ARG
MODES = [_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL]
ACTIONS = {_abi.OUT_POINT_BAD, _abi.OUT_FAILURE_QUEUE, _abi.OUT_NEVER_RETRY}
K, P = 9, 400   # nine keyframes: RECENT runs (five adjusted, four fixed)


@pytest.fixture(scope="module")
def ctx(hip):
    c = host.Context(lib=hip)
    yield c
    c.close()


def make_map(outliers, seed=3, n_kf=K):
    """A whole map around tests/map_ba_ref.map_from_problem, with never pairs that are in no measurement and a failure queue, so
    that the merge and the append start behind rows that are there already.  outliers: "none" and "one" have exact fixed poses and
    no displaced measurement but, for "one", a single row of the newest keyframe moved by 25 pixels; "many" displaces a seeded
    tenth of the rows as tests/test_gpu_map_ba.py does."""
    many = outliers == "many"
    prob = synth.make_ba_problem(n_kf, P, seed, window=6, outlier_frac=0.1 if many else 0.0, **({} if many else {"pose_noise": 0.0}))
    poses, fixed, points, meas = R.map_from_problem(prob, seed=seed)
    if outliers == "one":
        meas["root_pos"][np.flatnonzero(meas["kf"] == n_kf - 1)[7]] += (25.0, -25.0)
    h = with_ba_tables(poses, fixed, points, meas, seed=seed)
    rng = np.random.default_rng(seed + 100)
    free = np.ones((n_kf, P), bool)
    free[meas["kf"], meas["point"]] = False
    kf, pt = np.nonzero(free)
    pick = np.sort(rng.choice(len(kf), 40, replace=False))
    h["never"] = np.zeros(40, E.PAIR_DT)
    h["never"]["kf"], h["never"]["point"] = kf[pick], pt[pick]
    h["failure"] = np.zeros(7, E.PAIR_DT)
    h["failure"]["kf"], h["failure"]["point"] = rng.integers(0, n_kf, 7), rng.integers(0, P, 7)
    return h


def two_calls(m, mode, **kw):
    """the reference path: the bundle, its list down, the list up again"""
    got = m.bundle_adjust(mode, **kw)
    return got, m.apply_outliers(got["outliers"])


def routed_bytes(n_kf, ba):
    """include/ptam_hip.h: what ptam_rmap_bundle_adjust_routed moves, up and down"""
    if not ba["ran"]:
        return 0, 0
    return (97 * (ba["n_adjust"] + ba["n_fixed"]),
            32 + 4 * n_kf + (96 * n_kf if ba["accepted"] > 0 else 0) + (_abi.RMAP_WORD_BYTES if ba["n_outliers"] > 0 else 0))


def assert_routed_equals_two_calls(a, b, mode, **kw):
    """a: the two calls, b: the routed call, on equal maps -> the reference path's bundle result"""
    ref, ref_o = two_calls(a, mode, **kw)
    up0, down0 = b.traffic()
    got, got_o = b.bundle_adjust_routed(mode, **kw)
    up, down = b.traffic()
    assert got == {k: ref[k] for k in BA_COUNTS}
    assert got_o == ref_o
    ta, tb = a.tables(), b.tables()
    same_tables(tb, ta)
    check_invariants(tb)
    assert a.counts() == b.counts()
    assert (up - up0, down - down0) == routed_bytes(len(ta["poses"]), got)
    return ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("outliers", ["none", "one", "many"])
def test_routed_equals_the_two_calls(ctx, mode, outliers):
    h = make_map(outliers)
    a, b = uploaded(ctx, h), uploaded(ctx, h)
    ref = assert_routed_equals_two_calls(a, b, mode, deterministic=1)
    # the reference path itself has what the case is about
    assert ref["ran"] == 1 and ref["accepted"] > 0
    if outliers == "none":
        assert ref["n_outliers"] == 0
    elif outliers == "one":
        assert ref["n_outliers"] == 1
    else:
        assert ref["n_outliers"] > 64 and set(ref["outliers"]["action"]) == ACTIONS   # (64: never and failure grow)
        _, per_point = np.unique(ref["outliers"]["point"], return_counts=True)
        assert per_point.max() >= 2
    a.close()
    b.close()


def test_recent_then_all_on_the_tables_and_the_mirror_the_routed_call_left(ctx):
    """the second bundle marshals its cameras from the mirror and selects from the tables the first one's outlier stage wrote"""
    h = make_map("many", seed=5)
    a, b = uploaded(ctx, h), uploaded(ctx, h)
    n = 0
    for mode in (_abi.MAP_BA_RECENT, _abi.MAP_BA_ALL, _abi.MAP_BA_RECENT):
        n += assert_routed_equals_two_calls(a, b, mode, deterministic=1)["n_outliers"]
    assert n > 0
    a.close()
    b.close()


def test_recent_below_eight_keyframes_does_not_run(ctx):
    h = make_map("many", n_kf=7)
    a, b = uploaded(ctx, h), uploaded(ctx, h)
    before = b.tables()
    ref = assert_routed_equals_two_calls(a, b, _abi.MAP_BA_RECENT, deterministic=1)   # :790-793
    assert all(ref[k] == 0 for k in BA_COUNTS)
    same_tables(b.tables(), before)
    ba, out = b.bundle_adjust_routed(_abi.MAP_BA_RECENT)
    assert out == dict(n_point_bad=0, n_failure_added=0, n_never_added=0, n_meas_out=len(h["meas"]), n_never_out=40, n_failure_out=7)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES)
def test_abort_before_the_call(ctx, mode):
    h = make_map("many")
    a, b = uploaded(ctx, h), uploaded(ctx, h)
    before = b.tables()
    ref = assert_routed_equals_two_calls(a, b, mode, abort=np.ones(1, np.uint8), deterministic=1)
    assert ref["ran"] == 1 and ref["accepted"] == 0
    same_tables(b.tables(), before, keys=("poses", "points3", "points"))
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_refusal_leaves_what_the_two_calls_leave(ctx, mode):
    """A pair the bundle routes as NEVER_RETRY is in never already (src/MapMaker.cc:947-948 keeps the two sets apart): the outlier
    stage refuses, after the accepted bundle's scatter."""
    h = make_map("many")
    probe = uploaded(ctx, h)
    lst = probe.bundle_adjust(mode, deterministic=1)["outliers"]
    probe.close()
    rows = np.flatnonzero(lst["action"] == _abi.OUT_NEVER_RETRY)
    assert len(rows) >= 2
    clash = np.zeros(1, E.PAIR_DT)
    clash["kf"], clash["point"] = lst["kf"][rows[1]], lst["point"][rows[1]]
    h = dict(h, never=E.sort_pairs(np.concatenate([h["never"], clash])))
    a, b = uploaded(ctx, h), uploaded(ctx, h)
    before = b.tables()
    ref = a.bundle_adjust(mode, deterministic=1)
    assert ref["outliers"].tobytes() == lst.tobytes() and ref["accepted"] > 0
    assert a.apply_outliers(ref["outliers"], check=False) == E_ARG and a.last_refusal() == (_abi.RMAP_OUTLIERS, rows[1])
    assert b.bundle_adjust_routed(mode, check=False, deterministic=1) == E_ARG and b.last_refusal() == (_abi.RMAP_OUTLIERS, rows[1])
    ta, tb = a.tables(), b.tables()
    same_tables(tb, ta)            # (check_invariants does not hold: the map was made with a pair in both sets)
    same_tables(tb, before, keys=("bad", "meas", "never", "failure"))
    assert tb["poses"].tobytes() != before["poses"].tobytes()
    # both handles go on alike: the mirror followed the scatter on both
    ra, rb = a.bundle_adjust(_abi.MAP_BA_ALL, deterministic=1), b.bundle_adjust(_abi.MAP_BA_ALL, deterministic=1)
    assert all(ra[k] == rb[k] for k in BA_COUNTS) and ra["outliers"].tobytes() == rb["outliers"].tobytes()
    same_tables(b.tables(), a.tables())
    a.close()
    b.close()
