"""CPU: known answers, written by hand, for the restatement of the trail tracker and the stereo match table
(tests/trails_ref.py), and the ABI check that the library exports the new entry points."""
import ctypes
import math
import os

import numpy as np
import pytest

from ptam_cg_amd import _abi, host
from tests import trails_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ptam_cg_amd", "csrc", "libptam_hip.so")
NEW_ENTRIES = ("trails_create", "trails_destroy", "trails_start", "trails_advance", "trails_read", "trails_read_patches", "trails_matches",
               "init_points_from_trails")


def test_library_exports_the_trail_entry_points():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    for n in NEW_ENTRIES:
        assert n in _abi.PROTOTYPES and hasattr(lib, "ptam_" + n), n
    assert not set(NEW_ENTRIES) & set(_abi.bind(lib, "ptam_").missing)
    assert ctypes.sizeof(_abi.Trail) == 16 and ctypes.sizeof(_abi.HomographyMatch) == 64
    assert (_abi.INIT_MADE, _abi.INIT_SUBPIX_FAILED, _abi.INIT_BEHIND_CAMERA, _abi.INIT_TEMPLATE_BAD) == (0, 1, 2, 3)


def _noise(seed, shape=(48, 64)):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def _put(im, patch, x, y):
    im[y - 4:y + 5, x - 4:x + 5] = patch


def _corners(*xy):
    return np.array(sorted(xy, key=lambda c: (c[1], c[0])), dtype=np.int32).reshape(-1, 2)


def test_tie_goes_to_the_raster_first_corner():
    patch = _noise(1, (9, 9))
    im = _noise(2)
    _put(im, patch, 12, 20)
    _put(im, patch, 24, 20)
    found, pos = TR.find_patch((18, 20), im, _corners((24, 20), (12, 20)), patch)     # same row: the smaller x comes first
    assert found and pos == (12, 20)
    im = _noise(2)
    _put(im, patch, 24, 14)
    _put(im, patch, 12, 20)
    found, pos = TR.find_patch((18, 18), im, _corners((12, 20), (24, 14)), patch)     # the smaller y comes first
    assert found and pos == (24, 14)
    assert TR.ssd_at_point(im, 24, 14, patch) == 0 == TR.ssd_at_point(im, 12, 20, patch)


def test_box_is_closed_and_ten_wide():
    patch = _noise(1, (9, 9))
    for c, inside in (((30, 20), True), ((31, 20), False), ((20, 30), True), ((20, 31), False), ((10, 10), True), ((9, 20), False)):
        im = _noise(2)
        _put(im, patch, *c)                            # a perfect match at c: found iff c is inside the box
        assert TR.find_patch((20, 20), im, _corners(c), patch) == ((True, c) if inside else (False, (20, 20))), c


def test_corner_three_pixels_from_a_border_scores_max_plus_one():
    im = _noise(3)
    h, w = im.shape
    patch = TR.sample_patch(im, 20, 20)
    for x, y in ((3, 20), (20, 3), (w - 4, 20), (20, h - 4)):
        assert TR.ssd_at_point(im, x, y, patch) == 100001
    for x, y in ((4, 20), (20, 4), (w - 5, 20), (20, h - 5)):
        assert TR.ssd_at_point(im, x, y, patch) != 100001
    info = {}
    assert TR.find_patch((5, 20), im, _corners((3, 20)), patch, info=info) == (False, (5, 20))
    assert info == dict(scored=1, border=1, best_ssd=100001)


def test_best_ssd_of_exactly_the_limit_is_not_found():
    base = np.full((48, 64), 100, dtype=np.uint8)
    patch = np.full((9, 9), 100, dtype=np.uint8)
    patch.reshape(-1)[:10] = 200                       # ten differences of 100: 10 * 100^2 = 100000
    assert TR.ssd_at_point(base, 20, 20, patch) == 100000
    info = {}
    assert TR.find_patch((20, 20), base, _corners((20, 20)), patch, info=info) == (False, (20, 20))
    assert info["best_ssd"] == 100000
    patch = np.full((9, 9), 100, dtype=np.uint8)
    patch.reshape(-1)[:9] = 200                        # 9 * 100^2 + 99^2 + 14^2 + 1 + 1 = 99999
    patch.reshape(-1)[9:13] = (199, 114, 101, 99)
    assert TR.ssd_at_point(base, 20, 20, patch) == 99999
    assert TR.find_patch((22, 19), base, _corners((20, 20)), patch) == (True, (20, 20))


def _married_case(back):
    """one trail at S = (30, 30); the current frame shows its patch at E = (33, 30); the previous frame shows it at `back`"""
    patch = _noise(4, (9, 9))
    cur, prev = _noise(5), _noise(6)
    _put(cur, patch, 33, 30)
    _put(prev, patch, *back)
    t = TR.Trails()
    t.trails = [[(30, 30), (30, 30), patch]]
    t.prev = (prev, _corners(back))
    return t, t.advance(cur, _corners((33, 30)))


def test_married_check_keeps_two_and_erases_four():
    t, counts = _married_case((31, 31))                # (1, 1): mag_squared 2
    assert counts == (1, 1) and t.trails[0][0] == (30, 30) and t.trails[0][1] == (33, 30)
    assert t.stats["died_unmarried"] == 0
    t, counts = _married_case((32, 30))                # (2, 0): mag_squared 4
    assert counts == (1, 0) and t.trails == []
    assert t.stats["died_unmarried"] == 1 and t.stats["died_unfound"] == 0


def test_found_forwards_but_unmarried_counts_as_good():
    patch = _noise(4, (9, 9))
    cur, prev = _noise(5), _noise(6)
    _put(cur, patch, 33, 30)
    t = TR.Trails()
    t.trails = [[(30, 30), (30, 30), patch], [(10, 10), (10, 10), _noise(7, (9, 9))]]
    t.prev = (prev, _corners((45, 45)))                # nothing near: the backwards search finds nothing
    assert t.advance(cur, _corners((33, 30))) == (1, 0)      # the first trail was found forwards; the second not at all
    assert t.stats["died_unmarried"] == 1 and t.stats["died_unfound"] == 1
    assert np.array_equal(t.prev[0], cur)              # mPreviousFrameKF = mCurrentKF


def test_start_orders_by_score_then_y_then_x():
    mc = np.array([(20, 30), (40, 12), (12, 12), (30, 20), (5, 20), (25, 25)], dtype=np.int32)
    st = np.array([50.0, 80.0, 80.0, 80.0, 500.0, 20.0])
    # (5, 20) is inside the 10-pixel border: never a candidate; 20.0 is not above the threshold
    assert TR.start_order(mc, st, (48, 64), 20.0) == [2, 1, 3, 0]
    assert TR.start_order(mc, st, (48, 64), 80.0) == []
    im = _noise(8)
    t = TR.Trails()
    assert t.start(im, _corners(*map(tuple, mc)), mc, st, 20.0, max_initial=3) == 3
    assert [tr[0] for tr in t.trails] == [(12, 12), (40, 12), (30, 20)]
    assert np.array_equal(t.trails[0][2], im[8:17, 8:17]) and t.trails[0][1] == t.trails[0][0]
    assert t.start(im, _corners(*map(tuple, mc)), mc, st, 20.0, max_initial=1000, max_trails=2) == 2


def test_jac_is_the_derivative_at_the_second_point():
    cam = TR.Camera(size=(160, 128))
    tab = np.array([(30, 40, 120, 90)], dtype=host.TRAIL_DT)
    m = TR.match_table(cam, tab)[0]
    second_only = TR.Camera(size=(160, 128))
    assert tuple(m["second"]) == second_only.unproject(120.0, 90.0)
    assert tuple(m["jac"]) == second_only.projection_derivs()
    first_only = TR.Camera(size=(160, 128))
    assert tuple(m["first"]) == first_only.unproject(30.0, 40.0)
    assert not np.allclose(m["jac"], first_only.projection_derivs(), rtol=1e-3)

    def project(x, y):                                 # ATANCamera::Project (src/ATANCamera.cc:109-121)
        r = math.hypot(x, y)
        f = cam.w_inv * math.atan(r * cam.two_tan) / r
        return cam.centre[0] + cam.focal[0] * f * x, cam.centre[1] + cam.focal[1] * f * y
    x, y = m["second"]
    assert np.allclose(project(x, y), (120.0, 90.0), atol=1e-9)
    e = 1e-6
    num = [(project(x + e, y)[0] - project(x - e, y)[0]) / (2 * e), (project(x, y + e)[0] - project(x, y - e)[0]) / (2 * e),
           (project(x + e, y)[1] - project(x - e, y)[1]) / (2 * e), (project(x, y + e)[1] - project(x, y - e)[1]) / (2 * e)]
    assert np.allclose(m["jac"], num, rtol=1e-6, atol=1e-6)
