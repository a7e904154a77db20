"""CPU: the host side of ptam_rmap_init_from_stereo, ptam_rmap_align_to_plane and ptam_rmap_clear (their structs, status numbers and
argument counts are checked with the whole header in tests/test_abi.py): the wrappers exist, and the defaults
ptam_rmap_init_opts_default writes are the reference's (src/MapMaker.cc:34, :283, :333, :374, :382-385)."""
import ctypes

from ptam_cg_amd import _abi, host
from tests.abi_header import lib as bound_lib


def test_the_wrappers_exist():
    for method in ("init_opts", "InitFromStereo", "align_to_plane", "clear"):
        assert callable(getattr(host.ResidentMap, method))


def test_defaults_are_the_reference_s():
    lib = bound_lib()
    o = _abi.RmapInitOpts()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    assert lib.rmap_init_opts_default(ctypes.byref(o)) == 0 and lib.rmap_init_opts_default(None) == -1
    assert (o.homography.max_pixel_error, o.homography.trials, o.homography.seed, bool(o.homography.samples)) == (5.0, 300, 0, False)
    assert (o.wiggle_scale, o.subpix_max_its, o.first_bundles, o.max_bundles) == (0.1, 10, 5, 0)
    assert o.epipolar.n_levels == 4 and list(o.epipolar.levels) == [0, 3, 1, 2]
    ba, epi, plane = _abi.BaOpts(), _abi.EpipolarOpts(), _abi.PlaneOpts()
    lib.ba_opts_default(ctypes.byref(ba))
    lib.epipolar_opts_default(ctypes.byref(epi))
    lib.plane_opts_default(ctypes.byref(plane))
    assert bytes(o.ba) == bytes(ba)
    assert (o.epipolar.wiggle_scale, o.epipolar.min_shi_tomasi, o.epipolar.subpix_max_its) == (epi.wiggle_scale, epi.min_shi_tomasi, epi.subpix_max_its)
    assert (o.plane.max_dist, o.plane.trials, o.plane.seed, bool(o.plane.samples)) == (plane.max_dist, plane.trials, plane.seed, False) == (0.05, 100, 0, False)
