"""CPU: the host side of the map's publication to the tracker (ptam_map_snapshot_*, ptam_rmap_publish / point_serials /
resolve_serials, ptam_tracker_take_map / point_serials / read_iteration_serials; their structs and argument counts are checked with
the whole header in tests/test_abi.py): what a take reports, the built library exports each entry and the wrappers exist."""
from ptam_cg_amd import _abi, host

ENTRIES = ("map_snapshot_create", "map_snapshot_destroy", "map_snapshot_reserve", "map_snapshot_info", "rmap_publish", "rmap_point_serials",
           "rmap_resolve_serials", "tracker_take_map", "tracker_point_serials", "tracker_read_iteration_serials")


def test_a_take_reports_what_the_tracker_needs():
    for f in ("changed", "generation", "n_points", "n_carried", "n_new", "n_dropped"):
        assert f in dict(_abi.MapTakeResult._fields_)


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.ResidentMap, ("publish", "point_serials", "resolve_serials")), (host.Tracker, ("take_map", "point_serials", "iteration_serials")),
                       (host.MapSnapshot, ("reserve", "info", "close"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    # the table numbers of ptam_rmap_download stay: the serial column is not one of them
    assert _abi.RMAP_TABLES == 12 and len(host.ResidentMap.TABLES) == 12
