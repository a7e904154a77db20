"""CPU: the host side of the keyframes' publication to the relocaliser (ptam_snapshot_keyframes_enable / _info,
ptam_sbi_bank_take_keyframes / _clear / _read; their structs and argument counts are checked with the whole header in
tests/test_abi.py): what a take reports, the built library exports each entry and the wrappers exist."""
from ptam_cg_amd import _abi, host

ENTRIES = ("snapshot_keyframes_enable", "snapshot_keyframes_info", "sbi_bank_take_keyframes", "sbi_bank_clear", "sbi_bank_read")


def test_a_take_reports_what_the_relocaliser_needs():
    for f in ("changed", "n_kf", "n_new", "generation", "map_id", "link_bytes"):
        assert f in dict(_abi.KeyframesTakeResult._fields_)
    # the names the older lists pin stay as they were: no new entry begins with ptam_map_snapshot_ or ptam_frame_report_
    assert not [n for n in ENTRIES if n.startswith(("map_snapshot_", "frame_report_"))]


def test_the_library_exports_the_entries_and_the_wrappers_exist():
    from ptam_cg_amd._lib import load
    lib = load()
    for name in ENTRIES:
        assert lib.has(name), name
    for cls, names in ((host.MapSnapshot, ("enable_keyframes", "keyframes")), (host.Relocaliser, ("take_keyframes", "clear", "read"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
