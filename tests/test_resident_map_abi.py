"""CPU: host.ResidentMap names every table of the resident map (ptam_rmap) once, with the header's numbers and the record sizes (the
entries, numbers and structs themselves are checked with the whole header in tests/test_abi.py)."""
from ptam_cg_amd import _abi, host


def test_table_numbers_and_record_sizes_match_the_header():
    assert _abi.RMAP_TABLES == len(host.ResidentMap.TABLES) == 12
    assert sorted(i for i, _ in host.ResidentMap.TABLES.values()) == list(range(12))
    row_bytes = {k: dt.itemsize for k, (_, dt) in host.ResidentMap.TABLES.items()}
    assert row_bytes == dict(poses=96, fixed=1, points3=24, points=96, sources=80, bad=1, outlier_count=4, inlier_count=4, meas=32, never=8,
                             new_queue=4, failure=8)
