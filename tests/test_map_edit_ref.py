"""CPU: the two restatements of tests/map_edit_ref.py — the literal one with Python objects and the vectorised one — agree on
seeded maps for each of the three table edits, the tables stay valid input through the sequence outliers -> bad points -> new
points, and the inputs the GPU tests use exercise every class of each entry."""
import numpy as np
import pytest

from ptam_cg_amd import _abi
from tests import map_edit_ref as E

SEEDS = range(20)
K, N, M = 6, 40, 90


def small(seed):
    t = E.make_tables(seed, K, N, M, bad_share=0.1, count_share=0.1)
    t["outliers"] = E.make_outliers(seed + 1000, K, N, t["meas"], 30)
    return t


@pytest.mark.parametrize("seed", SEEDS)
def test_apply_outliers_literal_equals_vectorised(seed):
    t = small(seed)
    m = E.map_from_tables(K, N, t["meas"], t["never"], t["bad"], new_queue=t["new_queue"], failure=t["failure"])
    actions = E.literal_apply_outliers(m, list(zip(t["outliers"]["point"].tolist(), t["outliers"]["kf"].tolist())))
    assert actions == t["outliers"]["action"].tolist()      # the literal loop routes as tests/map_ba_ref.route does
    lit = E.tables_from_map(m)
    vec = E.np_apply_outliers(K, t["bad"], t["meas"], t["never"], t["failure"], t["outliers"])
    E.assert_same(lit, vec, (), ("bad", "meas", "never", "failure"))
    assert vec["n_point_bad"] + vec["n_failure_added"] + vec["n_never_added"] == len(t["outliers"])
    assert E.tables_valid(K, N, vec["meas"], vec["never"])


@pytest.mark.parametrize("seed", SEEDS)
def test_handle_bad_points_literal_equals_vectorised(seed):
    t = small(seed)
    m = E.map_from_tables(K, N, t["meas"], t["never"], t["bad"], t["outlier_count"], t["inlier_count"], t["new_queue"], t["failure"])
    n_marked = E.literal_handle_bad_points(m)
    lit = E.tables_from_map(m)
    cols = E.point_columns(seed, N)
    vec = E.np_handle_bad_points(K, N, t["meas"], t["never"], t["bad"], t["outlier_count"], t["inlier_count"], t["new_queue"], t["failure"], cols)
    E.assert_same(lit, vec, ("n_new_dropped",), ("meas", "never", "new_queue", "failure", "new_index", "kept"))
    assert n_marked == vec["n_marked"] and len(m.vpPointsTrash) == vec["n_removed"] and len(m.vpPoints) == vec["n_kept"]
    assert lit["n_failure_dropped"] == len(t["failure"]) - vec["n_failure_out"]
    for c, c0 in zip(vec["columns"], cols):
        assert c[:vec["n_kept"]].tobytes() == c0[vec["kept"]].tobytes() and c[vec["n_kept"]:].tobytes() == c0[vec["n_kept"]:].tobytes()
    assert E.tables_valid(K, vec["n_kept"], vec["meas"], vec["never"])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("target_source", [_abi.SRC_EPIPOLAR, _abi.SRC_TRAIL])
def test_add_points_literal_equals_vectorised(seed, target_source):
    t = small(seed)
    src_kf, target_kf = (K - 1, 2) if seed % 2 else (1, K - 2)
    made = E.make_made(seed, 7)
    m = E.map_from_tables(K, N, t["meas"], t["never"])
    E.literal_add_points(m, src_kf, target_kf, made, target_source)
    lit = E.tables_from_map(m)
    lit["points"], lit["sources"] = E.point_rows_of_made(m)
    vec = E.np_add_points(K, N, t["meas"], src_kf, target_kf, made, target_source)
    E.assert_same(lit, vec, (), ("meas", "new_queue", "points", "sources"))
    assert E.tables_valid(K, N + 7, vec["meas"], t["never"])


def test_the_sequence_keeps_the_tables_valid():
    t = small(7)
    a = E.np_apply_outliers(K, t["bad"], t["meas"], t["never"], t["failure"], t["outliers"])
    assert E.tables_valid(K, N, a["meas"], a["never"])
    b = E.np_handle_bad_points(K, N, a["meas"], a["never"], a["bad"], t["outlier_count"], t["inlier_count"], t["new_queue"], a["failure"])
    assert E.tables_valid(K, b["n_kept"], b["meas"], b["never"])
    assert (b["new_queue"] < b["n_kept"]).all() and (b["failure"]["point"] < b["n_kept"]).all()
    c = E.np_add_points(K, b["n_kept"], b["meas"], K - 1, K - 3, E.make_made(5, 9))
    assert E.tables_valid(K, b["n_kept"] + 9, c["meas"], b["never"]) and len(c["meas"]) == len(b["meas"]) + 18


def test_the_gpu_inputs_exercise_every_class():
    E.assert_every_class(E.gpu_case())
    E.assert_every_class(small(7))
