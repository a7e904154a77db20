// map_tables_check.h — what the map calls ask of tables that come from the host, each rule once.  Host only and no HIP: a plain C++
// compiler builds it (tools/mapmaker/map_host_check.cc runs the rules under the sanitizers).  A resident map's tables were checked
// by the rm_check_* kernels when they went up and every call keeps the rules, so only the host-table entries call these.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ptam_hip.h"

template <class Row>
inline bool mc_row_less(const Row& x, const Row& y) { return x.kf < y.kf || (x.kf == y.kf && x.point < y.point); }

// a table sorted strictly by (kf, point), every index in range (ptam_map_meas, ptam_map_pair)
template <class Row>
inline bool mc_sorted_in_range(int n, const Row* t, int n_kf, int n_points) {
    for (int i = 0; i < n; i++) {
        if (t[i].kf < 0 || t[i].kf >= n_kf || t[i].point < 0 || t[i].point >= n_points) return false;
        if (i > 0 && !mc_row_less(t[i - 1], t[i])) return false;
    }
    return true;
}
inline bool mc_meas_level_source(int n, const ptam_map_meas* m) {
    for (int i = 0; i < n; i++)
        if (m[i].level < 0 || m[i].level >= PTAM_LEVELS || m[i].source < PTAM_MAP_SRC_TRACKER || m[i].source > PTAM_MAP_SRC_EPIPOLAR) return false;
    return true;
}
inline bool mc_meas_valid(int n, const ptam_map_meas* m, int n_kf, int n_points) {
    return mc_sorted_in_range(n, m, n_kf, n_points) && mc_meas_level_source(n, m);
}
// mvFailureQueue: any order, duplicates allowed, indices in range
inline bool mc_pairs_in_range(int n, const ptam_map_pair* q, int n_kf, int n_points) {
    for (int i = 0; i < n; i++)
        if (q[i].kf < 0 || q[i].kf >= n_kf || q[i].point < 0 || q[i].point >= n_points) return false;
    return true;
}
// mqNewQueue, a NEW_POINTS work list: in range, no point twice
inline bool mc_queue_unique(int n, const int32_t* q, int n_points) {
    std::vector<uint8_t> seen((size_t)n_points, 0);
    for (int e = 0; e < n; e++) {
        if (q[e] < 0 || q[e] >= n_points || seen[(size_t)q[e]]) return false;
        seen[(size_t)q[e]] = 1;
    }
    return true;
}
// a new keyframe's measurement list: sorted by point, none repeated, in range
inline bool mc_kf_rows(int n_points, int n_rows, const ptam_map_kf_row* rows) {
    for (int i = 0; i < n_rows; i++) {
        if (rows[i].point < 0 || rows[i].point >= n_points || rows[i].level < 0 || rows[i].level >= PTAM_LEVELS) return false;
        if (i > 0 && !(rows[i - 1].point < rows[i].point)) return false;
    }
    return true;
}
// the re-find's point rows: the patch source of each
inline bool mc_points_source_range(int n_points, const ptam_map_refind_point* p, int n_kf) {
    for (int i = 0; i < n_points; i++)
        if (p[i].src_kf < 0 || p[i].src_kf >= n_kf || p[i].src_level < 0 || p[i].src_level >= PTAM_LEVELS) return false;
    return true;
}
// The outlier list of one bundle against the tables: -1 and the call's counts in *r, or the first offending entry.  Every action
// and row index in range; with the tables on the host (meas / never given; null with a resident map, whose kernels look) also: the
// entry names its row, no row is named twice, no NEVER_RETRY pair is in never already (src/MapMaker.cc:947-948).
inline int mc_outliers_tally(int n_outliers, const ptam_map_outlier* outliers, int n_meas, const ptam_map_meas* meas, int n_never,
                             const ptam_map_pair* never, int n_failure, ptam_map_outliers_result* r) {
    *r = ptam_map_outliers_result{};
    std::vector<uint8_t> named(meas ? (size_t)n_meas : 0, 0);
    for (int i = 0; i < n_outliers; i++) {
        const ptam_map_outlier& o = outliers[i];
        if (o.action < PTAM_MAP_OUT_POINT_BAD || o.action > PTAM_MAP_OUT_NEVER_RETRY || o.meas < 0 || o.meas >= n_meas) return i;
        if (meas) {
            if (meas[o.meas].kf != o.kf || meas[o.meas].point != o.point || named[(size_t)o.meas]) return i;
            named[(size_t)o.meas] = 1;
        }
        if (o.action == PTAM_MAP_OUT_NEVER_RETRY) {
            ptam_map_pair q;
            q.kf = o.kf;
            q.point = o.point;
            if (never && std::binary_search(never, never + n_never, q, mc_row_less<ptam_map_pair>)) return i;
            r->n_never_added++;
        } else if (o.action == PTAM_MAP_OUT_FAILURE_QUEUE)
            r->n_failure_added++;
        else
            r->n_point_bad++;
    }
    r->n_meas_out = n_meas - r->n_failure_added - r->n_never_added;
    r->n_never_out = n_never + r->n_never_added;
    r->n_failure_out = n_failure + r->n_failure_added;
    return -1;
}
