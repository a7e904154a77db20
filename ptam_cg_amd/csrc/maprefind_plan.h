// maprefind_plan.h — what the host decides of a map re-find before anything is enqueued (MapMaker::ReFind*, src/MapMaker.cc:1028-1081):
// the work list checked, the bBad filter of ReFindNewlyMade, the orders the kernels are told, the pair counts, and what a call that
// stopped early says of the queue.  Host only and no HIP (tools/mapmaker/map_host_check.cc runs it on the CPU).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "map_tables_check.h"

enum { MR_DEFAULT_PASS = 4096 };

struct MrPlan {
    int mode = 0, n_kf = 0, n_work = 0;
    int kf0 = 0;                          // KEYFRAME: the keyframe
    std::vector<int> wpts, wentry, wrank; // NEW_POINTS: the points that make pairs (queue order), their queue entries, their index-order places
    std::vector<ptam_map_pair> wq;        // FAILURE_QUEUE: sorted (:1074), duplicates kept (the kernel skips them)
    long long bound = 0;                  // the pair count the capacities are held against (bBad is the table's, not the count's, business)
    int pairs = 0;                        // the pairs the call visits
    int per_pass = 0;                     // NEW_POINTS: whole points, at least one
};

// the pairs in flight per pass: the caller's bound (0: the default), in NEW_POINTS whole points and at least one, never more than
// the call visits
inline int mr_per_pass(int mode, int n_kf, int max_pairs_per_pass, int pairs) {
    int per_pass = max_pairs_per_pass > 0 ? max_pairs_per_pass : (int)MR_DEFAULT_PASS;
    if (mode == PTAM_MAP_REFIND_NEW_POINTS && n_kf > 0) per_pass = n_kf * (per_pass / n_kf > 0 ? per_pass / n_kf : 1);
    return per_pass > pairs ? pairs : per_pass;
}

// bad_of(entry, point): bBad of a NEW_POINTS entry's point (:1056-1059).  false: the work list is refused.
template <class BadOf>
inline bool mr_plan(int mode, int n_kf, int n_points, int n_work, const void* work, BadOf bad_of, int max_pairs_per_pass, MrPlan* out) {
    MrPlan p;
    p.mode = mode;
    p.n_kf = n_kf;
    p.n_work = n_work;
    long long total = 0;
    if (mode == PTAM_MAP_REFIND_KEYFRAME) {
        if (n_work > 1) return false;
        if (n_work == 1) {
            p.kf0 = *(const int32_t*)work;
            if (p.kf0 < 0 || p.kf0 >= n_kf) return false;
            p.bound = total = n_points;
        }
    } else if (mode == PTAM_MAP_REFIND_NEW_POINTS) {
        const int32_t* w = (const int32_t*)work;
        if (!mc_queue_unique(n_work, w, n_points)) return false;
        for (int e = 0; e < n_work; e++) {
            if (bad_of(e, (int)w[e])) continue;
            p.wpts.push_back(w[e]);
            p.wentry.push_back(e);
        }
        p.bound = (long long)n_kf * n_work;
        total = (long long)n_kf * (long long)p.wpts.size();
        std::vector<int> by_index(p.wpts.size());
        for (size_t i = 0; i < by_index.size(); i++) by_index[i] = (int)i;
        std::sort(by_index.begin(), by_index.end(), [&](int x, int y) { return p.wpts[(size_t)x] < p.wpts[(size_t)y]; });
        p.wrank.resize(p.wpts.size());
        for (size_t r = 0; r < by_index.size(); r++) p.wrank[(size_t)by_index[r]] = (int)r;
    } else if (mode == PTAM_MAP_REFIND_FAILURE_QUEUE) {
        const ptam_map_pair* w = (const ptam_map_pair*)work;
        if (!mc_pairs_in_range(n_work, w, n_kf, n_points)) return false;
        p.wq.assign(w, w + n_work);
        std::sort(p.wq.begin(), p.wq.end(), mc_row_less<ptam_map_pair>);
        p.bound = total = n_work;
    } else
        return false;
    if (p.bound >= (1ll << 31)) return false;
    p.pairs = (int)total;
    p.per_pass = mr_per_pass(mode, n_kf, max_pairs_per_pass, p.pairs);
    *out = std::move(p);
    return true;
}

// NEW_POINTS, after `visited` pairs: queue entries behind the last visited point are popped while the flag is down (:1053-1059)
inline void mr_plan_consumed(const MrPlan& p, int visited, bool stopped, int* points_consumed, int* n_bad_points) {
    *points_consumed = *n_bad_points = 0;
    if (p.mode != PTAM_MAP_REFIND_NEW_POINTS) return;
    if (!stopped) {
        *points_consumed = p.n_work;
        *n_bad_points = p.n_work - (int)p.wpts.size();
        return;
    }
    const size_t wp = p.n_kf > 0 ? (size_t)(visited / p.n_kf) : 0;
    *points_consumed = wp > 0 ? p.wentry[wp - 1] + 1 : 0;
    *n_bad_points = *points_consumed - (int)wp;
}

// the result of a call that has no pair to visit; stop_now: the stop flag as it stands
inline ptam_map_refind_result mr_plan_nothing(const MrPlan& p, bool stop_now) {
    ptam_map_refind_result r = {};
    if (p.mode != PTAM_MAP_REFIND_NEW_POINTS) return r;
    r.stopped = stop_now && p.n_work > 0;
    mr_plan_consumed(p, 0, stop_now, &r.points_consumed, &r.n_bad_points);
    return r;
}
