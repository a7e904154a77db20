// map_host_check.cc — the host-only pieces of the map maker's calls on the CPU, for a run under the sanitizers: the table rules of
// ptam_cg_amd/csrc/map_tables_check.h and the re-find planning of maprefind_plan.h (the bBad filter, the index-order rank, the sorted
// failure queue, the pair counts, and what a stopped call says of the queue).  No HIP.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ptam_cg_amd/csrc tools/mapmaker/map_host_check.cc -o map_host_check
//     ./map_host_check cases.txt
//
// The cases file is words separated by white space; a case is a keyword and its numbers, a line of output answers each:
//   sorted K N n (kf point)*n                  -> "sorted 0|1"     mc_sorted_in_range on pairs
//   meas K N n (kf point level source)*n       -> "meas 0|1"       mc_meas_valid
//   pairs K N n (kf point)*n                   -> "pairs 0|1"      mc_pairs_in_range
//   queue N n (point)*n                        -> "queue 0|1"      mc_queue_unique
//   kf_rows N n (point level)*n                -> "kf_rows 0|1"    mc_kf_rows
//   sources K n (src_kf src_level)*n           -> "sources 0|1"    mc_points_source_range
//   outliers host M (kf point)*M V (kf point)*V F O (kf point meas action)*O
//                                              -> "outliers <offender or -1> n_point_bad n_failure_added n_never_added n_meas_out
//                                                  n_never_out n_failure_out"; host = 1: the tables are looked at too
//   plan mode K N per_pass W work*W [bad*W]    -> "plan 0" or "plan 1 pairs bound per_pass consumed bad | wpts | wentry | wrank | wq";
//                                                 work is W points, or W (kf point) for the failure queue; bad only with NEW_POINTS
//   stop visited                               -> "stop points_consumed n_bad_points" of the last plan, stopped after `visited` pairs
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "maprefind_plan.h"

template <class Row>
static std::vector<Row> read_pairs(std::istream& in, int n) {
    std::vector<Row> t((size_t)n);
    for (auto& r : t) {
        r = Row{};
        in >> r.kf >> r.point;
    }
    return t;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: map_host_check cases.txt\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string what;
    MrPlan plan;
    while (in >> what) {
        if (what == "sorted" || what == "pairs") {
            int K, N, n;
            in >> K >> N >> n;
            const auto t = read_pairs<ptam_map_pair>(in, n);
            std::printf("%s %d\n", what.c_str(), (int)(what == "sorted" ? mc_sorted_in_range(n, t.data(), K, N) : mc_pairs_in_range(n, t.data(), K, N)));
        } else if (what == "meas") {
            int K, N, n;
            in >> K >> N >> n;
            std::vector<ptam_map_meas> t((size_t)n);
            for (auto& r : t) {
                r = ptam_map_meas{};
                in >> r.kf >> r.point >> r.level >> r.source;
            }
            std::printf("meas %d\n", (int)mc_meas_valid(n, t.data(), K, N));
        } else if (what == "queue") {
            int N, n;
            in >> N >> n;
            std::vector<int32_t> q((size_t)n);
            for (auto& p : q) in >> p;
            std::printf("queue %d\n", (int)mc_queue_unique(n, q.data(), N));
        } else if (what == "kf_rows") {
            int N, n;
            in >> N >> n;
            std::vector<ptam_map_kf_row> t((size_t)n);
            for (auto& r : t) {
                r = ptam_map_kf_row{};
                in >> r.point >> r.level;
            }
            std::printf("kf_rows %d\n", (int)mc_kf_rows(N, n, t.data()));
        } else if (what == "sources") {
            int K, n;
            in >> K >> n;
            std::vector<ptam_map_refind_point> t((size_t)n);
            for (auto& r : t) {
                r = ptam_map_refind_point{};
                in >> r.src_kf >> r.src_level;
            }
            std::printf("sources %d\n", (int)mc_points_source_range(n, t.data(), K));
        } else if (what == "outliers") {
            int host, M, V, F, O;
            in >> host >> M;
            auto pm = read_pairs<ptam_map_meas>(in, M);
            in >> V;
            const auto never = read_pairs<ptam_map_pair>(in, V);
            in >> F >> O;
            std::vector<ptam_map_outlier> o((size_t)O);
            for (auto& r : o) {
                r = ptam_map_outlier{};
                in >> r.kf >> r.point >> r.meas >> r.action;
            }
            ptam_map_outliers_result r;
            const int bad = mc_outliers_tally(O, o.data(), M, host ? pm.data() : nullptr, V, host ? never.data() : nullptr, F, &r);
            std::printf("outliers %d %d %d %d %d %d %d\n", bad, r.n_point_bad, r.n_failure_added, r.n_never_added, r.n_meas_out, r.n_never_out,
                        r.n_failure_out);
        } else if (what == "plan") {
            int mode, K, N, per_pass, W;
            in >> mode >> K >> N >> per_pass >> W;
            std::vector<int32_t> w((size_t)W);
            std::vector<ptam_map_pair> wq;
            std::vector<int> bad;
            if (mode == PTAM_MAP_REFIND_FAILURE_QUEUE) wq = read_pairs<ptam_map_pair>(in, W);
            else
                for (auto& p : w) in >> p;
            if (mode == PTAM_MAP_REFIND_NEW_POINTS) {
                bad.resize((size_t)W);
                for (auto& b : bad) in >> b;
            }
            const void* work = mode == PTAM_MAP_REFIND_FAILURE_QUEUE ? (const void*)wq.data() : (const void*)w.data();
            plan = MrPlan{};
            if (!mr_plan(mode, K, N, W, work, [&](int e, int) { return bad[(size_t)e] != 0; }, per_pass, &plan)) {
                std::printf("plan 0\n");
                continue;
            }
            const ptam_map_refind_result r = mr_plan_nothing(plan, false);   // (points_consumed / n_bad_points of an unstopped call)
            std::printf("plan 1 %d %lld %d %d %d |", plan.pairs, plan.bound, plan.per_pass, r.points_consumed, r.n_bad_points);
            for (int p : plan.wpts) std::printf(" %d", p);
            std::printf(" |");
            for (int e : plan.wentry) std::printf(" %d", e);
            std::printf(" |");
            for (int k : plan.wrank) std::printf(" %d", k);
            std::printf(" |");
            for (const auto& q : plan.wq) std::printf(" %d %d", q.kf, q.point);
            std::printf("\n");
        } else if (what == "stop") {
            int visited, consumed, n_bad;
            in >> visited;
            mr_plan_consumed(plan, visited, true, &consumed, &n_bad);
            std::printf("stop %d %d\n", consumed, n_bad);
        } else {
            std::fprintf(stderr, "map_host_check: unknown case '%s'\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
