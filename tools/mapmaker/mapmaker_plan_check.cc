// mapmaker_plan_check.cc — ptam_cg_amd/csrc/mapmaker_plan.h on the CPU, one question per input line, one answer line each
// (tests/test_mapmaker_plan.py asks the whole decision table and compares with its own restatement of src/MapMaker.cc:57-114).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ptam_cg_amd/csrc tools/mapmaker/mapmaker_plan_check.cc -o mapmaker_plan_check
//   want R F queue seed period draws    -> "recent new all failure draws' add": the conditions of :88-112 on these flags
//   recent R F n_kf                     -> "runs R' F'": BundleAdjustRecent's size test (:790-793)
//   end R F recent accepted converged   -> "R' F' running abort": a bundle begun, an abort requested while it runs, then :895-913
//   queued running                      -> "abort": AddKeyFrame's rule (:486-487)
//   added R F | reset R F               -> "R' F' running abort": :516-517 | :45-50
//   mix seed n                          -> the n-th draw
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "mapmaker_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        s >> what;
        MmFlags f = {};
        unsigned long long a = 0, b = 0, c = 0, d = 0, e = 0, g = 0;
        s >> a >> b >> c >> d >> e >> g;
        f.converged_recent = a != 0;
        f.converged_full = b != 0;
        if (what == "want") {
            uint64_t draws = g;
            const int queue = (int)c;
            const bool r = mm_want_bundle_recent(f, queue), n = mm_want_refind_new(f, queue), al = mm_want_bundle_all(f, queue);
            const bool fl = mm_want_refind_failure(f, queue, d, (int)e, &draws);
            std::printf("%d %d %d %d %llu %d\n", r, n, al, fl, (unsigned long long)draws, mm_want_add_keyframe(queue));
        } else if (what == "recent") {
            const bool runs = mm_bundle_recent_runs(f, (int)c);
            std::printf("%d %d %d\n", runs, f.converged_recent, f.converged_full);
        } else if (what == "end") {
            mm_bundle_begin(f);
            mm_keyframe_queued(f);
            if (!f.bundle_running || !f.abort_requested) return 3;
            mm_bundle_end(f, c != 0, d != 0, e != 0);
            std::printf("%d %d %d %d\n", f.converged_recent, f.converged_full, f.bundle_running, f.abort_requested);
        } else if (what == "queued") {
            MmFlags q = {};
            q.bundle_running = a != 0;
            mm_keyframe_queued(q);
            std::printf("%d\n", q.abort_requested);
        } else if (what == "added" || what == "reset") {
            f.bundle_running = f.abort_requested = true;
            if (what == "added") {
                f.bundle_running = f.abort_requested = false;
                mm_keyframe_added(f);
            } else
                mm_reset(f);
            std::printf("%d %d %d %d\n", f.converged_recent, f.converged_full, f.bundle_running, f.abort_requested);
        } else if (what == "mix")
            std::printf("%llu\n", (unsigned long long)mm_splitmix64(a, b));
        else
            return 4;
    }
    return 0;
}
