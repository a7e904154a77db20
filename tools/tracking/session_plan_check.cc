// session_plan_check.cc — the stage rule of a session (ptam_cg_amd/csrc/tracker_plan.h, Tracker::TrackForInitialMap, src/Tracker.cc:311-347)
// on the CPU, one question per input line, one answer line each (tests/test_camera_session_plan.py asks the whole table).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ptam_cg_amd/csrc tools/tracking/session_plan_check.cc -o session_plan_check
//   action stage poke n_good min_good init_state init_status   -> "action consumes_poke"
//   pool clones a b tag                                         -> the clone states after clones_out(a, b, tag), release(tag), reset()
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "tracker_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string what;
        long long a = 0, b = 0, c = 0, d = 0, e = 0, f = 0;
        s >> what >> a >> b >> c >> d >> e >> f;
        if (what == "action") {
            const int act = tp_session_action((int)a, b != 0, (int)c, (int)d, (int)e, (int)f);
            std::printf("%d %d\n", act, tp_session_consumes_poke(act, b != 0));
        } else if (what == "pool") {
            TpPool p(1, (int)a);
            p.clones_out((int)b, (int)c, d);
            for (int st : p.clone_state) std::printf("%d ", st);
            std::printf("%d ", p.release(d));
            for (int st : p.clone_state) std::printf("%d ", st);
            p.reset();
            std::printf("%d\n", p.count(p.clone_state, TpPool::FREE));
        } else
            return 4;
    }
    return 0;
}
