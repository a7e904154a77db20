// snapshot_slots_check.cc — the host state machine of ptam_map_snapshot (ptam_cg_amd/csrc/snapshot_slots.h: three slots, one mutex, a
// generation) between a publisher thread and reader threads, for a run under ThreadSanitizer on the CPU.  No HIP: a slot's device
// memory is a plain array here, the publisher's kernel a loop that writes it, a take's copy a loop that reads it.
//
//     g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -I ptam_cg_amd/csrc tools/mapmaker/snapshot_slots_check.cc -o snapshot_slots_check
//     ./snapshot_slots_check [publishes] [readers]
//
// Checked, besides what the sanitizer reports: a reader never sees a slot whose words differ (a half-written generation) or whose
// stamp is not the generation it was told; the generations a reader sees increase; the last take sees the last publish; with one
// reader the publisher never waits for a slot.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "snapshot_slots.h"

enum { WORDS = 4096 };
struct Payload {
    long long stamp;
    long long words[WORDS];
};

int main(int argc, char** argv) {
    const int publishes = argc > 1 ? std::atoi(argv[1]) : 2000, n_readers = argc > 2 ? std::atoi(argv[2]) : 1;
    SnapSlots slots;
    static Payload slot[SnapSlots::SLOTS];
    std::atomic<int> errors{0};
    std::atomic<bool> done{false};

    std::thread publisher([&] {
        for (int p = 1; p <= publishes; p++) {
            const int s = slots.begin_write();
            if (s < 0) {
                errors++;
                return;
            }
            const long long gen = slots.next_generation();
            for (int i = 0; i < WORDS; i++) slot[s].words[i] = gen;   // (the gather kernel and its wait)
            slot[s].stamp = gen;
            if (p % 97 == 0) {   // a refused or failed publish: the current generation stays
                slots.abort_write();
                continue;
            }
            if (slots.commit_write() != gen) errors++;
        }
        done = true;
    });
    std::vector<std::thread> readers;
    std::vector<long long> last_seen((size_t)n_readers, 0);
    for (int r = 0; r < n_readers; r++)
        readers.emplace_back([&, r] {
            long long have = 0;
            for (;;) {
                const bool last = done.load();
                long long gen = 0;
                const int s = slots.begin_read(have, &gen);
                if (s >= 0) {
                    bool whole = slot[s].stamp == gen;
                    for (int i = 0; i < WORDS; i++) whole = whole && slot[s].words[i] == gen;   // (the copy and its wait)
                    slots.end_read(s);
                    if (!whole || gen <= have) errors++;
                    have = gen;
                } else if (s == SnapSlots::UNCHANGED && gen != have)
                    errors++;
                if (last) break;
            }
            last_seen[(size_t)r] = have;
        });
    publisher.join();
    for (std::thread& t : readers) t.join();
    long long gen = 0;
    const int held = slots.begin_read(-1, &gen);
    if (held >= 0) slots.end_read(held);
    const long long want = publishes - publishes / 97;
    for (long long seen : last_seen)
        if (seen != want) errors++;
    std::printf("publishes %d (aborted %d) readers %d: last generation %lld, every reader ended on it: %s, errors %d\n", publishes, publishes / 97,
                n_readers, gen, errors == 0 ? "yes" : "no", errors.load());
    return errors == 0 && gen == want ? 0 : 1;
}
