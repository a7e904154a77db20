// snapshot_slots.h — the host state of a ptam_map_snapshot (ptam_hip.h): which of its three slots is current, which one the
// publish is writing, which ones a take is copying, and the generation number.  Plain C++, no HIP: tools/mapmaker/
// snapshot_slots_check.cc runs it between two threads under -fsanitize=thread.
//
// The rules:
//   * the publisher asks for a slot that is neither current nor being read, fills it on its own queue, waits for that queue, and
//     only then commits: the slot becomes current and the generation moves, under the mutex;
//   * a reader takes the current slot under the mutex (its reader count goes up), copies from it on its own queue, waits for that
//     queue, and gives the slot back under the mutex;
//   * nothing else is shared.  What a slot holds is written before the commit and read after begin_read: the mutex orders the two.
// With one reader a free slot always exists (current + one being read leave one), so neither side waits for the other's device
// work.  With more readers than that, each on a slot of its own, begin_write waits on the condition variable until a reader
// gives its slot back — bounded by that reader's copy.
#pragma once
#include <condition_variable>
#include <mutex>

struct SnapSlots {
    enum { SLOTS = 3, NEVER = -1, UNCHANGED = -2 };
    std::mutex mu;
    std::condition_variable freed;
    int current = NEVER;             // the slot a take copies from
    int writing = NEVER;             // the slot a publish is filling (one publisher at a time)
    int readers[SLOTS] = {0, 0, 0};
    long long generation = 0;        // of the current slot; 0: never published into

    // the publisher's slot, or NEVER when a publish is already under way (two publishers: the caller's error)
    int begin_write() {
        std::unique_lock<std::mutex> lk(mu);
        if (writing != NEVER) return NEVER;
        for (;;) {
            for (int s = 0; s < SLOTS; s++)
                if (s != current && readers[s] == 0) return writing = s;
            freed.wait(lk);
        }
    }
    // the publish failed or was refused: the slot is nobody's, the current generation stays
    void abort_write() {
        std::lock_guard<std::mutex> lk(mu);
        writing = NEVER;
    }
    // the publisher's queue is idle: the slot is the current one -> its generation
    long long commit_write() {
        std::lock_guard<std::mutex> lk(mu);
        current = writing;
        writing = NEVER;
        return ++generation;
    }
    // what the next commit will return (the publisher stamps the slot with it before the commit; only the publisher moves it)
    long long next_generation() {
        std::lock_guard<std::mutex> lk(mu);
        return generation + 1;
    }
    // the current slot for a reader that holds generation `have` (0: none): NEVER, UNCHANGED, or the slot with its count raised
    int begin_read(long long have, long long* gen) {
        std::lock_guard<std::mutex> lk(mu);
        *gen = generation;
        if (current == NEVER) return NEVER;
        if (generation == have) return UNCHANGED;
        readers[current]++;
        return current;
    }
    void end_read(int slot) {
        {
            std::lock_guard<std::mutex> lk(mu);
            readers[slot]--;
        }
        freed.notify_all();
    }
    // for reserve / destroy: the slot is neither current, nor being written, nor being read
    bool idle(int slot) {
        std::lock_guard<std::mutex> lk(mu);
        return slot != current && slot != writing && readers[slot] == 0;
    }
};
