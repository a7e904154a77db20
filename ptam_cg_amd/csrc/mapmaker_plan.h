// mapmaker_plan.h — what MapMaker::run() decides (src/MapMaker.cc:57-114): which stage of an iteration runs, what a bundle, a new
// keyframe and a reset make of the mbBundleConverged_* flags, when AddKeyFrame asks a running bundle to stop, and the draw that
// stands for rand() % 20.  Host only and no HIP: a plain C++ compiler builds it (tools/mapmaker/mapmaker_plan_check.cc runs the
// whole decision table on the CPU).  ptam_mapmaker_step (mapmaker_run.hip) asks each question when it reaches the stage, with the
// queue as it stands then, as the reference does.
#pragma once
#include <cstdint>

struct MmFlags {
    bool converged_recent, converged_full;   // mbBundleConverged_Recent / _Full
    bool bundle_running, abort_requested;    // mbBundleRunning / mbBundleAbortRequested
};

// the n-th output of splitmix64 seeded with `seed`: a function of (seed, n), so a run can be replayed from its draw count
inline uint64_t mm_splitmix64(uint64_t seed, uint64_t n) {
    uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- the conditions of :88-112
inline bool mm_want_bundle_recent(const MmFlags& f, int queue) { return !f.converged_recent && queue == 0; }                     // :88
inline bool mm_want_refind_new(const MmFlags& f, int queue) { return f.converged_recent && queue == 0; }                          // :93
inline bool mm_want_bundle_all(const MmFlags& f, int queue) { return f.converged_recent && !f.converged_full && queue == 0; }    // :98
// :103 — the reference's && chain: rand() is called, and here a draw consumed, only when both flags are set; the queue is looked
// at behind the draw
inline bool mm_want_refind_failure(const MmFlags& f, int queue, uint64_t seed, int period, uint64_t* draws) {
    if (!(f.converged_recent && f.converged_full)) return false;
    const bool hit = mm_splitmix64(seed, (*draws)++) % (uint64_t)(period > 0 ? period : 1) == 0;
    return hit && queue == 0;
}
inline bool mm_want_add_keyframe(int queue) { return queue > 0; }   // :111

// ---- what the stages make of the flags
enum { MM_RECENT_MIN_KEYFRAMES = 8 };
// BundleAdjustRecent on a small map (:790-793): does not run, and says it has converged.  -> the bundle runs
inline bool mm_bundle_recent_runs(MmFlags& f, int n_kf) {
    if (n_kf >= MM_RECENT_MIN_KEYFRAMES) return true;
    f.converged_recent = true;
    return false;
}
inline void mm_bundle_begin(MmFlags& f) { f.bundle_running = true; }   // :841
// :895-913, after Compute(): accepted = nAccepted > 0, converged = b.Converged()
inline void mm_bundle_end(MmFlags& f, bool recent, bool accepted, bool converged) {
    if (accepted) {
        if (recent) f.converged_recent = false;
        f.converged_full = false;
    }
    if (converged) {
        f.converged_recent = true;
        if (!recent) f.converged_full = true;
    }
    f.bundle_running = false;
    f.abort_requested = false;
}
// AddKeyFrame, on the tracker's thread under the handle's mutex (:486-487): only a running bundle is asked to stop
inline void mm_keyframe_queued(MmFlags& f) {
    if (f.bundle_running) f.abort_requested = true;
}
inline void mm_keyframe_added(MmFlags& f) { f.converged_full = f.converged_recent = false; }   // :516-517
inline void mm_reset(MmFlags& f) {   // :45-50
    f.bundle_running = false;
    f.converged_full = f.converged_recent = true;
    f.abort_requested = false;
}

// ---- MapMaker::InitFromStereo (:268-405) run by the step for the tracker's thread (ptam_mapmaker_request_init)
enum { MM_INIT_NONE = 0, MM_INIT_PENDING = 1, MM_INIT_DONE = 2 };   // PTAM_MM_INIT_* (ptam_hip.h)
// one request at a time, and only for a map without a keyframe (the reference calls InitFromStereo while !mMap.IsGood())
inline bool mm_init_request_allowed(int init_state, bool map_has_keyframe) { return init_state != MM_INIT_PENDING && !map_has_keyframe; }
// the step runs a pending request in front of the :79 idle test; a request that a reset finds pending is dropped
inline bool mm_want_init(int init_state) { return init_state == MM_INIT_PENDING; }
// A map was made: the flags as the loop of :387-394 leaves them — BundleAdjustAll converged, which sets both (:905-910), and nothing
// runs.  No map (`return false` at :286, :294 or :393; too few points): the caller's Reset(), :45-50.
inline void mm_init_end(MmFlags& f, bool map_made) {
    if (!map_made) {
        mm_reset(f);
        return;
    }
    f.converged_recent = f.converged_full = true;
    f.bundle_running = false;
    f.abort_requested = false;
}
