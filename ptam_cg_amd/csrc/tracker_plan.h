// tracker_plan.h — the host's side of a tracked frame's two random orders (the stand-in for std::random_shuffle at
// src/Tracker.cc:483-484 and :597-600): the key of a point and the order the keys define.  Host only and no HIP: a plain C++
// compiler builds it.  ptam_shuffle_order_host is this function; the device's draw (tracker_run.hip) is held to it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "mapmaker_plan.h"   // mm_splitmix64

// order w (0: the level lists, 1: the chop of the fine set) of frame `frame`, point i: a random high word over the point's index.
// Distinct for distinct i, so sorting the keys is a total order; 2 * frame + w wraps at 2^32 (frames 2^31 apart draw alike).
inline uint64_t tp_shuffle_key(uint64_t seed, uint64_t frame, int w, uint32_t i) {
    const uint64_t draw = mm_splitmix64(seed, ((2 * frame + (uint64_t)w) << 32) | i);
    return (draw >> 32) << 32 | i;
}

// the low words of the n keys sorted ascending
inline void tp_shuffle_order(uint64_t seed, uint64_t frame, int w, int n, int32_t* out) {
    std::vector<uint64_t> keys((size_t)(n > 0 ? n : 0));
    for (int i = 0; i < n; i++) keys[(size_t)i] = tp_shuffle_key(seed, frame, w, (uint32_t)i);
    std::sort(keys.begin(), keys.end());
    for (int i = 0; i < n; i++) out[i] = (int32_t)(uint32_t)keys[(size_t)i];
}

// ---- what the tracker's thread decides behind a tracked frame (src/Tracker.cc:146-166), and the pools of a camera tracker ----------
// branch: PTAM_FRAME_TRACKED 0 / RECOVERED 1 / RECOVERY_FAILED 2; quality: PTAM_TRACK_GOOD is 1; frame: mnFrame after the frame
// (:111 counts it first); last_dropped: mnLastKeyFrameDropped; queue: MapMaker::QueueSize(); records: the report's n_records.
enum { TP_NEITHER = 0, TP_ADD = 1, TP_NOTE = 2 };
// :158 isTrackGood && isFarEnough && isQueueNeed (isNeedFrame is commented out there) on the tracking branch — and a frame that found
// nothing has no measurements to become a keyframe's.  Otherwise a frame that was tracked (or recovered) and found points is noted:
// CalcPoseUpdate's outlier / inlier counts (:989-997) happen on every TrackMap
inline int tp_decide(int branch, int quality, int frame, int last_dropped, int gap, int queue, int max_queue, int records) {
    if (branch != 0 && branch != 1) return TP_NEITHER;
    if (records <= 0) return TP_NEITHER;
    if (branch == 0 && quality == 1 && frame - last_dropped > gap && queue < max_queue) return TP_ADD;
    return TP_NOTE;
}
// could the frame that is about to be tracked end in TP_ADD?  (asked before the chain: a keyframe clone must be free then)
inline bool tp_may_add(int lost_frames, int frame_before, int last_dropped, int gap) { return lost_frames < 3 && frame_before + 1 - last_dropped > gap; }

// ---- Tracker::TrackForInitialMap (src/Tracker.cc:311-347) and what TrackFrame does around it: the stage rule of a session ---------------
// stage: mnInitialStage.  poke: mbUserPressedSpacebar.  n_good: TrailTracking_Advance's return value (looked at in STARTED only).
// init_state / init_status: what ptam_mapmaker_init_poll says of the handle's request — MM_INIT_NONE when it has none out, which in
// COMPLETE means that it tracks its map; init_status PTAM_INIT_MAP_* (0: a map was made).
enum { TP_TRAILS_NOT_STARTED = 0, TP_TRAILS_STARTED = 1, TP_TRAILS_COMPLETE = 2 };
enum {
    TP_S_IDLE = 0,         // :321-323  nothing but MakeKeyFrame_Lite and the frame count
    TP_S_START = 1,        // :315-320  TrailTracking_Start, stage STARTED
    TP_S_RESET = 2,        // :329-332  too few good trails: Reset(), stage NOT_STARTED (the poke is cleared with it, :52)
    TP_S_KEEP = 3,         // :344-345  the trails advanced, nothing else
    TP_S_REQUEST = 4,      // :335-343  the matches and the two keyframes go to the mapmaker, stage COMPLETE
    TP_S_WAIT = 5,         // the request has not been run yet: as IDLE (the reference's tracker is inside InitFromStereo meanwhile)
    TP_S_BEGIN = 6,        // a map was made: the model at the tracker's pose (:341), then this frame is tracked
    TP_S_INIT_FAILED = 7,  // no map was made: the tracker's side of Reset() (the reference stays in COMPLETE without a map for ever)
    TP_S_TRACK = 8         // src/Tracker.cc:127-176
};
inline int tp_session_action(int stage, bool poke, int n_good, int min_good, int init_state, int init_status) {
    if (stage == TP_TRAILS_NOT_STARTED) return poke ? TP_S_START : TP_S_IDLE;
    if (stage == TP_TRAILS_STARTED) {
        if (n_good < min_good) return TP_S_RESET;
        return poke ? TP_S_REQUEST : TP_S_KEEP;
    }
    if (init_state == MM_INIT_NONE) return TP_S_TRACK;
    if (init_state == MM_INIT_PENDING) return TP_S_WAIT;
    return init_status == 0 ? TP_S_BEGIN : TP_S_INIT_FAILED;
}
// does the action consume the poke (mbUserPressedSpacebar = false at :317, :337 and in Reset(), :52)?
inline bool tp_session_consumes_poke(int action, bool poke) { return poke && (action == TP_S_START || action == TP_S_REQUEST || action == TP_S_RESET); }

// The reports and the keyframe clones of one camera, by index.  A report is FREE, HELD by the frame in flight, or OUT with the
// mapmaker under a tag.  A clone is FREE, OUT under a tag, or IN_MAP: its tag came back, so the mapmaker's step has inserted it and
// the map names it — it returns only with reset().  (A tag that a mapmaker reset dropped also comes back; the tracker's reset that
// belongs to it, Tracker::Reset, frees everything.)
struct TpPool {
    enum { FREE = 0, HELD = 1, OUT = 2, IN_MAP = 3 };
    std::vector<int> report_state, clone_state;
    std::vector<int64_t> report_tag, clone_tag;
    TpPool(int reports = 0, int clones = 0)
        : report_state((size_t)reports, FREE), clone_state((size_t)clones, FREE), report_tag((size_t)reports, 0), clone_tag((size_t)clones, 0) {}
    static int first(const std::vector<int>& v, int what) {
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] == what) return (int)i;
        return -1;
    }
    int free_report() const { return first(report_state, FREE); }
    int free_clone() const { return first(clone_state, FREE); }
    int count(const std::vector<int>& v, int what) const {
        int n = 0;
        for (int s : v) n += s == what;
        return n;
    }
    // the frame in flight takes a report; -1: none is free
    int hold_report() {
        const int i = free_report();
        if (i >= 0) report_state[(size_t)i] = HELD;
        return i;
    }
    void return_report(int i) { report_state[(size_t)i] = FREE; }
    // NoteFrame (clone < 0) or AddKeyFrame: report (HELD) and clone (FREE) go out under the tag
    void hand_over(int report, int clone, int64_t tag) {
        report_state[(size_t)report] = OUT;
        report_tag[(size_t)report] = tag;
        if (clone >= 0) {
            clone_state[(size_t)clone] = OUT;
            clone_tag[(size_t)clone] = tag;
        }
    }
    // a tag came back from the mapmaker -> how many objects it named here (0: not ours)
    int release(int64_t tag) {
        int n = 0;
        for (size_t i = 0; i < report_state.size(); i++)
            if (report_state[i] == OUT && report_tag[i] == tag) report_state[i] = FREE, n++;
        for (size_t i = 0; i < clone_state.size(); i++)
            if (clone_state[i] == OUT && clone_tag[i] == tag) clone_state[i] = IN_MAP, n++;
        return n;
    }
    // the two keyframes of an initialisation request go out under its tag, without a report
    void clones_out(int a, int b, int64_t tag) {
        clone_state[(size_t)a] = clone_state[(size_t)b] = OUT;
        clone_tag[(size_t)a] = clone_tag[(size_t)b] = tag;
    }
    void reset() {
        std::fill(report_state.begin(), report_state.end(), (int)FREE);
        std::fill(clone_state.begin(), clone_state.end(), (int)FREE);
    }
};
