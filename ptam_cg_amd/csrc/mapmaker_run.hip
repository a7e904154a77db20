// mapmaker_run.hip — ptam_mapmaker (ptam_hip.h): one iteration of MapMaker::run() (src/MapMaker.cc:57-114) as one call on a resident
// map.  Host code only: every stage is a call that exists (ptam_rmap_bundle_adjust_routed, ptam_rmap_refind_queue,
// ptam_rmap_note_reports, ptam_rmap_handle_bad_points, ptam_rmap_insert_keyframe_report, ptam_rmap_publish, ptam_rmap_clear), and
// every decision is a function of mapmaker_plan.h.  What is the handle's own: the keyframe queue, the pending reports and the
// released tags under one mutex; the flags, written by the step and by AddKeyFrame under that mutex; the two bytes the device calls
// poll from the host between their launches (the bundle's abort, the re-find's stop).  The first map is made here too: the tracker's
// thread leaves a request (ptam_mapmaker_request_init: the two keyframes and a copy of the matches), the step runs
// ptam_rmap_init_from_stereo on the map's own thread and publishes, and the tracker's thread polls for the outcome.
#include <atomic>
#include <deque>
#include <mutex>
#include <vector>

#include "keyframe.h"
#include "mapmaker_plan.h"
#include "rmap_internal.h"

namespace {
struct MmKeyFrame {
    const ptam_kf* kf;
    double pose[12];
    int fixed;
    ptam_frame_report* report;
    double depth_mean, depth_sigma;
    int64_t tag;
};
struct MmNote {
    ptam_frame_report* report;
    int64_t tag;
};
struct MmInit {   // MapMaker::InitFromStereo's arguments, as the tracker's thread left them
    const ptam_kf* first;
    ptam_kf* second;
    std::vector<ptam_trail> matches;
    ptam_rmap_init_opts opts;
    int64_t tag;
};
}   // namespace

struct ptam_mapmaker {
    ptam_rmap* map;
    ptam_refinder* finder;
    ptam_map_snapshot* snapshot;   // nullable
    ptam_mapmaker_opts opts;
    std::mutex mu;                 // guards everything below but the two atomics
    std::deque<MmKeyFrame> queue;
    std::vector<MmNote> notes;
    std::deque<int64_t> released;
    MmFlags flags;
    uint64_t draws;
    volatile unsigned char abort_byte;       // mbBundleAbortRequested, as ptam_ba_compute polls it
    volatile unsigned char queue_nonempty;   // !mvpKeyFrameQueue.empty(), as the re-find polls it (:1053)
    std::atomic<bool> reset_requested, reset_done;
    // the initialisation the tracker's thread asks for
    int init_state;                          // MM_INIT_*
    MmInit init;
    ptam_rmap_init_result init_result;       // of the last request, readable until the next one
    volatile unsigned char init_stop;        // mbResetRequested as InitFromStereo's last loop reads it (:392): raised by request_reset
};

static int mm_queue_size(ptam_mapmaker* mm) {
    std::lock_guard<std::mutex> g(mm->mu);
    return (int)mm->queue.size();
}

// a request ends (under the mutex): its tag goes home and the outcome becomes readable.  r == nullptr: it never ran — STOPPED
static void mm_init_finish(ptam_mapmaker* mm, const ptam_rmap_init_result* r) {
    if (r) mm->init_result = *r;
    else {
        std::memset(&mm->init_result, 0, sizeof mm->init_result);
        mm->init_result.status = PTAM_INIT_MAP_STOPPED;
        mm->init_result.n_matches = (int)mm->init.matches.size();
    }
    mm->released.push_back(mm->init.tag);
    mm->init.matches.clear();
    mm->init_state = MM_INIT_DONE;
}

// MapMaker::Reset (:37-51)
static int mm_do_reset(ptam_mapmaker* mm) {
    const int rc = ptam_rmap_clear(mm->map);
    std::lock_guard<std::mutex> g(mm->mu);
    for (const MmKeyFrame& k : mm->queue) mm->released.push_back(k.tag);
    for (const MmNote& n : mm->notes) mm->released.push_back(n.tag);
    mm->queue.clear();
    mm->notes.clear();
    if (mm_want_init(mm->init_state)) mm_init_finish(mm, nullptr);   // a pending request is dropped
    mm->init_stop = 0;
    mm_reset(mm->flags);
    mm->abort_byte = mm->queue_nonempty = 0;
    mm->reset_done = true;
    mm->reset_requested = false;
    return rc;
}

// BundleAdjustRecent / BundleAdjustAll with the flags of :790-793, :841, :895-913.  -> the bundle was accepted, in *accepted
static int mm_bundle(ptam_mapmaker* mm, bool recent, ptam_map_ba_result* ba, ptam_map_outliers_result* out, bool* accepted) {
    {
        std::lock_guard<std::mutex> g(mm->mu);
        if (recent && !mm_bundle_recent_runs(mm->flags, mm->map->n[RM_N_KF])) return PTAM_OK;
        mm_bundle_begin(mm->flags);
    }
    const int rc = ptam_rmap_bundle_adjust_routed(mm->map, &mm->opts.ba, recent ? PTAM_MAP_BA_RECENT : PTAM_MAP_BA_ALL, &mm->abort_byte, ba, out);
    std::lock_guard<std::mutex> g(mm->mu);
    if (rc) {   // (no result to read the flags from: nothing runs any more, the flags stay)
        mm->flags.bundle_running = false;
        mm->abort_byte = 0;
        return rc;
    }
    mm_bundle_end(mm->flags, recent, ba->accepted > 0, ba->converged != 0);
    mm->abort_byte = 0;
    *accepted = *accepted || ba->accepted > 0;
    return PTAM_OK;
}

extern "C" {

int ptam_mapmaker_opts_default(ptam_mapmaker_opts* o) {
    ARG_TRY(o);
    std::memset(o, 0, sizeof *o);
    ptam_ba_opts_default(&o->ba);
    ptam_epipolar_opts_default(&o->insert.epipolar);
    const int levels[4] = {3, 0, 1, 2};   // :511-514
    o->insert.epipolar.n_levels = 4;
    for (int i = 0; i < 4; i++) o->insert.epipolar.levels[i] = levels[i];
    o->insert.target_kf = -1;
    o->failure_period = 20;
    return PTAM_OK;
}

int ptam_mapmaker_create(ptam_rmap* map, ptam_refinder* finder, ptam_map_snapshot* snapshot, const ptam_mapmaker_opts* opts, ptam_mapmaker** out) {
    ARG_TRY(map && finder && out);
    ARG_TRY(!opts || opts->failure_period >= 1);
    ptam_mapmaker* mm = new ptam_mapmaker();
    mm->map = map;
    mm->finder = finder;
    mm->snapshot = snapshot;
    if (opts) mm->opts = *opts;
    else if (int rc = ptam_mapmaker_opts_default(&mm->opts)) {
        delete mm;
        return rc;
    }
    mm_reset(mm->flags);
    mm->draws = 0;
    mm->abort_byte = mm->queue_nonempty = 0;
    mm->reset_requested = false;
    mm->reset_done = true;
    mm->init_state = MM_INIT_NONE;
    std::memset(&mm->init_result, 0, sizeof mm->init_result);
    mm->init_stop = 0;
    *out = mm;
    return PTAM_OK;
}

int ptam_mapmaker_destroy(ptam_mapmaker* mm) {
    delete mm;
    return PTAM_OK;
}

int ptam_mapmaker_add_keyframe(ptam_mapmaker* mm, const ptam_kf* clone, const double pose12[12], int fixed, ptam_frame_report* report,
                               double depth_mean, double depth_sigma, int64_t tag) {
    ARG_TRY(mm && clone && pose12 && report);
    MmKeyFrame k;
    k.kf = clone;
    std::memcpy(k.pose, pose12, sizeof k.pose);
    k.fixed = fixed ? 1 : 0;
    k.report = report;
    k.depth_mean = depth_mean;
    k.depth_sigma = depth_sigma;
    k.tag = tag;
    std::lock_guard<std::mutex> g(mm->mu);
    mm->queue.push_back(k);
    mm->queue_nonempty = 1;
    mm_keyframe_queued(mm->flags);
    if (mm->flags.abort_requested) mm->abort_byte = 1;
    return PTAM_OK;
}

int ptam_mapmaker_note_frame(ptam_mapmaker* mm, ptam_frame_report* report, int64_t tag) {
    ARG_TRY(mm && report);
    std::lock_guard<std::mutex> g(mm->mu);
    mm->notes.push_back(MmNote{report, tag});
    return PTAM_OK;
}

int ptam_mapmaker_queue_size(ptam_mapmaker* mm, int32_t* out) {
    ARG_TRY(mm && out);
    *out = mm_queue_size(mm);
    return PTAM_OK;
}

int ptam_mapmaker_request_reset(ptam_mapmaker* mm) {
    ARG_TRY(mm);
    std::lock_guard<std::mutex> g(mm->mu);   // (against mm_do_reset's two stores: a request between them would be wiped)
    mm->reset_done = false;
    mm->reset_requested = true;
    mm->init_stop = 1;
    return PTAM_OK;
}

int ptam_mapmaker_request_init(ptam_mapmaker* mm, const ptam_kf* first, ptam_kf* second, int n_matches, const ptam_trail* matches,
                               const ptam_rmap_init_opts* opts, int64_t tag) {
    ARG_TRY(mm && first && second && matches && n_matches >= 4);
    MmInit in;
    in.first = first;
    in.second = second;
    in.matches.assign(matches, matches + n_matches);
    in.tag = tag;
    if (opts) in.opts = *opts;
    else if (int rc = ptam_rmap_init_opts_default(&in.opts)) return rc;
    std::lock_guard<std::mutex> g(mm->mu);
    // (the map's keyframe count is a host word that only the mapmaker's thread writes, and only while it makes, grows or clears a map:
    // a tracker asks here while no map exists, when that thread idles at :79)
    const bool has_kf = __atomic_load_n(&mm->map->n[RM_N_KF], __ATOMIC_RELAXED) > 0;
    if (!mm_init_request_allowed(mm->init_state, has_kf)) {
        ptam_set_error("mapmaker_request_init: %s", mm->init_state == MM_INIT_PENDING ? "a request is pending" : "the map has a keyframe");
        return PTAM_E_STATE;
    }
    mm->init = std::move(in);
    mm->init_state = MM_INIT_PENDING;
    return PTAM_OK;
}

int ptam_mapmaker_init_poll(ptam_mapmaker* mm, int32_t* state, ptam_rmap_init_result* out) {
    ARG_TRY(mm && state);
    std::lock_guard<std::mutex> g(mm->mu);
    *state = mm->init_state;
    if (out && mm->init_state == MM_INIT_DONE) *out = mm->init_result;
    return PTAM_OK;
}

int ptam_mapmaker_reset_done(ptam_mapmaker* mm, int32_t* out) {
    ARG_TRY(mm && out);
    *out = mm->reset_done ? 1 : 0;
    return PTAM_OK;
}

int ptam_mapmaker_flags(ptam_mapmaker* mm, int32_t* converged_recent, int32_t* converged_full, int32_t* bundle_running) {
    ARG_TRY(mm && converged_recent && converged_full && bundle_running);
    std::lock_guard<std::mutex> g(mm->mu);
    *converged_recent = mm->flags.converged_recent;
    *converged_full = mm->flags.converged_full;
    *bundle_running = mm->flags.bundle_running;
    return PTAM_OK;
}

int ptam_mapmaker_set_flags(ptam_mapmaker* mm, int converged_recent, int converged_full) {
    ARG_TRY(mm);
    std::lock_guard<std::mutex> g(mm->mu);
    mm->flags.converged_recent = converged_recent != 0;
    mm->flags.converged_full = converged_full != 0;
    return PTAM_OK;
}

int ptam_mapmaker_released(ptam_mapmaker* mm, int cap, int64_t* tags, int32_t* n) {
    ARG_TRY(mm && n && cap >= 0 && (cap == 0 || tags));
    std::lock_guard<std::mutex> g(mm->mu);
    int k = 0;
    for (; k < cap && !mm->released.empty(); k++) {
        tags[k] = mm->released.front();
        mm->released.pop_front();
    }
    *n = k;
    return PTAM_OK;
}

// the stages; res->status and res->stages say how far they came, whatever is returned
static int mm_step_stages(ptam_mapmaker* mm, ptam_mapmaker_step_result* res) {
    const auto finish = [&](int status) {
        res->status = status;
        return PTAM_OK;
    };
#define MM_CHECK_RESET                                \
    if (mm->reset_requested) {                        \
        if (int rc__ = mm_do_reset(mm)) return rc__;  \
        return finish(PTAM_MM_RESET);                 \
    }
    MM_CHECK_RESET;
    bool want;
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_init(mm->init_state);
    }
    if (want) {   // InitFromStereo, which the reference runs on the tracker's thread while this loop idles (src/Tracker.cc:341)
        // (mm->init is the step's until the state changes: a second request is refused while this one is pending)
        ptam_rmap_init_result r;
        std::memset(&r, 0, sizeof r);
        int rc = ptam_rmap_init_from_stereo(mm->map, mm->init.first, mm->init.second, nullptr, (int)mm->init.matches.size(),
                                            mm->init.matches.data(), &mm->init.opts, &mm->init_stop, &r);
        if (rc) r.status = PTAM_INIT_MAP_STOPPED;   // (refused or failed: no map, the error is the step's)
        const bool made = !rc && r.status == PTAM_INIT_MAP_OK;
        res->stages |= PTAM_MM_STAGE_INIT;
        {
            std::lock_guard<std::mutex> g(mm->mu);
            mm_init_end(mm->flags, made);
        }
        if (made && mm->snapshot) {
            rc = ptam_rmap_publish(mm->map, mm->snapshot, &res->publish);
            if (!rc) res->stages |= PTAM_MM_STAGE_PUBLISH;
        }
        {
            std::lock_guard<std::mutex> g(mm->mu);
            mm_init_finish(mm, &r);   // (DONE only now: a tracker that reads it takes a snapshot that holds the map)
        }
        if (rc) return rc;
        if (made) return finish(PTAM_MM_INIT);
        MM_CHECK_RESET;   // (STOPPED: the reset that stopped it)
    }
    if (mm->map->n[RM_N_KF] == 0) return finish(PTAM_MM_IDLE);   // :79
    bool changed = false;   // what a tracker has to see: an accepted bundle, removed points, a new keyframe

    MM_CHECK_RESET;   // :86-89
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_bundle_recent(mm->flags, (int)mm->queue.size());
    }
    if (want) {
        if (int rc = mm_bundle(mm, true, &res->recent, &res->recent_outliers, &changed)) return rc;
        if (res->recent.ran) res->stages |= PTAM_MM_STAGE_BUNDLE_RECENT;
    }

    MM_CHECK_RESET;   // :91-94
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_refind_new(mm->flags, (int)mm->queue.size());
    }
    if (want) {
        if (int rc = ptam_rmap_refind_queue(mm->map, mm->finder, &mm->opts.refind, PTAM_MAP_REFIND_NEW_POINTS, &mm->queue_nonempty, &res->refind_new))
            return rc;
        res->stages |= PTAM_MM_STAGE_REFIND_NEW;
    }

    MM_CHECK_RESET;   // :96-99
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_bundle_all(mm->flags, (int)mm->queue.size());
    }
    if (want) {
        if (int rc = mm_bundle(mm, false, &res->all, &res->all_outliers, &changed)) return rc;
        res->stages |= PTAM_MM_STAGE_BUNDLE_ALL;
    }

    MM_CHECK_RESET;   // :101-104
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_refind_failure(mm->flags, (int)mm->queue.size(), mm->opts.failure_seed, mm->opts.failure_period, &mm->draws);
    }
    if (want) {
        if (int rc = ptam_rmap_refind_queue(mm->map, mm->finder, &mm->opts.refind, PTAM_MAP_REFIND_FAILURE_QUEUE, nullptr, &res->refind_failure))
            return rc;
        res->stages |= PTAM_MM_STAGE_REFIND_FAILURE;
    }

    MM_CHECK_RESET;   // :106-107, behind the tracked frames' counts
    std::vector<MmNote> notes;
    {
        std::lock_guard<std::mutex> g(mm->mu);
        notes.swap(mm->notes);
    }
    if (!notes.empty()) {
        std::vector<ptam_frame_report*> reps;
        for (const MmNote& n : notes) reps.push_back(n.report);
        const int rc = ptam_rmap_note_reports(mm->map, (int)reps.size(), reps.data(), &res->notes);
        {
            std::lock_guard<std::mutex> g(mm->mu);
            for (const MmNote& n : notes) mm->released.push_back(n.tag);
        }
        if (rc) return rc;
        res->stages |= PTAM_MM_STAGE_NOTES;
    }
    if (int rc = ptam_rmap_handle_bad_points(mm->map, &res->bad_points, nullptr, nullptr)) return rc;
    res->stages |= PTAM_MM_STAGE_BAD_POINTS;
    changed = changed || res->bad_points.n_removed > 0;

    MM_CHECK_RESET;   // :109-112
    MmKeyFrame k;
    {
        std::lock_guard<std::mutex> g(mm->mu);
        want = mm_want_add_keyframe((int)mm->queue.size());
        if (want) {
            k = mm->queue.front();
            mm->queue.pop_front();
            mm->queue_nonempty = mm->queue.empty() ? 0 : 1;
        }
    }
    if (want) {
        int rc = PTAM_OK;
        if (!k.kf->rest_made) rc = ptam_make_keyframe_rest(mm->map->ctx, const_cast<ptam_kf*>(k.kf));   // :500
        if (!rc) {
            ptam_rmap_insert_opts io = mm->opts.insert;
            io.epipolar.depth_mean = k.depth_mean;
            io.epipolar.depth_sigma = k.depth_sigma;
            rc = ptam_rmap_insert_keyframe_report(mm->map, mm->finder, k.kf, k.pose, k.fixed, k.report, &io, &res->insert, &res->insert_rows,
                                                  &res->insert_gone);
        }
        std::lock_guard<std::mutex> g(mm->mu);
        mm->released.push_back(k.tag);
        if (rc) return rc;
        mm_keyframe_added(mm->flags);
        res->stages |= PTAM_MM_STAGE_ADD_KEYFRAME;
        changed = true;
    }
#undef MM_CHECK_RESET
    if (mm->snapshot && changed) {
        if (int rc = ptam_rmap_publish(mm->map, mm->snapshot, &res->publish)) return rc;
        res->stages |= PTAM_MM_STAGE_PUBLISH;
    }
    return finish(PTAM_MM_RAN);
}

// the trailer — flags, queue and draws as the stages left them — is filled on an error too
int ptam_mapmaker_step(ptam_mapmaker* mm, ptam_mapmaker_step_result* res) {
    ARG_TRY(mm && res);
    std::memset(res, 0, sizeof *res);
    const int rc = mm_step_stages(mm, res);
    std::lock_guard<std::mutex> g(mm->mu);
    res->converged_recent = mm->flags.converged_recent;
    res->converged_full = mm->flags.converged_full;
    res->queue_size = (int)mm->queue.size();
    res->draws = mm->draws;
    return rc;
}

}   // extern "C"
