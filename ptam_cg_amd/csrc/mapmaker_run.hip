// mapmaker_run.hip — ptam_mapmaker (ptam_hip.h): one iteration of MapMaker::run() (src/MapMaker.cc:57-114) as one call on a resident
// map.  Host code only: every stage is a call that exists (ptam_rmap_bundle_adjust_routed, ptam_rmap_refind_queue,
// ptam_rmap_note_reports, ptam_rmap_handle_bad_points, ptam_rmap_insert_keyframe_report, ptam_rmap_publish, ptam_rmap_clear), and
// every decision is a function of mapmaker_plan.h.  What is the handle's own: the keyframe queue, the pending reports and the
// released tags under one mutex; the flags, written by the step and by AddKeyFrame under that mutex; the two bytes the device calls
// poll from the host between their launches (the bundle's abort, the re-find's stop).
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
};

static int mm_queue_size(ptam_mapmaker* mm) {
    std::lock_guard<std::mutex> g(mm->mu);
    return (int)mm->queue.size();
}

// MapMaker::Reset (:37-51)
static int mm_do_reset(ptam_mapmaker* mm) {
    const int rc = ptam_rmap_clear(mm->map);
    std::lock_guard<std::mutex> g(mm->mu);
    for (const MmKeyFrame& k : mm->queue) mm->released.push_back(k.tag);
    for (const MmNote& n : mm->notes) mm->released.push_back(n.tag);
    mm->queue.clear();
    mm->notes.clear();
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
    if (mm->map->n[RM_N_KF] == 0) return finish(PTAM_MM_IDLE);   // :79
    bool changed = false;   // what a tracker has to see: an accepted bundle, removed points, a new keyframe
    bool want;

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
