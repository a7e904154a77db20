// camera_tracker.hip — ptam_camera_tracker (ptam_hip.h): one frame of Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) with
// its hand-over to the mapmaker, as one call.  Host code over the library's own entries: the device work is
// ptam_track_frames_report_batch (trackmap.hip) and ptam_kf_copy (keyframe.hip); what is decided here is decided in tracker_plan.h
// (the add / note rule, the pools), which a plain C++ compiler checks on the CPU (tools/tracking/tracker_plan_check.cc).
// With ptam_camera_tracker_enable_session the handle also runs Tracker::TrackForInitialMap (:311-347): the stage rule is
// tp_session_action (tools/tracking/session_plan_check.cc), the trail-stage cameras of a call go through ptam_trails_advance_batch,
// the map is made by the mapmaker's step (ptam_mapmaker_request_init), and the tracking cameras go through the same body as
// ptam_camera_tracker_track_frames (ct_track_frames).
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "tracker_plan.h"

struct ptam_camera_tracker {
    ptam_ctx* ctx;
    ptam_camera_tracker_opts o;
    ptam_map_snapshot* snapshot;     // borrowed
    ptam_mapmaker* mapmaker;         // borrowed
    ptam_tracker* tracker;
    ptam_kf* current;
    ptam_rotation_estimator* estimator;   // null: use_rotation_estimator == 0
    ptam_sbi_bank* bank;
    ptam_sbi* scratch;
    ptam_track_state state;
    std::vector<ptam_frame_report*> reports;
    std::vector<ptam_kf*> clones;
    TpPool pool;
    int last_report;                 // index, -1 before the first frame
    // the session (ptam_camera_tracker_enable_session); without it the handle is COMPLETE with a map, for ever
    bool session;
    ptam_camera_session_opts so;
    int stage;                       // mnInitialStage
    ptam_trails* trails;             // mlTrails and mPreviousFrameKF
    ptam_kf* first_kf;               // mFirstKF
    bool init_pending, init_read;    // a request is with the mapmaker | init_result holds a request's outcome
    int64_t init_tag;
    ptam_rmap_init_result init_result;
    std::vector<ptam_trail> matches; // vMatches (:338-340): room for max_initial_trails
};

static void ct_free(ptam_camera_tracker* h) {
    for (ptam_frame_report* r : h->reports) ptam_frame_report_destroy(r);
    for (ptam_kf* k : h->clones) ptam_kf_destroy(k);
    if (h->scratch) ptam_sbi_destroy(h->scratch);
    if (h->bank) ptam_sbi_bank_destroy(h->bank);
    if (h->estimator) ptam_rotation_estimator_destroy(h->estimator);
    if (h->current) ptam_kf_destroy(h->current);
    if (h->tracker) ptam_tracker_destroy(h->tracker);
    if (h->trails) ptam_trails_destroy(h->trails);
    if (h->first_kf) ptam_kf_destroy(h->first_kf);
    delete h;
}

extern "C" {

int ptam_camera_tracker_opts_default(ptam_camera_tracker_opts* o) {
    ARG_TRY(o);
    std::memset(o, 0, sizeof *o);
    o->max_points = 8192;
    o->width = 640, o->height = 480;
    o->max_keyframes = 64;
    ptam_trackmap_opts_default(&o->trackmap);
    ptam_track_state_opts_default(&o->state);
    o->use_rotation_estimator = 1;   // Tracker.UseRotationEstimator
    o->rotation_blur = 0.75;         // Tracker.RotationEstimatorBlur
    o->keyframe_gap = 20;            // src/Tracker.cc:148
    o->max_queue = 3;                // :149
    o->reports = 8;
    o->keyframes = 32;
    return PTAM_OK;
}

int ptam_camera_tracker_create(ptam_ctx* ctx, const ptam_camera_tracker_opts* opts, ptam_map_snapshot* snapshot, ptam_mapmaker* mapmaker,
                               ptam_camera_tracker** out) {
    ARG_TRY(ctx && snapshot && mapmaker && out);
    ptam_camera_tracker_opts o;
    ptam_camera_tracker_opts_default(&o);
    if (opts) o = *opts;
    ARG_TRY(o.max_points >= 1 && o.width >= 8 && o.height >= 8 && o.max_keyframes >= 1);
    ARG_TRY(o.keyframe_gap >= 0 && o.max_queue >= 1 && o.reports >= 1 && o.reports <= 4096 && o.keyframes >= 1 && o.keyframes <= 4096);
    ARG_TRY(o.rotation_blur > 0.0);
    ptam_camera_tracker* h = new ptam_camera_tracker();
    h->ctx = ctx, h->o = o, h->snapshot = snapshot, h->mapmaker = mapmaker;
    h->tracker = nullptr, h->current = nullptr, h->estimator = nullptr, h->bank = nullptr, h->scratch = nullptr;
    h->pool = TpPool(o.reports, o.keyframes);
    h->last_report = -1;
    h->session = false, h->stage = TP_TRAILS_COMPLETE, h->trails = nullptr, h->first_kf = nullptr;
    h->init_pending = h->init_read = false, h->init_tag = 0;
    const double identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    ptam_track_state_reset(&h->state, identity);
    int rc = ptam_tracker_create(ctx, o.max_points, &h->tracker);
    if (!rc) rc = ptam_kf_create(ctx, o.width, o.height, &h->current);
    if (!rc && o.use_rotation_estimator) rc = ptam_rotation_estimator_create(ctx, o.width, o.height, o.rotation_blur, &h->estimator);
    if (!rc) rc = ptam_sbi_bank_create(ctx, o.width, o.height, o.max_keyframes, &h->bank);
    if (!rc) rc = ptam_sbi_create(ctx, o.width, o.height, &h->scratch);
    for (int i = 0; i < o.reports && !rc; i++) {
        ptam_frame_report* r = nullptr;
        rc = ptam_frame_report_create(ctx, o.max_points, &r);
        if (!rc) h->reports.push_back(r);
    }
    for (int i = 0; i < o.keyframes && !rc; i++) {
        ptam_kf* k = nullptr;
        rc = ptam_kf_create(ctx, o.width, o.height, &k);
        if (!rc) h->clones.push_back(k);
    }
    if (rc) {   // (the failing call's error text stands)
        const std::string e = ptam_last_error();
        ct_free(h);
        ptam_set_error("%s", e.c_str());
        return rc;
    }
    *out = h;
    return PTAM_OK;
}

int ptam_camera_tracker_destroy(ptam_camera_tracker* h) {
    if (!h) return PTAM_OK;
    ct_free(h);
    return PTAM_OK;
}

int ptam_camera_tracker_reset(ptam_camera_tracker* h, const double pose12[12]) {
    ARG_TRY(h && pose12);
    ptam_track_state_reset(&h->state, pose12);
    if (h->estimator)
        if (int rc = ptam_rotation_estimator_reset(h->estimator)) return rc;
    if (int rc = ptam_sbi_bank_clear(h->bank)) return rc;
    h->pool.reset();
    h->last_report = -1;
    h->init_pending = false;   // (its clones are free again: the request, if it is still pending, is the caller's to drop — request_reset)
    return PTAM_OK;
}

int ptam_camera_tracker_state(const ptam_camera_tracker* h, ptam_track_state* out) {
    ARG_TRY(h && out);
    *out = h->state;
    return PTAM_OK;
}
ptam_tracker* ptam_camera_tracker_tracker(ptam_camera_tracker* h) { return h ? h->tracker : nullptr; }
ptam_kf* ptam_camera_tracker_current_keyframe(ptam_camera_tracker* h) { return h ? h->current : nullptr; }
ptam_frame_report* ptam_camera_tracker_last_report(ptam_camera_tracker* h) {
    return h && h->last_report >= 0 ? h->reports[(size_t)h->last_report] : nullptr;
}
int ptam_camera_tracker_pool(const ptam_camera_tracker* h, int32_t* free_reports, int32_t* free_keyframes) {
    ARG_TRY(h);
    if (free_reports) *free_reports = h->pool.count(h->pool.report_state, TpPool::FREE);
    if (free_keyframes) *free_keyframes = h->pool.count(h->pool.clone_state, TpPool::FREE);
    return PTAM_OK;
}

}   // extern "C"

// Tracker::TrackFrame's branch for a good map (:127-176) for nb handles: the body of ptam_camera_tracker_track_frames, and of the
// tracking subset of ptam_camera_tracker_session_frames
static int ct_track_frames(int nb, ptam_camera_tracker* const* hs, const uint8_t* const* d_frames, ptam_camera_track_result* results) {
    ARG_TRY(nb >= 1 && nb <= 4096 && hs && d_frames && results);
    for (int i = 0; i < nb; i++) {
        ARG_TRY(hs[i] && d_frames[i]);
        for (int j = 0; j < i; j++) ARG_TRY(hs[j] != hs[i]);
        // (one chain, one set of TrackMap and state options: the batch entries take them once)
        ARG_TRY(std::memcmp(&hs[i]->o.trackmap, &hs[0]->o.trackmap, sizeof hs[0]->o.trackmap) == 0);
        ARG_TRY(std::memcmp(&hs[i]->o.state, &hs[0]->o.state, sizeof hs[0]->o.state) == 0);
    }
    const size_t n = (size_t)nb;
    // ---- (a) what the mapmakers have released, once per mapmaker, dealt out to the handles of the call
    std::map<ptam_mapmaker*, std::vector<int64_t>> released;
    for (int i = 0; i < nb; i++) released[hs[i]->mapmaker];
    for (auto& mm : released) {
        int64_t tags[64];
        int32_t got = 0;
        do {
            if (int rc = ptam_mapmaker_released(mm.first, 64, tags, &got)) return rc;
            mm.second.insert(mm.second.end(), tags, tags + got);
        } while (got == 64);
    }
    for (int i = 0; i < nb; i++)
        for (int64_t tag : released[hs[i]->mapmaker]) hs[i]->pool.release(tag);
    for (int i = 0; i < nb; i++) {
        const ptam_camera_tracker& h = *hs[i];
        if (h.pool.free_report() < 0) {
            ptam_set_error("ptam_camera_tracker_track_frames: camera %d has no free report (%d are with the mapmaker)", i, (int)h.reports.size());
            return PTAM_E_STATE;
        }
        if (tp_may_add(h.state.lost_frames, h.state.frame, h.state.last_keyframe_dropped, h.o.keyframe_gap) && h.pool.free_clone() < 0) {
            ptam_set_error("ptam_camera_tracker_track_frames: camera %d has no free keyframe clone (%d are with the map)", i, (int)h.clones.size());
            return PTAM_E_STATE;
        }
    }
    // ---- (b) the map and its keyframes
    std::vector<ptam_map_take_result> takes(n);
    std::vector<ptam_keyframes_take_result> kf_takes(n);
    for (int i = 0; i < nb; i++) {
        ptam_camera_tracker& h = *hs[i];
        ptam_map_snapshot_info_t si = {};
        if (int rc = ptam_map_snapshot_info(h.snapshot, &si)) return rc;
        if (si.generation == 0 || si.n_points == 0) {
            ptam_set_error("ptam_camera_tracker_track_frames: no map (camera %d: %s)", i, si.generation == 0 ? "nothing was published" : "the map has no point");
            return PTAM_E_STATE;
        }
        if (int rc = ptam_tracker_take_map(h.tracker, h.snapshot, &takes[(size_t)i])) return rc;
        if (int rc = ptam_sbi_bank_take_keyframes(h.bank, h.snapshot, &kf_takes[(size_t)i])) return rc;
    }
    // ---- (c) the chain
    std::vector<ptam_tracker*> ts(n);
    std::vector<ptam_kf*> curs(n);
    std::vector<ptam_rotation_estimator*> ests(n);
    std::vector<ptam_sbi_bank*> banks(n);
    std::vector<ptam_sbi*> scratch(n);
    std::vector<ptam_track_state> states(n);
    std::vector<ptam_frame_report*> reps(n);
    std::vector<int> rep_at(n);
    std::vector<int64_t> tags(n);
    std::vector<uint64_t> seeds(n);
    std::vector<ptam_trackmap_result> outs(n);
    std::vector<ptam_track_frame_state_info> infos(n);
    std::vector<ptam_track_report_info> rinfos(n);
    for (int i = 0; i < nb; i++) {
        ptam_camera_tracker& h = *hs[i];
        const size_t k = (size_t)i;
        ts[k] = h.tracker, curs[k] = h.current, ests[k] = h.estimator, banks[k] = h.bank, scratch[k] = h.scratch;
        states[k] = h.state;
        rep_at[k] = h.pool.free_report();          // (held only when the chain has delivered)
        reps[k] = h.reports[(size_t)rep_at[k]];
        tags[k] = h.o.tag_base + h.state.frame;
        seeds[k] = h.o.shuffle_seed;
    }
    // (one set of options serves a call: checked above)
    const int rc_chain = ptam_track_frames_report_batch(nb, ts.data(), curs.data(), d_frames, states.data(), ests.data(), banks.data(), scratch.data(),
                                                        &hs[0]->o.trackmap, &hs[0]->o.state, outs.data(), infos.data(), reps.data(), tags.data(),
                                                        seeds.data(), rinfos.data());
    if (rc_chain) return rc_chain;   // (the reports hold max_points records: none is too small for its frame)
    // ---- (d) the hand-over, (e) the results
    int rc_late = PTAM_OK;
    std::string late;
    for (int i = 0; i < nb; i++) {
        ptam_camera_tracker& h = *hs[i];
        const size_t k = (size_t)i;
        h.state = states[k];
        h.pool.report_state[(size_t)rep_at[k]] = TpPool::HELD;
        h.last_report = rep_at[k];
        ptam_camera_track_result& r = results[i];
        std::memset(&r, 0, sizeof r);
        r.track = outs[k], r.info = infos[k], r.report = rinfos[k].report, r.report_in_chain = rinfos[k].report_in_chain;
        r.map_take = takes[k], r.keyframes_take = kf_takes[k], r.tag = tags[k];
        int32_t queue = 0;
        int rc = ptam_mapmaker_queue_size(h.mapmaker, &queue);
        r.queue_size = queue;
        const int what = rc ? TP_NEITHER
                            : tp_decide(infos[k].branch, h.state.quality, h.state.frame, h.state.last_keyframe_dropped, h.o.keyframe_gap, queue,
                                        h.o.max_queue, rinfos[k].report.n_records);
        if (what == TP_ADD) {
            const int c = h.pool.free_clone();   // (there is one: asked before the chain)
            ptam_kf* clone = h.clones[(size_t)c];
            rc = ptam_kf_copy(h.ctx, h.current, clone);
            if (!rc) rc = ptam_ctx_sync(h.ctx);   // the mapmaker's thread reads the clone on its own queue
            if (!rc)
                rc = ptam_mapmaker_add_keyframe(h.mapmaker, clone, outs[k].pose, 0, reps[k], h.state.model.scene_depth_mean,
                                                h.state.model.scene_depth_sigma, tags[k]);
            if (!rc) {
                h.pool.hand_over(rep_at[k], c, tags[k]);
                h.state.last_keyframe_dropped = h.state.frame;   // :165
                r.added_keyframe = 1;
            }
        } else if (what == TP_NOTE) {
            rc = ptam_mapmaker_note_frame(h.mapmaker, reps[k], tags[k]);
            if (!rc) {
                h.pool.hand_over(rep_at[k], -1, tags[k]);
                r.noted_frame = 1;
            }
        }
        if (!r.added_keyframe && !r.noted_frame) h.pool.return_report(rep_at[k]);
        if (rc && !rc_late) rc_late = rc, late = ptam_last_error();
    }
    if (rc_late) ptam_set_error("%s", late.c_str());
    return rc_late;
}

// the tracker's side of Tracker::Reset (:49-65)
static int ct_restart(ptam_camera_tracker* h) {
    const double identity[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    if (int rc = ptam_camera_tracker_reset(h, identity)) return rc;
    if (h->session) h->stage = TP_TRAILS_NOT_STARTED;
    return PTAM_OK;
}

extern "C" {

int ptam_camera_tracker_track_frames(int nb, ptam_camera_tracker* const* hs, const uint8_t* const* d_frames, ptam_camera_track_result* results) {
    return ct_track_frames(nb, hs, d_frames, results);
}

int ptam_camera_session_opts_default(ptam_camera_session_opts* o) {
    ARG_TRY(o);
    std::memset(o, 0, sizeof *o);
    o->max_initial_trails = 1000;   // Tracker.MaxInitialTrails, src/Tracker.cc:360
    o->min_good_trails = 10;        // :329
    o->min_shi_tomasi = 70.0;       // Level::vCandidates' threshold, src/KeyFrame.cc:66-76
    return ptam_rmap_init_opts_default(&o->init);
}

int ptam_camera_tracker_enable_session(ptam_camera_tracker* h, const ptam_camera_session_opts* opts) {
    ARG_TRY(h);
    ptam_camera_session_opts so;
    if (int rc = ptam_camera_session_opts_default(&so)) return rc;
    if (opts) so = *opts;
    ARG_TRY(so.max_initial_trails >= 1 && so.min_good_trails >= 0);
    const int busy = (int)h->reports.size() - h->pool.count(h->pool.report_state, TpPool::FREE) + (int)h->clones.size() -
                     h->pool.count(h->pool.clone_state, TpPool::FREE);
    if (h->session || busy) {
        ptam_set_error("ptam_camera_tracker_enable_session: %s", h->session ? "the session is enabled already" : "a report or a clone is out");
        return PTAM_E_STATE;
    }
    ptam_trails* tr = nullptr;
    ptam_kf* first = nullptr;
    int rc = ptam_trails_create(h->ctx, so.max_initial_trails, &tr);
    if (!rc) rc = ptam_kf_create(h->ctx, h->o.width, h->o.height, &first);
    if (rc) {
        const std::string e = ptam_last_error();
        if (tr) ptam_trails_destroy(tr);
        ptam_set_error("%s", e.c_str());
        return rc;
    }
    h->trails = tr, h->first_kf = first, h->so = so;
    h->matches.assign((size_t)so.max_initial_trails, ptam_trail());
    h->session = true;
    return ct_restart(h);
}

int ptam_camera_tracker_restart(ptam_camera_tracker* h) {
    ARG_TRY(h);
    return ct_restart(h);
}

ptam_trails* ptam_camera_tracker_trails(ptam_camera_tracker* h) { return h ? h->trails : nullptr; }
int ptam_camera_tracker_init_result(const ptam_camera_tracker* h, ptam_rmap_init_result* out) {
    ARG_TRY(h && out);
    if (!h->init_read) {
        ptam_set_error("ptam_camera_tracker_init_result: no request's outcome has been read");
        return PTAM_E_STATE;
    }
    *out = h->init_result;
    return PTAM_OK;
}
int ptam_camera_tracker_stage(const ptam_camera_tracker* h, int32_t* stage) {
    ARG_TRY(h && stage);
    *stage = h->stage;
    return PTAM_OK;
}

int ptam_camera_tracker_session_frames(int nb, ptam_camera_tracker* const* hs, const uint8_t* const* d_frames, const uint8_t* pokes,
                                       ptam_camera_track_result* results, ptam_camera_session_result* session) {
    ARG_TRY(nb >= 1 && nb <= 4096 && hs && d_frames && results && session);
    for (int i = 0; i < nb; i++) {
        ARG_TRY(hs[i] && d_frames[i]);
        for (int j = 0; j < i; j++) ARG_TRY(hs[j] != hs[i]);
    }
    const size_t n = (size_t)nb;
    // ---- what each camera does, as far as it is known before its trails have advanced: no device is touched, nothing changes
    std::vector<int> action(n);
    std::vector<ptam_rmap_init_result> polled(n);
    std::vector<int> advancing, tracking;
    for (int i = 0; i < nb; i++) {
        const ptam_camera_tracker& h = *hs[i];
        const bool poke = pokes && pokes[i];
        int32_t init_state = MM_INIT_NONE;
        if (h.stage == TP_TRAILS_COMPLETE && h.init_pending)
            if (int rc = ptam_mapmaker_init_poll(h.mapmaker, &init_state, &polled[(size_t)i])) return rc;
        if (h.stage == TP_TRAILS_COMPLETE && h.init_pending && init_state == MM_INIT_NONE) init_state = MM_INIT_PENDING;   // (a mapmaker that knows of no request: wait)
        // (STARTED: the good count is not known yet; min_good stands in for "enough", the rule is asked again behind the advance)
        action[(size_t)i] = tp_session_action(h.stage, poke, h.so.min_good_trails, h.so.min_good_trails, init_state, polled[(size_t)i].status);
        if (h.stage == TP_TRAILS_STARTED) {
            advancing.push_back(i);
            if (poke && h.pool.count(h.pool.clone_state, TpPool::FREE) < 2) {
                ptam_set_error("ptam_camera_tracker_session_frames: camera %d has fewer than two free keyframe clones for the first map", i);
                return PTAM_E_STATE;
            }
        }
        if (action[(size_t)i] == TP_S_TRACK || action[(size_t)i] == TP_S_BEGIN) tracking.push_back(i);
    }
    std::memset(results, 0, n * sizeof *results);
    std::memset(session, 0, n * sizeof *session);
    for (int i = 0; i < nb; i++) session[i].stage_before = session[i].stage_after = hs[i]->stage;
    // ---- the trail stage.  STARTED: one chain for all of them; its refusals come before anything is enqueued
    if (!advancing.empty()) {
        const size_t na = advancing.size();
        std::vector<ptam_trails*> trs(na);
        std::vector<ptam_kf*> curs(na);
        std::vector<const uint8_t*> frs(na);
        std::vector<int32_t> good(na), alive(na);
        for (size_t k = 0; k < na; k++) trs[k] = hs[advancing[k]]->trails, curs[k] = hs[advancing[k]]->current, frs[k] = d_frames[advancing[k]];
        if (na == 1) {   // (one camera: the per-camera calls are the shorter path, 49.7 against 68.1 us a frame — docs/LOG_tracker.md)
            int g = 0, a = 0;
            if (int rc = ptam_make_keyframe_lite_dev(hs[advancing[0]]->ctx, curs[0], frs[0])) return rc;
            if (int rc = ptam_trails_advance(trs[0], curs[0], &g, &a)) return rc;
            good[0] = g, alive[0] = a;
        } else if (int rc = ptam_trails_advance_batch((int)na, trs.data(), curs.data(), frs.data(), good.data(), alive.data()))
            return rc;
        for (size_t k = 0; k < na; k++) {
            const int i = advancing[k];
            ptam_camera_tracker& h = *hs[i];
            ptam_camera_session_result& s = session[i];
            const bool poke = pokes && pokes[i];
            h.state.frame++;   // :111
            s.n_good = good[k], s.n_alive = alive[k];
            const int what = tp_session_action(h.stage, poke, good[k], h.so.min_good_trails, MM_INIT_NONE, 0);
            action[(size_t)i] = what;
            s.poked = tp_session_consumes_poke(what, poke);
            if (what == TP_S_RESET) {   // :329-332
                if (int rc = ct_restart(&h)) return rc;
                s.trail_reset = 1;
            } else if (what == TP_S_REQUEST) {   // :335-343
                int n_matches = 0;
                int rc = ptam_trails_read(h.trails, h.matches.data(), (int)h.matches.size(), &n_matches);
                const int c0 = h.pool.free_clone();
                int c1 = c0 + 1;   // (there are two: asked at the entry)
                while (h.pool.clone_state[(size_t)c1] != TpPool::FREE) c1++;
                const int64_t tag = h.o.tag_base + h.state.frame - 1;   // the state's frame at entry
                if (!rc) rc = ptam_kf_copy(h.ctx, h.first_kf, h.clones[(size_t)c0]);
                if (!rc) rc = ptam_kf_copy(h.ctx, h.current, h.clones[(size_t)c1]);
                if (!rc) rc = ptam_ctx_sync(h.ctx);   // the mapmaker's thread reads the clones on its own queue
                if (!rc) rc = ptam_mapmaker_request_init(h.mapmaker, h.clones[(size_t)c0], h.clones[(size_t)c1], n_matches, h.matches.data(), &h.so.init, tag);
                if (rc) return rc;   // (the trails have advanced and the stage stays STARTED: the next poke asks again)
                h.pool.clones_out(c0, c1, tag);
                h.stage = TP_TRAILS_COMPLETE;
                h.init_pending = true, h.init_tag = tag;
                s.init_requested = 1, s.init_tag = tag, s.n_trails = n_matches;
            }
            s.stage_after = h.stage;
        }
    }
    // NOT_STARTED, and COMPLETE while the request is pending or has failed
    for (int i = 0; i < nb; i++) {
        ptam_camera_tracker& h = *hs[i];
        ptam_camera_session_result& s = session[i];
        const int what = action[(size_t)i];
        const bool poke = pokes && pokes[i];
        if (s.stage_before == TP_TRAILS_STARTED || what == TP_S_TRACK || what == TP_S_BEGIN) continue;   // (done above | below)
        if (what == TP_S_INIT_FAILED) {   // the outcome is read: the tracker's side of Reset(), which frees the request's two clones
            if (int rc = ct_restart(&h)) return rc;
            h.init_result = polled[(size_t)i], h.init_read = true;
            s.init_done = 1, s.init_status = polled[(size_t)i].status;
            s.stage_after = h.stage;
            continue;   // (Reset() ends TrackFrame's work on this frame as it does at :329-332)
        }
        if (int rc = ptam_make_keyframe_lite_dev(h.ctx, h.current, d_frames[i])) return rc;   // :92
        h.state.frame++;                                                                        // :111
        if (what == TP_S_START) {   // :315-320, :352-370
            int n_trails = 0;
            int rc = ptam_make_keyframe_rest(h.ctx, h.current);
            if (!rc) rc = ptam_kf_copy(h.ctx, h.current, h.first_kf);
            if (!rc) rc = ptam_trails_start(h.trails, h.current, h.so.min_shi_tomasi, h.so.max_initial_trails, &n_trails);
            if (rc) return rc;
            h.stage = TP_TRAILS_STARTED;
            s.n_trails = n_trails;
        }
        s.poked = tp_session_consumes_poke(what, poke);
        s.stage_after = h.stage;
    }
    // ---- the tracking subset: a camera whose map has just been made starts from the tracker's pose (:341)
    if (tracking.empty()) return PTAM_OK;
    const size_t nt = tracking.size();
    std::vector<ptam_camera_tracker*> ths(nt);
    std::vector<const uint8_t*> tfr(nt);
    std::vector<ptam_camera_track_result> tres(nt);
    std::vector<ptam_track_state> before(nt);
    for (size_t k = 0; k < nt; k++) {
        const int i = tracking[k];
        ptam_camera_tracker& h = *hs[i];
        ths[k] = &h, tfr[k] = d_frames[i];
        before[k] = h.state;
        if (action[(size_t)i] != TP_S_BEGIN) continue;
        const int frame = h.state.frame, last = h.state.last_keyframe_dropped;
        ptam_track_state_reset(&h.state, polled[(size_t)i].tracker_pose);
        h.state.frame = frame, h.state.last_keyframe_dropped = last;
        if (h.estimator)   // (it has seen no frame since the handle's last reset: resetting it again changes nothing if the call is refused)
            if (int rc = ptam_rotation_estimator_reset(h.estimator)) return rc;
    }
    const int rc = ct_track_frames((int)nt, ths.data(), tfr.data(), tres.data());
    // A refusal leaves every state where it was; a failure of the hand-over comes behind frames that were delivered.  A camera whose
    // frame was delivered has begun: its request is read.  One whose call was refused keeps its request pending and its old state.
    for (size_t k = 0; k < nt; k++) {
        const int i = tracking[k];
        ptam_camera_tracker& h = *hs[i];
        const bool delivered = h.state.frame != before[k].frame;
        if (delivered) results[i] = tres[k], session[i].tracked = 1;
        if (action[(size_t)i] != TP_S_BEGIN) continue;
        if (!delivered) {
            h.state = before[k];
            continue;
        }
        h.init_pending = false;
        h.init_result = polled[(size_t)i], h.init_read = true;
        session[i].init_done = 1, session[i].init_status = polled[(size_t)i].status;
    }
    return rc;
}

}   // extern "C"
