// session_demo.cc — a session from the first frame through ptam_shim.hpp: ptam::Tracker with EnableSession() and PokeTracker(), and
// ptam::MapMaker over an EMPTY resident map.  The tracker counts frames, starts its trails at the first poke, hands the two keyframes
// and the matches to the mapmaker at the second (MapMaker::RequestInit inside Tracker::TrackFrame), and tracks from the frame after the
// step that made the map (tests/test_gpu_session_shim.py builds and runs it).
//   session_demo <in> <out>            one thread: the tracker and a second one that is poked once and stays in its trail stage, both
//                                      through Tracker::TrackFrames (a mixed call), then MapMaker::Step, frame after frame; then the
//                                      pieces on their own — TrailTracker::AdvanceBatch for two cameras, MapMaker::RequestInit / InitPoll
//                                      on a second map — and Tracker::Restart.  <out> is compared byte for byte with the same
//                                      sequence through host.*
//   session_demo <in> <out> threads    a tracker thread beside MapMaker::Run(); after its second poke the tracker waits for
//                                      MapMaker::InitPoll() to say DONE, as the reference's tracker waits inside InitFromStereo
//   in:  int32 width, height, n_frames; n_frames images; n_frames poke bytes
//   out: per frame the ptam_camera_session_result, the ptam_trackmap_result, 7 int32 (branch, records, entries, outliers, added, noted,
//        queue), the tag, and (one thread) the second tracker's ptam_camera_session_result and the step's status and stages; (one
//        thread) the pieces: per advance two good and two alive counts, both trail lists, 7 int32 of the request (state before, step
//        status and stages, state after, init status, points, keyframes) and the released tag; the second tracker's stage and frame
//        count after Restart; then the ptam_track_state, the two pool counts, the trails made by the last start, the map's keyframe
//        poses and its measurement table
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ptam_shim.hpp"

template <class T>
static void put(FILE* f, const T& v) {
    std::fwrite(&v, sizeof(T), 1, f);
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        std::fprintf(stderr, "usage: session_demo <frames in> <result out> [threads]\n");
        return 2;
    }
    const bool threads = argc == 4;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[3];
    if (!f || std::fread(h, 4, 3, f) != 3) return 3;
    const int width = h[0], height = h[1], n_frames = h[2];
    const size_t px = (size_t)width * height;
    std::vector<uint8_t> images(px * (size_t)n_frames), pokes((size_t)n_frames);
    if (std::fread(images.data(), 1, images.size(), f) != images.size() || std::fread(pokes.data(), 1, pokes.size(), f) != pokes.size()) return 3;
    std::fclose(f);
    const ptam::Vec<5> cam{1.0803, 1.43987, 0.519983, 0.548655, 0.244943};
    int rc = 0;
    try {
        ptam::Context cm(cam, {width, height}), ct(cam, {width, height});   // the mapmaker's and the tracker's
        const int cap = 8192;
        ptam::ResidentMap map(cm);                                            // empty: the session makes the map
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        snapshot.EnableKeyFrames(16);
        ptam_mapmaker_opts mo = ptam::MapMaker::DefaultOpts();
        mo.ba.deterministic = 1;
        ptam::MapMaker mm(map, finder, &snapshot, &mo);

        ptam_camera_tracker_opts to = ptam::Tracker::DefaultOpts(ct);
        to.max_points = cap, to.max_keyframes = 16, to.shuffle_seed = 7, to.tag_base = 1000, to.keyframe_gap = 1, to.reports = 8, to.keyframes = 8;
        ptam::Tracker tracker(ct, snapshot, mm, &to);
        ptam_camera_session_opts so;
        ptam::check(ptam_camera_session_opts_default(&so), "ptam_camera_session_opts_default");
        so.init.max_bundles = 20, so.init.homography.seed = 3, so.init.ba.deterministic = 1, so.init.plane.seed = 5;
        tracker.EnableSession(&so);
        ptam::Context ct2(cam, {width, height});
        ptam::Tracker second(ct2, snapshot, mm, &to);
        second.EnableSession(&so);
        bool second_poked = false;

        std::vector<void*> d_frames((size_t)n_frames, nullptr);
        for (int k = 0; k < n_frames; k++) {
            ptam::check(ptam_dev_alloc(ct.handle(), px, &d_frames[(size_t)k]), "ptam_dev_alloc");
            ptam::check(ptam_dev_upload(ct.handle(), d_frames[(size_t)k], images.data() + px * (size_t)k, px), "ptam_dev_upload");
        }
        FILE* out = std::fopen(argv[2], "wb");
        if (!out) return 3;
        int tracked = 0, last_trails = 0, last_branch = -1;
        const auto frame = [&](int k) {
            if (pokes[(size_t)k]) tracker.PokeTracker();
            const uint8_t* d = (const uint8_t*)d_frames[(size_t)k];
            ptam_camera_track_result r;
            if (threads)
                r = tracker.TrackFrame(d);
            else {   // (frames in device memory are the device's: the second tracker's context reads them as well)
                if (pokes[(size_t)k] && !second_poked) second.PokeTracker(), second_poked = true;
                r = ptam::Tracker::TrackFrames({&tracker, &second}, {d, d})[0];
            }
            const ptam_camera_session_result s = tracker.Session();
            put(out, s);
            put(out, r.track);
            const int32_t words[7] = {r.info.branch, r.report.n_records, r.report.n_entries, r.report.n_outliers, r.added_keyframe, r.noted_frame, r.queue_size};
            put(out, words);
            put(out, r.tag);
            if (s.stage_after == PTAM_TRAIL_TRACKING_STARTED && s.stage_before == PTAM_TRAIL_TRACKING_NOT_STARTED) last_trails = s.n_trails;
            if (s.tracked) tracked++, last_branch = r.info.branch;
            return s;
        };
        if (!threads) {
            for (int k = 0; k < n_frames; k++) {
                frame(k);
                put(out, second.Session());
                const ptam_mapmaker_step_result st = mm.Step();
                put(out, st.status);
                put(out, st.stages);
            }
            // ---- the pieces: two trail trackers in contexts of their own through one chain, then a request on a second, empty map
            ptam::Context ca(cam, {width, height}), cb(cam, {width, height});
            ptam::KeyFrame fa(ca), fb(cb), ka(ca), kb(cb);
            fa.MakeKeyFrame_Lite(images.data(), width), fb.MakeKeyFrame_Lite(images.data(), width);
            fa.MakeKeyFrame_Rest(), fb.MakeKeyFrame_Rest();
            ptam::TrailTracker ta(ca), tb(cb, 64);
            ta.Start(fa), tb.Start(fb);
            for (int k = 2; k <= 6 && k < n_frames; k++) {
                const std::vector<int> good = ptam::TrailTracker::AdvanceBatch({&ta, &tb}, {&ka, &kb}, {(const uint8_t*)d_frames[(size_t)k], (const uint8_t*)d_frames[(size_t)k]});
                const int32_t counts[4] = {good[0], good[1], ta.Alive(), tb.Alive()};
                put(out, counts);
            }
            const std::vector<ptam_trail> la = ta.Trails(), lb = tb.Trails();
            std::fwrite(la.data(), sizeof(ptam_trail), la.size(), out);
            std::fwrite(lb.data(), sizeof(ptam_trail), lb.size(), out);
            ptam::KeyFrame c0(fa), c1(ka);   // the clones the map will name
            ptam::check(ptam_ctx_sync(ca.handle()), "ptam_ctx_sync");
            ptam::ResidentMap map2(cm);
            ptam::ReFinder finder2(cm);
            ptam::MapMaker mm2(map2, finder2, nullptr, &mo);
            mm2.RequestInit(c0, c1, la, &so.init, 5);
            const int before = mm2.InitPoll();
            const ptam_mapmaker_step_result st2 = mm2.Step();
            ptam_rmap_init_result res;
            const int after = mm2.InitPoll(&res);
            const int32_t req[7] = {before, st2.status, st2.stages, after, res.status, res.counts.n_points, res.counts.n_kf};
            put(out, req);
            const std::vector<int64_t> home = mm2.Released();
            put(out, home.size() == 1 ? home[0] : (int64_t)-1);
            second.Restart();
            const int32_t restarted[2] = {second.Stage(), second.State().frame};
            put(out, restarted);
        } else {
            std::atomic<bool> stop{false};
            std::atomic<int> failed{0};
            std::thread mapmaker([&] {
                try {
                    mm.Run(stop);
                } catch (const std::exception& e) {
                    std::fprintf(stderr, "mapmaker: %s\n", e.what());
                    failed = 1;
                }
            });
            try {
                for (int k = 0; k < n_frames && !failed; k++)
                    if (frame(k).init_requested)
                        while (mm.InitPoll() != PTAM_MM_INIT_DONE && !failed) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
            }
            stop = true;
            mapmaker.join();
            if (failed) rc = 5;
        }
        if (!rc) {
            const ptam::TrackState state = tracker.State();
            put(out, static_cast<const ptam_track_state&>(state));
            int free_reports = 0, free_keyframes = 0;
            tracker.Pool(free_reports, free_keyframes);
            const int32_t tail[3] = {free_reports, free_keyframes, last_trails};
            put(out, tail);
            const std::vector<ptam::SE3> poses = map.Download<ptam::SE3>(PTAM_RMAP_KF_POSES);
            const std::vector<ptam_map_meas> meas = map.Download<ptam_map_meas>(PTAM_RMAP_MEAS);
            std::fwrite(poses.data(), sizeof(ptam::SE3), poses.size(), out);
            std::fwrite(meas.data(), sizeof(ptam_map_meas), meas.size(), out);
            const ptam_rmap_counts_t n = map.Counts();
            std::printf("SESSIONDEMO rc %d frames %d tracked %d stage %d branch %d quality %d kf %d points %d\n", rc, n_frames, tracked, tracker.Stage(),
                        last_branch, tracker.Quality(), n.n_kf, n.n_points);
        }
        std::fclose(out);
        for (void* d : d_frames) ptam_dev_free(ct.handle(), d);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "session_demo: %s\n", e.what());
        rc = 4;
    }
    return rc;
}
