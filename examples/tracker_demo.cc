// tracker_demo.cc — ptam::Tracker and ptam::MapMaker (ptam_shim.hpp) as the two threads of the reference's System over one resident map:
// the tracker's thread calls Tracker::TrackFrame once per frame — the map and its keyframes are taken from the snapshot, the frame's
// random orders are drawn, the frame is tracked, reported and handed over inside that one call — while the mapmaker's thread sits in
// MapMaker::Run().  20 frames; per frame the branch, found / attempted and whether the frame became a keyframe or was noted; at the
// end the mapmaker works its queue off, one more frame brings every tag home, and the table counts are printed
// (tests/test_gpu_camera_tracker_shim.py builds and runs it).
//   in:  the file of examples/insert_keyframe_demo.cc
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "ptam_shim.hpp"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: tracker_demo <map in>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> h;
    std::vector<double> par;
    if (!f || !get(f, h, 8) || !get(f, par, 3)) return 3;
    const size_t K = (size_t)h[0], N = (size_t)h[1];
    const int width = h[5], height = h[6];
    std::vector<uint8_t> im_b, im_c, im_a, fixed, bad;
    std::vector<ptam::SE3> poses, new_pose;
    std::vector<ptam::Vec<3>> points;
    std::vector<ptam_map_refind_point> rpoints;
    std::vector<ptam_map_point_source> sources;
    std::vector<ptam_map_meas> meas;
    std::vector<int32_t> new_queue;
    const size_t px = (size_t)width * height;
    if (!get(f, im_b, px) || !get(f, im_c, px) || !get(f, im_a, px) || !get(f, poses, K) || !get(f, fixed, K) || !get(f, points, N) ||
        !get(f, rpoints, N) || !get(f, sources, N) || !get(f, bad, N) || !get(f, meas, (size_t)h[2]) || !get(f, new_queue, (size_t)h[3]) ||
        !get(f, new_pose, 1))
        return 3;
    std::fclose(f);
    const ptam::Vec<5> cam{1.0803, 1.43987, 0.519983, 0.548655, 0.244943};
    enum { FRAMES = 20 };
    int rc = 0;
    try {
        ptam::Context cm(cam, {width, height}), ct(cam, {width, height});   // the mapmaker's and the tracker's: one queue each
        ptam::KeyFrame kfb(cm), kfc(cm);
        kfb.MakeKeyFrame_Lite(im_b.data(), width);
        kfc.MakeKeyFrame_Lite(im_c.data(), width);
        std::vector<const ptam::KeyFrame*> kfs;
        for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
        const int cap = (int)N + 4096;
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        snapshot.EnableKeyFrames(16);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(snapshot);
        ptam_mapmaker_opts mo = ptam::MapMaker::DefaultOpts();
        mo.insert.epipolar.min_shi_tomasi = par[2];
        mo.ba.deterministic = 1;
        ptam::MapMaker mm(map, finder, &snapshot, &mo);

        ptam_camera_tracker_opts to = ptam::Tracker::DefaultOpts(ct);
        to.max_points = cap, to.max_keyframes = 16, to.shuffle_seed = 7, to.reports = FRAMES + 2, to.keyframes = 4;
        ptam::Tracker tracker(ct, snapshot, mm, &to);
        tracker.Reset(new_pose[0]);
        void* d_frame = nullptr;
        ptam::check(ptam_dev_alloc(ct.handle(), px, &d_frame), "ptam_dev_alloc");
        ptam::check(ptam_dev_upload(ct.handle(), d_frame, im_a.data(), px), "ptam_dev_upload");

        std::atomic<bool> stop{false};
        std::atomic<int> failed{0};
        std::vector<ptam_camera_track_result> results;
        std::thread mapmaker([&] {
            try {
                mm.Run(stop);
            } catch (const std::exception& e) {
                std::fprintf(stderr, "mapmaker: %s\n", e.what());
                failed = 1;
            }
        });
        std::thread tracking([&] {
            try {
                for (int frame = 0; frame < FRAMES && !failed; frame++) results.push_back(tracker.TrackFrame((const uint8_t*)d_frame));
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
            }
        });
        tracking.join();
        stop = true;
        mapmaker.join();
        if (failed) rc = 5;
        int added = 0, noted = 0;
        if (!rc) {
            static const char* const branch[3] = {"tracked", "recovered", "recovery-failed"};
            for (size_t i = 0; i < results.size(); i++) {
                const ptam_camera_track_result& r = results[i];
                int found = 0, attempted = 0;
                for (int l = 0; l < 4; l++) found += r.track.found[l], attempted += r.track.attempted[l];
                std::printf("FRAME %d %s found %d / %d records %d in-chain %d %s queue %d map-points %d\n", (int)i, branch[r.info.branch], found, attempted,
                            r.report.n_records, r.report_in_chain, r.added_keyframe ? "added" : r.noted_frame ? "noted" : "-", r.queue_size,
                            r.map_take.n_points);
                added += r.added_keyframe, noted += r.noted_frame;
            }
            for (int i = 0; i < 4; i++) mm.Step();                                        // at most max_queue keyframes, and the pending notes
            const ptam_camera_track_result last = tracker.TrackFrame((const uint8_t*)d_frame);   // reads the released tags
            int free_reports = 0, free_keyframes = 0;
            tracker.Pool(free_reports, free_keyframes);
            const int out_now = last.added_keyframe || last.noted_frame;
            if (free_reports != to.reports - out_now || free_keyframes != to.keyframes - added - last.added_keyframe) rc = 6;   // every tag came back
            const ptam_rmap_counts_t n = map.Counts();
            if (n.n_kf != (int)K + added || (int)results.size() != FRAMES) rc = rc ? rc : 7;
            const std::vector<ptam_map_meas> m = map.Download<ptam_map_meas>(PTAM_RMAP_MEAS);
            for (size_t i = 1; i < m.size(); i++)
                if (!(m[i - 1].kf < m[i].kf || (m[i - 1].kf == m[i].kf && m[i - 1].point < m[i].point))) rc = rc ? rc : 8;
            const ptam::SE3 pose = tracker.GetCurrentPose();
            (void)pose;
            std::printf("TRACKERDEMO rc %d frames %d added %d noted %d quality %d lost %d kf %d points %d meas %d queue %d free-reports %d free-keyframes %d\n",
                        rc, (int)results.size(), added, noted, tracker.Quality(), tracker.LostFrames(), n.n_kf, n.n_points, n.n_meas, mm.QueueSize(),
                        free_reports, free_keyframes);
        }
        ptam_dev_free(ct.handle(), d_frame);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "tracker_demo: %s\n", e.what());
        rc = 4;
    }
    return rc;
}
