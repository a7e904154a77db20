// mapmaker_demo.cc — ptam::MapMaker (ptam_shim.hpp): the mapmaker's thread of the reference over a ResidentMap, as a two-thread host
// instantiates it (tests/test_gpu_mapmaker_shim.py builds and runs it).
// Part 1, one thread: a tracked frame is noted, a second one is queued as a keyframe, and three Step()s are taken — the keyframe
// (only HandleBadPoints and the insert run while the queue is not empty), then the new points and the bundles under the flags.
// Every step's result is printed, and the tables are written out, for comparison with the same sequence through host.MapMaker.
// Part 2, two threads, a context each: the tracker's thread takes the map the mapmaker publishes, tracks, reports, and hands every
// frame over — every second one as a keyframe (AddKeyFrame), the others to be counted (NoteFrame) — while the mapmaker's thread
// sits in Run().  The reports are the tracker's until their tags come back from Released().  Checked: every tag comes back exactly
// once, every keyframe is in the map, the measurement table is in (kf, point) order; and it ends.
//   in:  the file of examples/insert_keyframe_demo.cc
//   out: n_meas ptam_map_meas | n_kf poses | n_points int64 serials, as part 1 left them
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "ptam_shim.hpp"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: mapmaker_demo <map in> <tables out>\n");
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
    std::vector<ptam_map_kf_row> rows;
    const size_t px = (size_t)width * height;
    if (!get(f, im_b, px) || !get(f, im_c, px) || !get(f, im_a, px) || !get(f, poses, K) || !get(f, fixed, K) || !get(f, points, N) ||
        !get(f, rpoints, N) || !get(f, sources, N) || !get(f, bad, N) || !get(f, meas, (size_t)h[2]) || !get(f, new_queue, (size_t)h[3]) ||
        !get(f, new_pose, 1) || !get(f, rows, (size_t)h[4]))
        return 3;
    std::fclose(f);
    const ptam::Vec<5> cam{1.0803, 1.43987, 0.519983, 0.548655, 0.244943};
    ptam::Context cm(cam, {width, height}), ct(cam, {width, height});   // the mapmaker's and the tracker's: one queue each
    ptam::KeyFrame kfb(cm), kfc(cm), kfa(cm), cur(ct);
    kfb.MakeKeyFrame_Lite(im_b.data(), width);
    kfc.MakeKeyFrame_Lite(im_c.data(), width);
    kfa.MakeKeyFrame_Lite(im_a.data(), width);   // (no MakeKeyFrame_Rest: the step runs it on a keyframe that lacks it, :500)
    cur.MakeKeyFrame_Lite(im_a.data(), width);
    std::vector<const ptam::KeyFrame*> kfs;
    for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    const int cap = (int)N + 8192;
    ptam_mapmaker_opts opts = ptam::MapMaker::DefaultOpts();
    opts.ba.deterministic = 1;
    opts.insert.epipolar.min_shi_tomasi = par[2];
    opts.failure_period = 1;
    const auto pose_at = [&](int i) {
        ptam::SE3 p = new_pose[0];
        p.t[0] += 0.015 * i;   // another camera centre for every keyframe
        return p;
    };

    // ---- part 1
    {
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap), own(cm, cap);   // what Step() publishes into | what this part's tracker takes
        ptam::MapTracker tracker(ct, cap);
        ptam::FrameReport noted(ct, cap), queued(ct, cap);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(own);
        tracker.TakeMap(own);
        ptam::MapMaker mm(map, finder, &snapshot, &opts);
        tracker.TrackMap(cur, new_pose[0]);
        tracker.ReportFrame(noted, 1);
        mm.NoteFrame(noted, 1);
        tracker.TrackMap(cur, new_pose[0]);
        tracker.ReportFrame(queued, 2);
        mm.AddKeyFrame(kfa, pose_at(1), false, queued, par[0], par[1], 2);
        for (int step = 0; step < 3; step++) {
            const ptam_mapmaker_step_result r = mm.Step();
            const ptam_rmap_counts_t n = map.Counts();
            std::printf("MAPMAKER step %d status %d stages %d recent %d full %d queue %d draws %llu kf %d points %d meas %d never %d new %d failure %d "
                        "rows %d made %d removed %d accepted %d generation %lld released",
                        step, r.status, r.stages, r.converged_recent, r.converged_full, r.queue_size, (unsigned long long)r.draws, n.n_kf, n.n_points,
                        n.n_meas, n.n_never, n.n_new, n.n_failure, r.insert_rows, r.insert.n_made, r.bad_points.n_removed, r.all.accepted,
                        (long long)r.publish.generation);
            for (int64_t t : mm.Released()) std::printf(" %lld", (long long)t);
            std::printf("\n");
        }
        put(g, map.Download<ptam_map_meas>(PTAM_RMAP_MEAS));
        put(g, map.Download<ptam::SE3>(PTAM_RMAP_KF_POSES));
        put(g, map.PointSerials());
    }
    std::fclose(g);

    // ---- part 2
    enum { FRAMES = 8 };
    int rc = 0;
    {
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        ptam::MapTracker tracker(ct, cap);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(snapshot);
        ptam::MapMaker mm(map, finder, &snapshot, &opts);
        std::vector<std::unique_ptr<ptam::FrameReport>> reports;
        for (int i = 0; i < FRAMES; i++) reports.emplace_back(new ptam::FrameReport(ct, cap));
        std::atomic<bool> stop{false};
        std::atomic<int> failed{0};
        std::vector<int> back(FRAMES, 0);   // the tracker's thread alone counts the tags that came back
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(60);

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
                int n_back = 0;
                const auto collect = [&] {
                    for (int64_t t : mm.Released()) {
                        if (t < 0 || t >= FRAMES) throw std::runtime_error("a tag that was never handed over");
                        back[(size_t)t]++;
                        n_back++;
                    }
                };
                for (int frame = 0; frame < FRAMES && !failed; frame++) {
                    tracker.TakeMap(snapshot);
                    tracker.TrackMap(cur, new_pose[0]);
                    tracker.ReportFrame(*reports[(size_t)frame], frame);
                    if (frame % 2 == 1) mm.AddKeyFrame(kfa, pose_at(frame), false, *reports[(size_t)frame], par[0], par[1], frame);
                    else mm.NoteFrame(*reports[(size_t)frame], frame);
                    collect();
                }
                while (n_back < FRAMES && !failed) {   // the mapmaker works the queue off
                    if (std::chrono::steady_clock::now() > deadline) throw std::runtime_error("the tags did not come back in 60 s");
                    std::this_thread::sleep_for(std::chrono::milliseconds(2));
                    collect();
                }
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
            }
        });
        tracking.join();
        stop = true;
        mapmaker.join();
        if (failed) rc = 5;
        if (!rc) {
            for (int c : back)
                if (c != 1) rc = 6;   // every tag exactly once
            const ptam_rmap_counts_t n = map.Counts();
            if (n.n_kf != (int)K + FRAMES / 2 || mm.QueueSize() != 0) rc = 7;
            const std::vector<ptam_map_meas> m = map.Download<ptam_map_meas>(PTAM_RMAP_MEAS);
            for (size_t i = 1; i < m.size(); i++)
                if (!(m[i - 1].kf < m[i].kf || (m[i - 1].kf == m[i].kf && m[i - 1].point < m[i].point))) rc = 8;
            for (const ptam_map_meas& r : m)
                if (r.kf < 0 || r.kf >= n.n_kf || r.point < 0 || r.point >= n.n_points) rc = 8;
            std::printf("TWOTHREAD rc %d frames %d kf %d points %d meas %d queue %d\n", rc, (int)FRAMES, n.n_kf, n.n_points, n.n_meas, mm.QueueSize());
        }
    }
    return rc;
}
