// frame_report_demo.cc — a tracked frame handed from the tracker's thread to the mapmaker's on the device (ptam_shim.hpp): the
// opposite direction of publish_map_demo.cc.  The tracker thread takes the published map, tracks FRAMES frames and reports each
// (MapTracker::ReportFrame) into a report of a small pool, which it passes to the mapmaker through a queue; the pool and the queue
// are this program's, as mvpKeyFrameQueue is the reference's.  The mapmaker thread notes every report in the map's counts
// (ResidentMap::NoteTracked(report)), runs HandleBadPoints after the second one — so the later reports name points that are gone
// — and inserts the last frame as a keyframe from its report.  No record crosses the host link on either side
// (tests/test_gpu_frame_report_shim.py builds and runs it).
//   in:  the file of examples/insert_keyframe_demo.cc
//   out: FRAMES x int32 {tag, n_records, n_outliers, n_gone} | int32 n_removed, n_rows, n_gone, n_made |
//        int32 n_points, n_meas | n_points int32 outlier_count | n_points int32 inlier_count | n_meas ptam_map_meas |
//        n_points int64 serials | the first frame's records
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <memory>
#include <mutex>
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

// the two lists between the threads: reports the tracker may fill, reports the mapmaker has yet to consume
struct Channel {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<ptam::FrameReport*> free_list, filled;
    bool stop = false;
    void push(std::deque<ptam::FrameReport*>& q, ptam::FrameReport* r) {
        {
            std::lock_guard<std::mutex> l(mu);
            q.push_back(r);
        }
        cv.notify_all();
    }
    ptam::FrameReport* pop(std::deque<ptam::FrameReport*>& q) {   // null: the other thread has failed
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return stop || !q.empty(); });
        if (q.empty()) return nullptr;
        ptam::FrameReport* r = q.front();
        q.pop_front();
        return r;
    }
    void abort() {
        {
            std::lock_guard<std::mutex> l(mu);
            stop = true;
        }
        cv.notify_all();
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: frame_report_demo <map in> <lists out>\n");
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
    kfa.MakeKeyFrame_Lite(im_a.data(), width);
    kfa.MakeKeyFrame_Rest();
    cur.MakeKeyFrame_Lite(im_a.data(), width);
    std::vector<const ptam::KeyFrame*> kfs;
    for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    const int cap = (int)N + 4096;
    enum { FRAMES = 4, POOL = 2 };
    int rc = 0;
    {
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        ptam::MapTracker tracker(ct, cap);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(snapshot);
        // every fifth row's point was an outlier in 21 frames: the HandleBadPoints below removes it
        std::vector<int32_t> pts;
        for (size_t i = 0; i < rows.size(); i += 5)
            for (int k = 0; k < 21; k++) pts.push_back(rows[i].point);
        map.NoteTracked(pts, std::vector<uint8_t>(pts.size(), 1));

        std::vector<std::unique_ptr<ptam::FrameReport>> pool;
        Channel ch;
        for (int i = 0; i < POOL; i++) {
            pool.emplace_back(new ptam::FrameReport(ct, cap));
            ch.free_list.push_back(pool.back().get());
        }
        std::atomic<int> failed{0};
        int32_t per_frame[FRAMES][4] = {}, tail[4] = {};
        std::vector<ptam_frame_record> first_records;

        std::thread tracking([&] {
            try {
                tracker.TakeMap(snapshot);
                for (int frame = 0; frame < FRAMES; frame++) {
                    tracker.TrackMap(cur, new_pose[0]);
                    ptam::FrameReport* r = ch.pop(ch.free_list);   // (waits while the mapmaker holds the whole pool)
                    if (!r) return;
                    tracker.ReportFrame(*r, frame);                // complete on the device when this returns
                    ch.push(ch.filled, r);
                }
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
                ch.abort();
            }
        });
        std::thread mapmaker([&] {
            try {
                for (int frame = 0; frame < FRAMES; frame++) {
                    ptam::FrameReport* r = ch.pop(ch.filled);
                    if (!r) return;
                    const ptam_frame_report_info_t info = r->Info();
                    if (frame == 0) first_records = r->Read();
                    const ptam_rmap_note_result note = map.NoteTracked(*r);
                    const int32_t row[4] = {(int32_t)info.tag, info.n_records, info.n_outliers, note.n_gone};
                    std::copy(row, row + 4, per_frame[frame]);
                    if (frame == 1) tail[0] = map.HandleBadPoints(false).result.n_removed;
                    if (frame == FRAMES - 1) {   // the last frame becomes a keyframe: its measurements are its report
                        ptam_rmap_insert_opts opts = ptam::ResidentMap::InsertOpts(par[0], par[1]);
                        opts.epipolar.min_shi_tomasi = par[2];
                        opts.target_kf = h[7];
                        tail[3] = map.InsertKeyFrame(finder, kfa, new_pose[0], false, *r, opts, &tail[1], &tail[2]).n_made;
                    }
                    ch.push(ch.free_list, r);      // the tracker may refill it
                }
            } catch (const std::exception& e) {
                std::fprintf(stderr, "mapmaker: %s\n", e.what());
                failed = 1;
                ch.abort();
            }
        });
        tracking.join();
        mapmaker.join();
        if (failed) rc = 5;

        if (!rc) {
            const ptam_rmap_counts_t n = map.Counts();
            const int32_t sizes[2] = {n.n_points, n.n_meas};
            std::fwrite(per_frame, sizeof per_frame, 1, g);
            std::fwrite(tail, sizeof tail, 1, g);
            std::fwrite(sizes, sizeof sizes, 1, g);
            put(g, map.Download<int32_t>(PTAM_RMAP_OUTLIER_COUNT));
            put(g, map.Download<int32_t>(PTAM_RMAP_INLIER_COUNT));
            put(g, map.Download<ptam_map_meas>(PTAM_RMAP_MEAS));
            put(g, map.PointSerials());
            put(g, first_records);
            std::printf("FRAMEREPORT frames %d records %d gone %d removed %d rows %d rows-gone %d made %d points %d meas %d\n", (int)FRAMES,
                        per_frame[FRAMES - 1][1], per_frame[FRAMES - 1][3], tail[0], tail[1], tail[2], tail[3], n.n_points, n.n_meas);
        }
    }
    std::fclose(g);
    return rc;
}
