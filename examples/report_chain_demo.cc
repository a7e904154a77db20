// report_chain_demo.cc — one tracker-thread frame as ONE call (ptam_shim.hpp): MapTracker::TrackFramesReportBatch draws the frame's two
// random orders on the device, tracks the frame and leaves its FrameReport filled; what stays the caller's is shown with it — the
// keyframe for MapMaker::AddKeyFrame copied into a pooled one without an allocation (KeyFrame::CopyFrom).  Three frames of one camera
// on a published map, then the orders by themselves (DrawShuffles / ReadShuffle against ShuffleOrder, the same order in host code),
// then a frame whose report is one record too small: the call says so, the frame is delivered and the state has moved
// (tests/test_gpu_report_chain_shim.py builds and runs it).
//   in:  the file of examples/insert_keyframe_demo.cc
//   out: FRAMES x { ptam_trackmap_result | ptam_track_state | int64 tag, n_records, n_entries, n_outliers, in_chain, too_small } |
//        the first frame's records | int32 n | the orders after frame 0: read back (2 x n), ShuffleOrder (2 x n) |
//        the orders of DrawShuffles(seed, 77): read back (2 x n) | the pooled keyframe after CopyFrom: per level int32 corners,
//        the corners, the row LUT; level 3's pixels | the too-small frame: int64 delivered, ptam_track_state, the six words, the
//        small report's n_records
#include <cstdio>
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
static void put_info(FILE* g, const ptam_track_report_info& r) {
    const int64_t w[6] = {r.report.tag, r.report.n_records, r.report.n_entries, r.report.n_outliers, r.report_in_chain, r.report_too_small};
    std::fwrite(w, sizeof w, 1, g);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: report_chain_demo <map in> <lists out>\n");
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
    const uint64_t SEED = 0x2545F4914F6CDD1Dull;
    enum { FRAMES = 3 };
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    int rc = 0;
    try {
        ptam::Context cm(cam, {width, height}), ct(cam, {width, height});   // the mapmaker's and the tracker's
        ptam::KeyFrame kfb(cm), kfc(cm), cur(ct), pooled(ct);
        kfb.MakeKeyFrame_Lite(im_b.data(), width);
        kfc.MakeKeyFrame_Lite(im_c.data(), width);
        pooled.MakeKeyFrame_Lite(im_b.data(), width);     // a clone from the pool: it held another frame, and its rest data
        pooled.MakeKeyFrame_Rest();
        std::vector<const ptam::KeyFrame*> kfs;
        for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
        const int cap = (int)N + 4096;
        ptam::ResidentMap map(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        ptam::MapTracker tracker(ct, cap);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(snapshot);
        const int n = tracker.TakeMap(snapshot).n_points;
        void* d_frame = nullptr;
        ptam::check(ptam_dev_alloc(ct.handle(), px, &d_frame), "ptam_dev_alloc");
        ptam::check(ptam_dev_upload(ct.handle(), d_frame, im_a.data(), px), "ptam_dev_upload");

        ptam::FrameReport report(ct, cap);
        std::vector<ptam::TrackState> states(1, ptam::TrackState(new_pose[0]));
        std::vector<ptam_trackmap_result> res;
        std::vector<ptam_track_frame_state_info> info;
        std::vector<ptam_track_report_info> rinfo;
        std::vector<ptam_frame_record> first;
        std::vector<int32_t> la, lb;
        int last_records = 0;
        for (int frame = 0; frame < FRAMES; frame++) {
            const bool ok = ptam::MapTracker::TrackFramesReportBatch({&tracker}, {&cur}, {(const uint8_t*)d_frame}, states, {}, {}, {&report},
                                                                     {10 + frame}, {SEED}, res, info, rinfo);
            if (!ok) throw std::runtime_error("a report of the map's size was too small");
            std::fwrite(&res[0], sizeof res[0], 1, g);
            std::fwrite(static_cast<const ptam_track_state*>(&states[0]), sizeof(ptam_track_state), 1, g);
            put_info(g, rinfo[0]);
            if (frame == 0) {
                first = report.Read();
                tracker.ReadShuffle(n, la, lb);      // what the chain drew for frame 0 of this state
            }
            last_records = rinfo[0].report.n_records;
        }
        put(g, first);
        const int32_t n32 = n;
        std::fwrite(&n32, 4, 1, g);
        put(g, la);
        put(g, lb);
        put(g, ptam::MapTracker::ShuffleOrder(SEED, 0, 0, n));
        put(g, ptam::MapTracker::ShuffleOrder(SEED, 0, 1, n));
        tracker.DrawShuffles(SEED, 77);
        tracker.ReadShuffle(n, la, lb);
        put(g, la);
        put(g, lb);
        // the hand-over's keyframe: the current one into the pooled clone
        pooled.CopyFrom(cur);
        for (int l = 0; l < PTAM_LEVELS; l++) {
            const ptam::Level& L = pooled.aLevels(l);
            const int32_t nc = (int32_t)L.vCorners.size();
            std::fwrite(&nc, 4, 1, g);
            put(g, L.vCorners);
            put(g, L.vCornerRowLUT);
            if (l == PTAM_LEVELS - 1) put(g, L.im);
        }
        // a report one record too small for its frame
        ptam::FrameReport small(ct, last_records > 1 ? last_records - 1 : 1);
        const bool ok = ptam::MapTracker::TrackFramesReportBatch({&tracker}, {&cur}, {(const uint8_t*)d_frame}, states, {}, {}, {&small}, {99},
                                                                 {SEED}, res, info, rinfo);
        const int64_t delivered = ok ? 1 : 0;
        std::fwrite(&delivered, 8, 1, g);
        std::fwrite(static_cast<const ptam_track_state*>(&states[0]), sizeof(ptam_track_state), 1, g);
        put_info(g, rinfo[0]);
        const int64_t small_records = small.Info().n_records;
        std::fwrite(&small_records, 8, 1, g);
        std::printf("REPORTCHAIN frames %d points %d records %d in-chain %d too-small-delivered %d state-frame %d\n", (int)FRAMES, n, last_records,
                    rinfo[0].report_in_chain, (int)!ok, states[0].frame);
        ptam_dev_free(ct.handle(), d_frame);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "report_chain_demo: %s\n", e.what());
        rc = 5;
    }
    std::fclose(g);
    return rc;
}
