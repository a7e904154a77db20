// init_map_demo.cc — the first spacebar to a tracked frame without a host-side map table (ptam_shim.hpp): ptam::TrailTracker over a
// short sequence, ptam::ResidentMap::InitFromStereo as one call, Publish, MapTracker::TakeMap, and the last frame tracked from
// se3TrackerPose.  It prints what tests/test_gpu_init_map_shim.py reads.
//   in: int32 w, h, n_frames, max_trails, max_bundles | double min_shi_tomasi | uint64 homography seed, plane seed |
//       n_frames x (w * h) bytes
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

// FNV-1a over a table's bytes
template <class T>
static uint64_t hash_rows(const std::vector<T>& v, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); i++) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
struct Row96 {
    double v[12];
};
struct Row24 {
    double v[3];
};

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: init_map_demo <frames in>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[5];
    double thr;
    uint64_t seeds[2];
    if (!f || std::fread(h, sizeof(int32_t), 5, f) != 5 || std::fread(&thr, sizeof thr, 1, f) != 1 || std::fread(seeds, 8, 2, f) != 2) return 3;
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {h[0], h[1]});
    ptam::KeyFrame kFirst(c), kCurrent(c);
    ptam::TrailTracker tt(c, h[3], thr);
    std::vector<uint8_t> im((size_t)h[0] * h[1]);
    for (int k = 0; k < h[2]; k++) {   // TrackForInitialMap: the first spacebar, then the trails
        if (std::fread(im.data(), 1, im.size(), f) != im.size()) return 3;
        if (k == 0) {
            kFirst.MakeKeyFrame_Lite(im.data(), h[0]);
            kFirst.MakeKeyFrame_Rest();
            std::printf("START %d\n", tt.Start(kFirst));
        } else {
            kCurrent.MakeKeyFrame_Lite(im.data(), h[0]);
            tt.Advance(kCurrent);
        }
    }
    std::fclose(f);
    std::printf("ALIVE %d\n", tt.Alive());
    // the second spacebar: the one call
    ptam::ResidentMap map(c);
    ptam::ResidentMap::InitOpts o = ptam::ResidentMap::InitOptsDefault();
    o.max_bundles = h[4];
    o.ba.deterministic = 1;
    o.homography.seed = seeds[0];
    o.plane.seed = seeds[1];
    ptam::SE3 se3TrackerPose = ptam::SE3::Identity();
    const bool ok = map.InitFromStereo(kFirst, kCurrent, tt, se3TrackerPose, o);
    const ptam_rmap_init_result& r = map.LastInit();
    std::printf("INIT %d %d %d %d %d %d %d %d %d\n", (int)ok, r.status, r.n_matches, r.n_made, r.n_bundles, r.n_outliers, r.n_epipolar, r.plane.status,
                r.plane.n_inliers);
    std::printf("COUNTS %d %d %d %d %d %d\n", r.counts.n_kf, r.counts.n_points, r.counts.n_meas, r.counts.n_never, r.counts.n_new, r.counts.n_failure);
    if (!ok) return 0;
    double p[12];
    se3TrackerPose.to12(p);
    std::printf("POSE");
    for (double x : p) std::printf(" %.17g", x);
    std::printf("\n");
    uint64_t hs = hash_rows(map.Download<Row96>(PTAM_RMAP_KF_POSES));
    hs = hash_rows(map.Download<Row24>(PTAM_RMAP_POINTS3), hs);
    hs = hash_rows(map.Download<ptam_map_refind_point>(PTAM_RMAP_REFIND_POINTS), hs);
    hs = hash_rows(map.Download<ptam_map_point_source>(PTAM_RMAP_SOURCES), hs);
    hs = hash_rows(map.Download<uint8_t>(PTAM_RMAP_BAD), hs);
    hs = hash_rows(map.Download<ptam_map_meas>(PTAM_RMAP_MEAS), hs);
    hs = hash_rows(map.Download<int32_t>(PTAM_RMAP_NEW_QUEUE), hs);
    std::printf("TABLES %" PRIu64 "\n", hs);
    // the map to the tracker, on the device, and one frame tracked from se3TrackerPose
    ptam::MapSnapshot snapshot(c, r.counts.n_points);
    const ptam_map_publish_result pub = map.Publish(snapshot);
    ptam::MapTracker tracker(c, r.counts.n_points);
    const ptam_map_take_result took = tracker.TakeMap(snapshot);
    std::printf("TAKE %d %d %d\n", pub.n_points, took.n_points, took.n_new);
    const ptam_trackmap_result t = tracker.TrackMap(kCurrent, se3TrackerPose);
    std::printf("TRACK %d %d %d %d %d\n", t.n_meas, t.found[0], t.found[1], t.found[2], t.found[3]);
    std::printf("TRACKED");
    for (double x : t.pose) std::printf(" %.17g", x);
    std::printf("\n");
    return 0;
}
