// resident_map_demo.cc — one MapMaker::run() iteration (src/MapMaker.cc:57-114) on a ptam::ResidentMap (ptam_shim.hpp): the map goes
// up once, every step works on the tables in device memory, and the tables come down once at the end
// (tests/test_gpu_resident_map_shim.py builds and runs it).  The steps: BundleAdjust RECENT and its outliers, ReFind of the new-point
// queue, BundleAdjust ALL and its outliers, ReFind of the failure queue, HandleBadPoints, a new keyframe (frame A) with its rows,
// ReFind in it, new points between it and keyframe `target`, the scene depth.
//   in:  int32 K, N, M, V, Q, A, R, width, height, target_kf, target_source, 0 | two images width x height (frame B, frame A; keyframe
//        i of the table is frame B for even i, frame A for odd i) | K x 12 doubles poses | K bytes bFixed | N x 3 doubles points3 |
//        N ptam_map_refind_point | N ptam_map_point_source | N bytes bBad | M ptam_map_meas | V ptam_map_pair never | Q int32 new queue |
//        A ptam_new_map_point | 12 doubles: the new keyframe's pose | R ptam_map_kf_row: its measurements
//   out: ptam_rmap_counts_t | int32 outliers of the two bundles | the three ptam_map_refind_result | ptam_map_bad_points_result |
//        kept | the twelve tables in PTAM_RMAP_* order | K + 1 ptam_scene_depth
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static unsigned put(FILE* f, const std::vector<T>& v) {   // -> a byte sum, for the printed line
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
    unsigned s = 0;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); i++) s = s * 31u + p[i];
    return s;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: resident_map_demo <map in> <tables out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> h;
    if (!f || !get(f, h, 12)) return 3;
    const size_t K = (size_t)h[0], N = (size_t)h[1];
    const int width = h[7], height = h[8];
    std::vector<uint8_t> im_b, im_a, fixed, bad;
    std::vector<ptam::SE3> poses, new_pose;
    std::vector<ptam::Vec<3>> points;
    std::vector<ptam_map_refind_point> rpoints;
    std::vector<ptam_map_point_source> sources;
    std::vector<ptam_map_meas> meas;
    std::vector<ptam_map_pair> never;
    std::vector<int32_t> new_queue;
    std::vector<ptam_new_map_point> made;
    std::vector<ptam_map_kf_row> rows;
    if (!get(f, im_b, (size_t)width * height) || !get(f, im_a, (size_t)width * height) || !get(f, poses, K) || !get(f, fixed, K) ||
        !get(f, points, N) || !get(f, rpoints, N) || !get(f, sources, N) || !get(f, bad, N) || !get(f, meas, (size_t)h[2]) ||
        !get(f, never, (size_t)h[3]) || !get(f, new_queue, (size_t)h[4]) || !get(f, made, (size_t)h[5]) || !get(f, new_pose, 1) ||
        !get(f, rows, (size_t)h[6]))
        return 3;
    std::fclose(f);
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {width, height});
    ptam::KeyFrame kfb(c), kfa(c);
    kfb.MakeKeyFrame_Lite(im_b.data(), width);
    kfa.MakeKeyFrame_Lite(im_a.data(), width);
    std::vector<const ptam::KeyFrame*> kfs;
    for (size_t i = 0; i < K; i++) kfs.push_back(i % 2 == 0 ? &kfb : &kfa);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;

    {
        ptam::ResidentMap map(c);   // (destroyed before the context)
        ptam::ReFinder finder(c);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, never, new_queue, {});
        ptam_ba_opts opts;
        ptam_ba_opts_default(&opts);
        opts.deterministic = 1;
        int32_t n_outliers[2];
        ptam_map_refind_result refound[3];
        ptam::MapBundleAdjustResult ba = map.BundleAdjust(PTAM_MAP_BA_RECENT, &opts);
        map.ApplyBundleOutliers(ba.outliers);
        n_outliers[0] = ba.result.n_outliers;
        refound[0] = map.ReFind(finder, PTAM_MAP_REFIND_NEW_POINTS).result;
        ba = map.BundleAdjust(PTAM_MAP_BA_ALL, &opts);
        map.ApplyBundleOutliers(ba.outliers);
        n_outliers[1] = ba.result.n_outliers;
        refound[1] = map.ReFind(finder, PTAM_MAP_REFIND_FAILURE_QUEUE).result;
        const ptam::HandleBadPointsResult rb = map.HandleBadPoints();
        map.AddKeyFrame(&kfa, new_pose[0], false, rows);
        const int32_t k_new = (int32_t)K;
        refound[2] = map.ReFind(finder, PTAM_MAP_REFIND_KEYFRAME, &k_new, 1).result;
        map.AddPointsToTables(k_new, h[9], made, h[10]);
        const std::vector<ptam_scene_depth> depth = map.RefreshSceneDepth();

        const ptam_rmap_counts_t n = map.Counts();
        std::fwrite(&n, sizeof n, 1, g);
        std::fwrite(n_outliers, sizeof n_outliers, 1, g);
        std::fwrite(refound, sizeof refound, 1, g);
        std::fwrite(&rb.result, sizeof rb.result, 1, g);
        unsigned sum = put(g, rb.vKept);
        sum += put(g, map.Download<ptam::SE3>(PTAM_RMAP_KF_POSES));
        sum += put(g, map.Download<uint8_t>(PTAM_RMAP_KF_FIXED));
        sum += put(g, map.Download<ptam::Vec<3>>(PTAM_RMAP_POINTS3));
        sum += put(g, map.Download<ptam_map_refind_point>(PTAM_RMAP_REFIND_POINTS));
        sum += put(g, map.Download<ptam_map_point_source>(PTAM_RMAP_SOURCES));
        sum += put(g, map.Download<uint8_t>(PTAM_RMAP_BAD));
        sum += put(g, map.Download<int32_t>(PTAM_RMAP_OUTLIER_COUNT));
        sum += put(g, map.Download<int32_t>(PTAM_RMAP_INLIER_COUNT));
        sum += put(g, map.Download<ptam_map_meas>(PTAM_RMAP_MEAS));
        sum += put(g, map.Download<ptam_map_pair>(PTAM_RMAP_NEVER));
        sum += put(g, map.Download<int32_t>(PTAM_RMAP_NEW_QUEUE));
        sum += put(g, map.Download<ptam_map_pair>(PTAM_RMAP_FAILURE));
        sum += put(g, depth);
        unsigned long long up = 0, down = 0;
        map.Traffic(up, down);
        std::printf("RESIDENTMAP kf %d points %d meas %d never %d new %d failure %d outliers %d+%d refound %d+%d+%d removed %d checksum %08x up %llu "
                    "down %llu\n", n.n_kf, n.n_points, n.n_meas, n.n_never, n.n_new, n.n_failure, n_outliers[0], n_outliers[1], refound[0].n_found,
                    refound[1].n_found, refound[2].n_found, rb.result.n_removed, sum, up, down);
    }
    std::fclose(g);
    return 0;
}
