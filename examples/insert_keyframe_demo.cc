// insert_keyframe_demo.cc — MapMaker::AddKeyFrameFromTopOfQueue (src/MapMaker.cc:493-518) as ONE call on a ptam::ResidentMap
// (ptam_shim.hpp): the map goes up, ResidentMap::InsertKeyFrame adds the keyframe's rows, re-finds the map's points in it, picks the
// closest keyframe, makes new points against it and appends them to the tables, all on the device; ResidentMap::ClosestKeyFrames
// ranks the map's keyframes around the new one; the tables come down once at the end
// (tests/test_gpu_insert_keyframe_shim.py builds and runs it).
//   in:  int32 K, N, M, Q, R, width, height, target_kf | 3 doubles: depth mean, depth sigma, Shi-Tomasi threshold |
//        three images width x height: B (keyframes 0 and 1 of the table), C (keyframe 2 and later), A (the new keyframe) |
//        K x 12 doubles poses | K bytes bFixed | N x 3 doubles points3 | N ptam_map_refind_point | N ptam_map_point_source | N bytes bBad |
//        M ptam_map_meas | Q int32 new queue | 12 doubles: the new keyframe's pose | R ptam_map_kf_row: its measurements
//   out: ptam_rmap_insert_result | int32 n_closest | n_closest int32 keyframes | n_closest doubles distances | ptam_rmap_counts_t |
//        the twelve tables in PTAM_RMAP_* order
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
        std::fprintf(stderr, "usage: insert_keyframe_demo <map in> <tables out>\n");
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
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {width, height});
    ptam::KeyFrame kfb(c), kfc(c), kfa(c);
    kfb.MakeKeyFrame_Lite(im_b.data(), width);
    kfc.MakeKeyFrame_Lite(im_c.data(), width);
    kfa.MakeKeyFrame_Lite(im_a.data(), width);
    kfa.MakeKeyFrame_Rest();
    std::vector<const ptam::KeyFrame*> kfs;
    for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;

    {
        ptam::ResidentMap map(c);   // (destroyed before the context)
        ptam::ReFinder finder(c);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        ptam_rmap_insert_opts opts = ptam::ResidentMap::InsertOpts(par[0], par[1]);
        opts.epipolar.min_shi_tomasi = par[2];
        opts.target_kf = h[7];
        const ptam_rmap_insert_result r = map.InsertKeyFrame(finder, kfa, new_pose[0], false, rows, opts);
        std::vector<double> dist;
        const std::vector<int32_t> closest = map.ClosestKeyFrames(r.kf, (int)K, &dist);
        const int32_t n_closest = (int32_t)closest.size();

        const ptam_rmap_counts_t n = map.Counts();
        std::fwrite(&r, sizeof r, 1, g);
        std::fwrite(&n_closest, sizeof n_closest, 1, g);
        unsigned sum = put(g, closest);
        sum += put(g, dist);
        std::fwrite(&n, sizeof n, 1, g);
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
        std::printf("INSERTKEYFRAME kf %d target %d refound %d never %d made %d first %d points %d meas %d closest %d checksum %08x\n", r.kf,
                    r.target_kf, r.refind.n_found, r.refind.n_never, r.n_made, r.first_point, n.n_points, n.n_meas, n_closest ? closest[0] : -1, sum);
    }
    std::fclose(g);
    return 0;
}
