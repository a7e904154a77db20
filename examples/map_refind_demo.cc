// map_refind_demo.cc — ptam::MapReFind (ptam_shim.hpp) on map tables read from a file, results written to another
// (tests/test_gpu_map_refind_shim.py builds and runs it).
//   in:  int32 mode, K, N, M, V, W, width, height | two images width x height (frame B, frame A) | K x 12 doubles se3CfromW |
//        N ptam_map_refind_point | M ptam_map_meas | V ptam_map_pair | the work: W int32 (KEYFRAME, NEW_POINTS) or W ptam_map_pair
//        Keyframe entry i of the table is frame B for even i and frame A for odd i.
//   out: ptam_map_refind_result | found rows | their sub-pixel flags | new never pairs | merged meas | merged never
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

template <class T>
static bool get(FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}
template <class T>
static void put(FILE* f, const T* p, size_t n) {
    if (n) std::fwrite(p, sizeof(T), n, f);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: map_refind_demo <tables in> <results out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[8];
    if (!f || !get(f, h, 8)) return 3;
    const int mode = h[0], K = h[1], W = h[5], width = h[6], height = h[7];
    std::vector<uint8_t> im_b((size_t)width * height), im_a((size_t)width * height);
    std::vector<ptam::SE3> poses((size_t)K);
    std::vector<ptam_map_refind_point> points((size_t)h[2]);
    std::vector<ptam_map_meas> meas((size_t)h[3]);
    std::vector<ptam_map_pair> never((size_t)h[4]);
    std::vector<int32_t> work((size_t)W * (mode == PTAM_MAP_REFIND_FAILURE_QUEUE ? 2 : 1));
    if (!get(f, im_b.data(), im_b.size()) || !get(f, im_a.data(), im_a.size()) || !get(f, poses.data(), poses.size()) ||
        !get(f, points.data(), points.size()) || !get(f, meas.data(), meas.size()) || !get(f, never.data(), never.size()) ||
        !get(f, work.data(), work.size()))
        return 3;
    std::fclose(f);
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {width, height});
    ptam::KeyFrame kfb(c), kfa(c);
    kfb.MakeKeyFrame_Lite(im_b.data(), width);
    kfa.MakeKeyFrame_Lite(im_a.data(), width);
    std::vector<const ptam::KeyFrame*> kfs;
    for (int i = 0; i < K; i++) kfs.push_back(i % 2 == 0 ? &kfb : &kfa);
    ptam::ReFinder finder(c);
    const ptam::MapReFindResult r = ptam::MapReFind(c, finder, mode, kfs, poses, points, meas, never, work.data(), W);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    put(g, &r.result, 1);
    put(g, r.vFound.data(), r.vFound.size());
    put(g, r.vFoundSubPix.data(), r.vFoundSubPix.size());
    put(g, r.vNeverNew.data(), r.vNeverNew.size());
    put(g, meas.data(), meas.size());
    put(g, never.data(), never.size());
    std::fclose(g);
    std::printf("MAPREFIND pairs %d skipped %d found %d never %d bad points %d template kept %d\n", r.result.n_pairs, r.result.n_skipped,
                r.result.n_found, r.result.n_never, r.result.n_bad_points, r.result.n_template_kept);
    return 0;
}
