// map_ba_demo.cc — ptam::MapBundleAdjust (ptam_shim.hpp) on map tables read from a file, results written to another
// (tests/test_gpu_map_ba_shim.py builds and runs it).
//   in:  int32 mode, K, N, M | K x 12 doubles se3CfromW | K bytes bFixed | N x 3 doubles | M ptam_map_meas
//   out: ptam_map_ba_result | K x 12 doubles | N x 3 doubles | outliers | cam_kf | point_ids
// The bundle runs with deterministic = 1 (bit-identical to the same call made from Python).
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
        std::fprintf(stderr, "usage: map_ba_demo <tables in> <results out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[4];
    if (!f || !get(f, h, 4)) return 3;
    const int mode = h[0];
    std::vector<ptam::SE3> poses((size_t)h[1]);
    std::vector<uint8_t> fixed((size_t)h[1]);
    std::vector<ptam::Vec<3>> points((size_t)h[2]);
    std::vector<ptam_map_meas> meas((size_t)h[3]);
    if (!get(f, poses.data(), poses.size()) || !get(f, fixed.data(), fixed.size()) || !get(f, points.data(), points.size()) ||
        !get(f, meas.data(), meas.size()))
        return 3;
    std::fclose(f);
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {640, 480});
    ptam_ba_opts o;
    ptam_ba_opts_default(&o);
    o.deterministic = 1;
    const ptam::MapBundleAdjustResult r = ptam::MapBundleAdjust(c, mode, poses, fixed, points, meas, nullptr, &o);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    put(g, &r.result, 1);
    put(g, poses.data(), poses.size());
    put(g, points.data(), points.size());
    put(g, r.outliers.data(), r.outliers.size());
    put(g, r.cam_kf.data(), r.cam_kf.size());
    put(g, r.point_ids.data(), r.point_ids.size());
    std::fclose(g);
    std::printf("MAPBA ran %d accepted %d adjust %d fixed %d points %d meas %d outliers %d\n", r.result.ran, r.result.accepted,
                r.result.n_adjust, r.result.n_fixed, r.result.n_points, r.result.n_meas, r.result.n_outliers);
    return 0;
}
