// map_edit_demo.cc — ptam::ApplyBundleOutliers, ptam::HandleBadPoints and ptam::AddPointsToTables (ptam_shim.hpp) one after the
// other on map tables read from a file, every stage's tables written to another (tests/test_gpu_map_edit_shim.py builds and runs it).
//   in:  int32 K, N, M, V, Q, F, O, A, src_kf, target_kf, target_source, 0 | N bytes bBad | N int32 outlier counts | N int32 inlier
//        counts | M ptam_map_meas | V ptam_map_pair never | Q int32 new queue | F ptam_map_pair failure queue | O ptam_map_outlier |
//        A ptam_new_map_point | N x 3 doubles points3
//   out: ptam_map_outliers_result | bBad | meas | never | failure                                      (after the outliers)
//        ptam_map_bad_points_result | new_index | kept | meas | never | new queue | failure | points3  (after the bad points)
//        meas | A ptam_map_refind_point | A ptam_map_point_source                                       (after the new points)
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

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: map_edit_demo <tables in> <results out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> h;
    if (!f || !get(f, h, 12)) return 3;
    const int K = h[0], N = h[1];
    std::vector<uint8_t> bad;
    std::vector<int32_t> n_out, n_in, new_queue;
    std::vector<ptam_map_meas> meas;
    std::vector<ptam_map_pair> never, failure;
    std::vector<ptam_map_outlier> outliers;
    std::vector<ptam_new_map_point> made;
    std::vector<ptam::Vec<3>> points;
    if (!get(f, bad, (size_t)N) || !get(f, n_out, (size_t)N) || !get(f, n_in, (size_t)N) || !get(f, meas, (size_t)h[2]) ||
        !get(f, never, (size_t)h[3]) || !get(f, new_queue, (size_t)h[4]) || !get(f, failure, (size_t)h[5]) || !get(f, outliers, (size_t)h[6]) ||
        !get(f, made, (size_t)h[7]) || !get(f, points, (size_t)N))
        return 3;
    std::fclose(f);
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {640, 480});
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;

    const ptam_map_outliers_result ro = ptam::ApplyBundleOutliers(c, K, bad, meas, never, failure, outliers);
    std::fwrite(&ro, sizeof ro, 1, g);
    put(g, bad);
    put(g, meas);
    put(g, never);
    put(g, failure);

    const ptam::HandleBadPointsResult rb = ptam::HandleBadPoints(c, K, bad, n_out.data(), n_in.data(), meas, never, new_queue, failure,
                                                                 {{points.data(), (int32_t)sizeof(ptam::Vec<3>), 0}});
    points.resize((size_t)rb.result.n_kept);
    std::fwrite(&rb.result, sizeof rb.result, 1, g);
    put(g, rb.vNewIndex);
    put(g, rb.vKept);
    put(g, meas);
    put(g, never);
    put(g, new_queue);
    put(g, failure);
    put(g, points);

    const ptam::AddPointsResult ra = ptam::AddPointsToTables(c, K, rb.result.n_kept, meas, h[8], h[9], made, h[10]);
    put(g, meas);
    put(g, ra.vPoints);
    put(g, ra.vSources);
    std::fclose(g);
    std::printf("MAPEDIT outliers %d/%d/%d removed %d kept %d made %d rows %d\n", ro.n_point_bad, ro.n_failure_added, ro.n_never_added,
                rb.result.n_removed, rb.result.n_kept, (int)made.size(), (int)meas.size());
    return 0;
}
