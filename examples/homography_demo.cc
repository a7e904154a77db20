// homography_demo.cc — ptam::HomographyInit (ptam_shim.hpp) on matches and a sample table read from a file; the pose, the status
// and the inlier count are printed (tests/test_gpu_homography_shim.py builds and runs it).
//   in: int32 n_matches, n_trials | double max_pixel_error | n_matches x 8 doubles (first, second, jac) | n_trials x 4 int32
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: homography_demo <matches in>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[2];
    double max_err;
    if (!f || std::fread(h, sizeof(int32_t), 2, f) != 2 || std::fread(&max_err, sizeof max_err, 1, f) != 1 || h[0] < 0 || h[1] < 0) return 3;
    std::vector<ptam::HomographyMatch> m((size_t)h[0]);
    std::vector<int32_t> samples((size_t)h[1] * 4);
    if (std::fread(m.data(), sizeof m[0], m.size(), f) != m.size() || std::fread(samples.data(), sizeof(int32_t), samples.size(), f) != samples.size())
        return 3;
    std::fclose(f);
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {160, 128});
    ptam::HomographyInit hi(c);
    hi.SetSamples(samples);
    ptam::SE3 se3 = ptam::SE3::Identity();
    const bool ok = hi.Compute(m, max_err, se3);
    std::printf("OK %d STATUS %d\n", ok ? 1 : 0, hi.Info().status);
    std::printf("INLIERS %d BEST_TRIAL %d AMBIGUOUS %d\n", hi.Info().n_inliers, hi.Info().best_trial, hi.Info().ambiguous);
    std::printf("SE3");
    for (int i = 0; i < 9; i++) std::printf(" %.17g", se3.R[i]);
    for (int i = 0; i < 3; i++) std::printf(" %.17g", se3.t[i]);
    std::printf("\n");
    return 0;
}
