// plane_align_demo.cc — ptam::AlignMapToPlane and ptam::RefreshSceneDepth (ptam_shim.hpp) on a small synthetic map built here:
// 120 points about the plane z = 2 + x / 4 - y / 8, every fourth one half a unit off it, seen by two keyframes.  The map as it was
// built, the status, the aligner and the scene depths after the call are printed (tests/test_gpu_plane_align_shim.py builds and
// runs it and works the same map through the numpy restatement).
#include <cmath>
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

static uint64_t next(uint64_t& state) {   // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double unit(uint64_t& state) { return (double)(int)(next(state) % 2001) / 1000.0 - 1.0; }   // -1 .. 1 in steps of 1 / 1000

int main() {
    const int n = 120;
    uint64_t state = 2024;
    std::vector<ptam::Vec<3>> points((size_t)n);
    std::vector<ptam_map_point_source> sources((size_t)n);
    std::vector<ptam_map_meas> meas;
    for (int i = 0; i < n; i++) {
        const double x = unit(state), y = unit(state), off = i % 4 == 3 ? 0.5 : 0.02 * unit(state);
        points[(size_t)i] = {x, y, 2.0 + x / 4 - y / 8 + off};
        ptam_map_point_source& s = sources[(size_t)i];
        s.src_kf = i % 2;
        s.pad_ = 0;
        const double u = 0.3 * unit(state), v = 0.3 * unit(state);
        const double c[3][2] = {{u, v}, {u + 0.002, v}, {u, v + 0.002}};
        double* dst[3] = {s.center_nc, s.one_right_nc, s.one_down_nc};
        for (int k = 0; k < 3; k++) {
            const double nrm = std::sqrt(c[k][0] * c[k][0] + c[k][1] * c[k][1] + 1.0);
            dst[k][0] = c[k][0] / nrm, dst[k][1] = c[k][1] / nrm, dst[k][2] = 1.0 / nrm;
        }
    }
    std::vector<ptam::SE3> poses(2, ptam::SE3::Identity());
    poses[1].t[0] = 0.1, poses[1].t[2] = 0.05;
    for (int k = 0; k < 2; k++)
        for (int i = k; i < n; i += 1 + k) meas.push_back(ptam_map_meas{k, i, 0, PTAM_MAP_SRC_ROOT, {0.0, 0.0}});
    for (const auto& p : points) std::printf("POINT %.17g %.17g %.17g\n", p[0], p[1], p[2]);
    for (const auto& s : sources) {
        std::printf("SOURCE %d", s.src_kf);
        for (const double* v : {s.center_nc, s.one_right_nc, s.one_down_nc}) std::printf(" %.17g %.17g %.17g", v[0], v[1], v[2]);
        std::printf("\n");
    }

    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {160, 128});
    ptam_plane_opts o;
    ptam_plane_opts_default(&o);
    o.seed = 5;
    std::vector<ptam_pvs_point> rows;
    const ptam::PlaneAligner a = ptam::AlignMapToPlane(c, poses, points, &sources, &rows, &o);
    std::printf("STATUS %d INLIERS %d BEST_TRIAL %d SKIPPED %d\n", a.info.status, a.info.n_inliers, a.info.best_trial, a.info.trials_skipped);
    std::printf("SE3");
    for (int i = 0; i < 9; i++) std::printf(" %.17g", a.se3.R[i]);
    for (int i = 0; i < 3; i++) std::printf(" %.17g", a.se3.t[i]);
    std::printf("\n");
    for (const auto& r : rows)
        std::printf("ROW %.17g %.17g %.17g %.17g %.17g %.17g\n", r.pixel_right_w[0], r.pixel_right_w[1], r.pixel_right_w[2],
                    r.pixel_down_w[0], r.pixel_down_w[1], r.pixel_down_w[2]);
    for (const auto& d : ptam::RefreshSceneDepth(c, poses, points, meas)) std::printf("DEPTH %.17g %.17g %d\n", d.depth_mean, d.depth_sigma, d.n_meas);
    return a.info.status == PTAM_PLANE_OK ? 0 : 1;
}
