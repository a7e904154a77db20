// calib_demo.cc — ptam::CameraCalibrator (ptam_shim.hpp) on grid corners read from a file: every member is driven, and what it
// returns goes to a result file as %.17g (tests/test_gpu_calib_shim.py builds it, runs it and compares the bits).
//   in:  int32 width, height, n_images, steps_a, steps_b, disable | n_images x int32 n_corners | per corner int32 gx, gy, double u, v
//   out: ADDED / STEP / OPT / PARAMS / POSE / CFG lines
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: calib_demo <corners in> <result out> <camera.cfg out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[6];
    if (!f || std::fread(h, sizeof(int32_t), 6, f) != 6 || h[2] < 1) return 3;
    std::vector<int32_t> counts((size_t)h[2]);
    if (std::fread(counts.data(), sizeof(int32_t), counts.size(), f) != counts.size()) return 3;
    std::vector<ptam::CalibImage> images(counts.size());
    for (size_t k = 0; k < images.size(); k++)
        for (int i = 0; i < counts[k]; i++) {
            ptam_calib_corner c;
            if (std::fread(&c, sizeof c, 1, f) != 1) return 3;
            ptam::CalibGridCorner g;
            g.irGridPos = {c.gx, c.gy};
            g.Params.v2Pos = {c.u, c.v};
            images[k].mvGridCorners.push_back(g);
        }
    std::fclose(f);
    FILE* out = std::fopen(argv[2], "w");
    if (!out) return 4;
    ptam::Context ctx({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {h[0], h[1]});
    ptam::CameraCalibrator cal(ctx, (int)images.size(), 1 << 16);
    cal.Reset(h[5] != 0);
    for (const ptam::CalibImage& im : images) std::fprintf(out, "ADDED %d\n", cal.AddImage(im) ? 1 : 0);
    for (int k = 0; k < h[3]; k++) {
        const bool ok = cal.OptimizeOneStep();
        std::fprintf(out, "STEP %d %.17g %d\n", ok ? 1 : 0, cal.MeanPixelError(), cal.Result().n_measurements);
    }
    const bool ok = cal.Optimize(h[4]);
    std::fprintf(out, "OPT %d %.17g %d %.17g %d\n", ok ? 1 : 0, cal.MeanPixelError(), cal.Result().n_measurements,
                 cal.Result().pixel_aspect_ratio, (int)cal.RMSHistory().size());
    const ptam::Vec<5> p = cal.Params();
    std::fprintf(out, "PARAMS %.17g %.17g %.17g %.17g %.17g\n", p[0], p[1], p[2], p[3], p[4]);
    for (const ptam::CalibImage& im : cal.mvCalibImgs) {
        double q[12];
        im.mse3CamFromWorld.to12(q);
        std::fprintf(out, "POSE");
        for (int i = 0; i < 12; i++) std::fprintf(out, " %.17g", q[i]);
        std::fprintf(out, "\n");
    }
    std::fprintf(out, "CFG %s", ptam::CameraCalibrator::ConfigLine(p).c_str());
    std::fclose(out);
    return cal.SaveCalib(argv[3]) ? 0 : 5;
}
