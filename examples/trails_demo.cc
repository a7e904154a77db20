// trails_demo.cc — ptam::TrailTracker (ptam_shim.hpp) on grey frames read from a file: the first frame starts the trails, every
// later one advances them; the trail list after the last frame is printed (tests/test_gpu_trails_shim.py builds and runs it).
//   in: int32 w, h, n_frames, max_trails | double min_shi_tomasi | n_frames x (w * h) bytes
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: trails_demo <frames in>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[4];
    double thr;
    if (!f || std::fread(h, sizeof(int32_t), 4, f) != 4 || std::fread(&thr, sizeof thr, 1, f) != 1) return 3;
    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {h[0], h[1]});
    ptam::KeyFrame kf(c);
    ptam::TrailTracker tt(c, h[3], thr);
    std::vector<uint8_t> im((size_t)h[0] * h[1]);
    for (int k = 0; k < h[2]; k++) {
        if (std::fread(im.data(), 1, im.size(), f) != im.size()) return 3;
        kf.MakeKeyFrame_Lite(im.data(), h[0]);
        if (k == 0) {
            kf.MakeKeyFrame_Rest();
            std::printf("START %d\n", tt.Start(kf));
        } else {
            const int good = tt.Advance(kf);
            std::printf("ADVANCE %d %d\n", good, tt.Alive());
        }
    }
    std::fclose(f);
    for (const ptam_trail& t : tt.Trails()) std::printf("TRAIL %d %d %d %d\n", t.initial_x, t.initial_y, t.current_x, t.current_y);
    std::printf("MATCHES %zu\n", tt.Matches().size());
    return 0;
}
