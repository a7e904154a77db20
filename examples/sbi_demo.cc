// sbi_demo.cc — ptam::SmallBlurryImage and ptam::Relocaliser (ptam_shim.hpp) on three synthetic 336x272 frames built here: a smooth
// pattern, the same pattern seen after a small in-plane turn and shift, and a different pattern.  The frames, one CalcSBIRotation
// and one AttemptRecovery are printed (tests/test_gpu_sbi_shim.py builds and runs it and works the same frames through the numpy
// restatement).
#include <cmath>
#include <cstdio>
#include <vector>

#include "ptam_shim.hpp"

static const int W = 336, H = 272;

// the pattern at (x, y), turned by `turn` about the image centre and shifted; `phase` makes another scene of it
static std::vector<uint8_t> frame(double turn, double sx, double sy, double phase) {
    std::vector<uint8_t> im((size_t)W * H);
    const double c = std::cos(turn), s = std::sin(turn);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const double dx = x - W / 2, dy = y - H / 2;
            const double u = c * dx - s * dy + sx, v = s * dx + c * dy + sy;
            const double g = 128.0 + 50.0 * std::sin(0.031 * u + 1.3 * std::sin(0.017 * v + phase)) + 45.0 * std::cos(0.027 * v - 0.011 * u + phase) +
                             20.0 * std::sin(0.09 * u + 0.07 * v);
            im[(size_t)y * W + x] = (uint8_t)std::lround(std::fmin(255.0, std::fmax(0.0, g)));
        }
    return im;
}

static void print_frame(const char* tag, const std::vector<uint8_t>& im) {
    for (int y = 0; y < H; y++) {
        std::printf("FRAME %s ", tag);
        for (int x = 0; x < W; x++) std::printf("%02x", im[(size_t)y * W + x]);
        std::printf("\n");
    }
}

static void print_alignment(const char* tag, const ptam_sbi_alignment& a) {
    std::printf("%s %d %d %d", tag, a.n_used, a.iterations_done, a.degenerate);
    for (double v : a.se2_rot) std::printf(" %.17g", v);
    for (double v : a.se2_trans) std::printf(" %.17g", v);
    std::printf(" %.17g %.17g", a.score, a.mean_offset);
    for (double v : a.rotation) std::printf(" %.17g", v);
    std::printf("\n");
}

int main() {
    const std::vector<uint8_t> a = frame(0.0, 0.0, 0.0, 0.0), b = frame(0.03, 6.0, -4.0, 0.0), other = frame(0.0, 0.0, 0.0, 2.0);
    print_frame("A", a);
    print_frame("B", b);
    print_frame("C", other);

    ptam::Context c({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {W, H});
    ptam::KeyFrame kA(c), kB(c), kC(c);
    kA.MakeKeyFrame_Lite(a.data(), W);
    kB.MakeKeyFrame_Lite(b.data(), W);
    kC.MakeKeyFrame_Lite(other.data(), W);

    // the tracker's pair: this frame against the last, blur 0.75
    ptam::SmallBlurryImage last(c, kA, 0.75), now(c, kB, 0.75);
    ptam_sbi_alignment al;
    const std::pair<ptam::SE3, double> rot = now.CalcSBIRotation(&last, 6, &al);
    std::printf("SIZE %d %d\n", now.GetSize().x, now.GetSize().y);
    print_alignment("ALIGN", al);

    // the relocaliser: the other scene first, then the scene the current frame shows
    kC.se3CfromW.t[2] = 1.0;
    kA.se3CfromW.t[0] = 0.25, kA.se3CfromW.t[1] = -0.5, kA.se3CfromW.t[2] = 2.0;
    ptam::Relocaliser reloc(c, 4);
    reloc.AddKeyFrame(kC);
    reloc.AddKeyFrame(kA);
    const bool good = reloc.AttemptRecovery(kB);
    const ptam::SE3 pose = reloc.BestPose();
    std::printf("RELOC %d %d %.17g", reloc.mnBest(), good ? 1 : 0, reloc.mdBestScore());
    for (double v : pose.R) std::printf(" %.17g", v);
    for (double v : pose.t) std::printf(" %.17g", v);
    std::printf("\n");
    print_alignment("RELOC_ALIGN", reloc.Last().align);
    return good && reloc.mnBest() == 1 && rot.second == al.score ? 0 : 1;
}
