// track_recover_demo.cc — ptam::MapTracker::TrackFramesRecoverBatch (ptam_shim.hpp): Tracker::TrackFrame for a good map, for three
// cameras on one device in one chain of launches per round.  Camera 0 tracks throughout; cameras 1 (no rotation estimator) and 2 are
// lost from the start: in the first half of the rounds no keyframe is acceptable (Reloc2.MaxScore = 0) and their recovery fails, in
// round 2 they recover in the call in which camera 0 tracks, and in round 3 all three track.  Every camera has its own relocaliser with
// two keyframes.  The frames, the toy map and, per round and camera, the result, the info and the state are printed
// (tests/test_gpu_track_recover_shim.py builds and runs it and feeds the same frames and map through the Python binding).
//   g++ -O2 -std=c++17 -Iinclude examples/track_recover_demo.cc -Lptam_cg_amd/csrc -lptam_hip -Wl,-rpath,$PWD/ptam_cg_amd/csrc
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "ptam_shim.hpp"

static const int W = 160, H = 120, FRAMES = 4, ROUNDS = 4, CAMERAS = 3;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// a blocky synthetic scene, seen shifted by (dx, dy) pixels
static std::vector<uint8_t> frame(int dx, int dy) {
    std::vector<uint8_t> im((size_t)W * H, 128);
    uint32_t s = 12345;
    for (int k = 0; k < 40; k++) {
        const int x0 = (int)(lcg(s) % 150) + dx, y0 = (int)(lcg(s) % 110) + dy, w = 8 + (int)(lcg(s) % 40), h = 8 + (int)(lcg(s) % 40), v = 30 + (int)(lcg(s) % 190);
        for (int y = std::max(y0, 0); y < y0 + h && y < H; y++)
            for (int x = std::max(x0, 0); x < x0 + w && x < W; x++) im[(size_t)y * W + x] = (uint8_t)v;
    }
    return im;
}

static void print_hex(const char* tag, int a, int b, const void* p, size_t n) {
    std::printf("%s %d %d ", tag, a, b);
    for (size_t i = 0; i < n; i++) std::printf("%02x", ((const uint8_t*)p)[i]);
    std::printf("\n");
}

struct Camera {
    ptam::Context ctx;
    ptam::KeyFrame source, second, current;
    ptam::MapTracker tracker;
    ptam::Relocaliser relocaliser;
    std::unique_ptr<ptam::RotationEstimator> estimator;
    std::vector<void*> frames;
    Camera(const std::vector<std::vector<uint8_t>>& ims, const std::vector<ptam_pvs_point>& pts, std::vector<ptam_template_query> src, bool with_estimator)
        : ctx({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {W, H}), source(ctx), second(ctx), current(ctx), tracker(ctx, (int)pts.size() + 1),
          relocaliser(ctx, 4) {
        source.MakeKeyFrame_Lite(ims[0].data(), W);
        second.MakeKeyFrame_Lite(ims[3].data(), W);
        for (auto& q : src) q.src_kf = source.handle();
        tracker.SetMap(pts, src);
        // the map's keyframes: frame 0 at the identity, frame 3 a little to its side (SetKeyFramePose: as after a bundle adjustment)
        relocaliser.AddKeyFrames({&source, &second});
        ptam::SE3 moved = ptam::SE3::Identity();
        moved.t[0] = 0.02;
        relocaliser.SetKeyFramePose(1, moved);
        if (with_estimator) estimator.reset(new ptam::RotationEstimator(ctx));
        for (auto& im : ims) {
            void* d = nullptr;
            ptam::check(ptam_dev_alloc(ctx.handle(), im.size(), &d), "ptam_dev_alloc");
            ptam::check(ptam_dev_upload(ctx.handle(), d, im.data(), im.size()), "ptam_dev_upload");
            frames.push_back(d);
        }
    }
    ~Camera() {
        for (void* d : frames) ptam_dev_free(ctx.handle(), d);
    }
};

int main() {
    std::vector<std::vector<uint8_t>> ims;
    for (int f = 0; f < FRAMES; f++) {
        ims.push_back(frame(f, -(f / 2)));
        print_hex("FRAME", f, 0, ims.back().data(), ims.back().size());
    }
    // the toy map of shim_demo.cc: level-0 corners of frame 0 near the image centre, back-projected to Z = 1, seen from the identity
    std::vector<ptam_pvs_point> pts;
    std::vector<ptam_template_query> src;
    {
        ptam::Context ctx({1.0803, 1.43987, 0.519983, 0.548655, 0.244943}, {W, H});
        ptam::KeyFrame kf(ctx);
        kf.MakeKeyFrame_Lite(ims[0].data(), W);
        double cc[8];
        ptam::check(ptam_ctx_camera_constants(ctx.handle(), cc), "ptam_ctx_camera_constants");
        for (auto& c : kf.aLevels(0).vCorners) {
            if (!(c.x >= 20 && c.y >= 20 && c.x < 140 && c.y < 100)) continue;
            const double x = (c.x - cc[2]) / cc[0], y = (c.y - cc[3]) / cc[1];
            if (std::sqrt(x * x + y * y) > 0.12) continue;
            ptam_pvs_point p{};
            p.world[0] = x, p.world[1] = y, p.world[2] = 1.0;
            p.pixel_right_w[0] = 1.0 / cc[0];
            p.pixel_down_w[1] = 1.0 / cc[1];
            pts.push_back(p);
            ptam_template_query q{};
            q.src_level = 0;
            q.center_x = c.x, q.center_y = c.y;
            src.push_back(q);
            print_hex("POINT", q.center_x, q.center_y, &p, sizeof p);
        }
    }
    std::vector<std::unique_ptr<Camera>> cams;
    for (int i = 0; i < CAMERAS; i++) cams.emplace_back(new Camera(ims, pts, src, i != 1));
    std::vector<ptam::TrackState> states((size_t)CAMERAS);
    states[1].lost_frames = states[2].lost_frames = 3;
    states[1].quality = states[2].quality = PTAM_TRACK_BAD;
    int ok = 1;
    for (int r = 0; r < ROUNDS; r++) {
        std::vector<ptam::MapTracker*> vT;
        std::vector<ptam::KeyFrame*> vK;
        std::vector<const uint8_t*> vF;
        std::vector<ptam::RotationEstimator*> vE;
        std::vector<ptam::Relocaliser*> vR;
        for (int i = 0; i < CAMERAS; i++) {
            vT.push_back(&cams[i]->tracker);
            vK.push_back(&cams[i]->current);
            vF.push_back((const uint8_t*)cams[i]->frames[(size_t)(r % FRAMES)]);
            vE.push_back(cams[i]->estimator.get());
            vR.push_back(&cams[i]->relocaliser);
        }
        ptam_track_state_opts so;
        ptam_track_state_opts_default(&so);
        if (r < ROUNDS / 2) so.reloc_max_score = 0.0;   // nothing scores below 0: whoever is lost stays lost
        std::vector<ptam_track_frame_state_info> vInfo;
        const std::vector<ptam_trackmap_result> res = ptam::MapTracker::TrackFramesRecoverBatch(vT, vK, vF, states, vE, vR, vInfo, nullptr, &so);
        for (int i = 0; i < CAMERAS; i++) {
            const ptam_track_frame_state_info& fi = vInfo[(size_t)i];
            print_hex("RESULT", r, i, &res[(size_t)i], sizeof(ptam_trackmap_result));
            print_hex("INFO", r, i, &fi, sizeof fi);
            print_hex("STATE", r, i, static_cast<const ptam_track_state*>(&states[(size_t)i]), sizeof(ptam_track_state));
            std::printf("SUMMARY %d %d branch %d n_meas %d quality %d lost %d frame %d best %d closest %d want_keyframe %d\n", r, i, fi.branch,
                        res[(size_t)i].n_meas, states[(size_t)i].quality, states[(size_t)i].lost_frames, states[(size_t)i].frame, fi.reloc.best,
                        fi.closest_kf, fi.want_keyframe);
            ok &= states[(size_t)i].frame == r + 1;
            if (fi.branch != PTAM_FRAME_RECOVERY_FAILED) ok &= std::memcmp(states[(size_t)i].model.pose, res[(size_t)i].pose, sizeof res[(size_t)i].pose) == 0;
            if (fi.want_keyframe) states[(size_t)i].KeyFrameAdded();   // (a map maker with room in its queue, :149-165)
        }
        ok &= cams[1]->relocaliser.KeyFramePose(1).t[0] == 0.02;
    }
    return ok ? 0 : 1;
}
