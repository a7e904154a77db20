// publish_keyframes_demo.cc — the map's keyframes handed to the relocaliser on the device (ptam_shim.hpp): a ptam::ResidentMap in the
// mapmaker's context, a ptam::MapTracker and a ptam::Relocaliser in the tracker's, one ptam::MapSnapshot with its keyframe section
// enabled between them.  The mapmaker's thread inserts a second keyframe (InsertKeyFrame) and publishes, moves the whole map
// (ApplyGlobalTransformationToMap, which changes every keyframe's pose) and publishes again.  The tracker's thread starts LOST: per
// pass it polls TakeMap and TakeKeyFrames and runs one frame through TrackFramesRecoverBatch, whose relocaliser sees only what the
// takes brought — no keyframe handle and no pose table is carried between the threads by the host.  At the end the bank's poses
// and images and the map's own pose table are printed (tests/test_gpu_keyframe_publish_shim.py builds and runs it and fills a
// bank by hand from the printed frames).
//   g++ -O2 -std=c++17 -pthread -Iinclude examples/publish_keyframes_demo.cc -Lptam_cg_amd/csrc -lptam_hip -Wl,-rpath,$PWD/ptam_cg_amd/csrc
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "ptam_shim.hpp"

static const int W = 160, H = 120, FRAMES = 4;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the blocky synthetic scene of track_recover_demo.cc, seen shifted by (dx, dy) pixels
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

static void print_hex(const char* tag, int a, const void* p, size_t n) {
    std::printf("%s %d ", tag, a);
    for (size_t i = 0; i < n; i++) std::printf("%02x", ((const uint8_t*)p)[i]);
    std::printf("\n");
}

static void unit(const double v[3], double out[3]) {
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 3; i++) out[i] = v[i] / n;
}

int main() {
    std::vector<std::vector<uint8_t>> ims;
    for (int f = 0; f < FRAMES; f++) {
        ims.push_back(frame(f, -(f / 2)));
        print_hex("FRAME", f, ims.back().data(), ims.back().size());
    }
    const ptam::Vec<5> cam{1.0803, 1.43987, 0.519983, 0.548655, 0.244943};
    ptam::Context cm(cam, {W, H}), ct(cam, {W, H});   // the mapmaker's and the tracker's: one queue each
    ptam::KeyFrame kf0(cm), kf1(cm), current(ct);
    kf0.MakeKeyFrame_Lite(ims[0].data(), W);
    kf1.MakeKeyFrame_Lite(ims[3].data(), W);
    kf1.MakeKeyFrame_Rest();
    // the toy map of shim_demo.cc as map tables: level-0 corners of frame 0 near the image centre, back-projected to Z = 1, seen from
    // the identity, each measured once in keyframe 0
    double cc[8];
    ptam::check(ptam_ctx_camera_constants(cm.handle(), cc), "ptam_ctx_camera_constants");
    std::vector<ptam::Vec<3>> points;
    std::vector<ptam_map_refind_point> rpoints;
    std::vector<ptam_map_point_source> sources;
    std::vector<ptam_map_meas> meas;
    std::vector<ptam_map_kf_row> rows;   // the second keyframe's measurements: the same corners, three pixels to the right
    for (auto& c : kf0.aLevels(0).vCorners) {
        if (!(c.x >= 20 && c.y >= 20 && c.x < 140 && c.y < 100)) continue;
        const double x = (c.x - cc[2]) / cc[0], y = (c.y - cc[3]) / cc[1];
        if (std::sqrt(x * x + y * y) > 0.12) continue;
        const int i = (int)points.size();
        ptam_map_refind_point p{};
        p.pv.world[0] = x, p.pv.world[1] = y, p.pv.world[2] = 1.0;
        p.pv.pixel_right_w[0] = 1.0 / cc[0];
        p.pv.pixel_down_w[1] = 1.0 / cc[1];
        p.src_kf = 0, p.src_level = 0, p.center_x = c.x, p.center_y = c.y;
        ptam_map_point_source s{};
        const double centre[3] = {x, y, 1.0}, right[3] = {x + 1.0 / cc[0], y, 1.0}, down[3] = {x, y + 1.0 / cc[1], 1.0};
        unit(centre, s.center_nc);
        unit(right, s.one_right_nc);
        unit(down, s.one_down_nc);
        ptam_map_meas m{};
        m.kf = 0, m.point = i, m.level = 0, m.source = PTAM_MAP_SRC_ROOT;
        m.root_pos[0] = c.x, m.root_pos[1] = c.y;
        ptam_map_kf_row r{};
        r.point = i, r.level = 0;
        r.root_pos[0] = c.x + 3.0, r.root_pos[1] = c.y - 1.0;
        points.push_back({x, y, 1.0});
        rpoints.push_back(p);
        sources.push_back(s);
        meas.push_back(m);
        rows.push_back(r);
    }
    const int N = (int)points.size(), cap = N + 4096;
    ptam::SE3 second = ptam::SE3::Identity(), shift = ptam::SE3::Identity();
    second.t[0] = 0.02;
    shift.t[0] = 0.05, shift.t[1] = -0.01, shift.t[2] = 0.02;
    int rc = 0;
    {
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        snapshot.EnableKeyFrames(8);
        ptam::MapTracker tracker(ct, cap);
        ptam::Relocaliser relocaliser(ct, 8);
        ptam::RotationEstimator estimator(ct);
        map.Upload({&kf0}, {ptam::SE3::Identity()}, {1}, points, rpoints, sources, std::vector<uint8_t>((size_t)N, 0), nullptr, nullptr, meas, {}, {}, {});
        map.Publish(snapshot);   // generation 1: one keyframe, made into the slot's bank layout by the publish itself
        std::atomic<int> failed{0};
        int n_made = 0, branches[3] = {0, 0, 0}, takes = 0, last_best = -1;
        long long generation = 0;

        std::thread mapmaker([&] {
            try {
                ptam_rmap_insert_opts opts = ptam::ResidentMap::InsertOpts(1.0, 0.2);
                n_made = map.InsertKeyFrame(finder, kf1, second, false, rows, opts).n_made;
                map.Publish(snapshot);   // generation 2: the second keyframe's pose and image ride on the publish
                map.ApplyGlobalTransformationToMap(shift, false);
                map.Publish(snapshot);   // generation 3: both poses moved; no image is made for the slot that holds them already
            } catch (const std::exception& e) {
                std::fprintf(stderr, "mapmaker: %s\n", e.what());
                failed = 1;
            }
        });
        std::thread tracking([&] {
            try {
                void* d_frame = nullptr;
                ptam::check(ptam_dev_alloc(ct.handle(), ims[3].size(), &d_frame), "ptam_dev_alloc");
                ptam::check(ptam_dev_upload(ct.handle(), d_frame, ims[3].data(), ims[3].size()), "ptam_dev_upload");
                std::vector<ptam::TrackState> states(1);
                states[0].lost_frames = 3;   // lost from the start: the first frame goes through Relocaliser::AttemptRecovery
                states[0].quality = PTAM_TRACK_BAD;
                for (int pass = 0; pass < 100000 && !failed; pass++) {
                    const ptam_map_take_result tm = tracker.TakeMap(snapshot);              // the per-frame polls: a mutex hold each
                    const ptam_keyframes_take_result tk = relocaliser.TakeKeyFrames(snapshot);   // when nothing changed
                    takes += tk.changed;
                    std::vector<ptam_track_frame_state_info> vInfo;
                    ptam::MapTracker::TrackFramesRecoverBatch({&tracker}, {&current}, {(const uint8_t*)d_frame}, states, {&estimator}, {&relocaliser}, vInfo);
                    branches[vInfo[0].branch]++;
                    if (vInfo[0].branch == PTAM_FRAME_RECOVERED) last_best = vInfo[0].reloc.best;
                    if (vInfo[0].want_keyframe) states[0].KeyFrameAdded();
                    generation = tk.generation;
                    if (tm.generation == 3 && tk.generation == 3) break;
                }
                ptam_dev_free(ct.handle(), d_frame);
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
            }
        });
        mapmaker.join();
        tracking.join();
        if (failed) rc = 5;
        if (!rc) {
            const ptam_snapshot_keyframes_info_t info = snapshot.KeyFrames();
            const int n = relocaliser.KeyFrameCount();
            const std::vector<ptam::SE3> poses = map.Download<ptam::SE3>(PTAM_RMAP_KF_POSES);
            for (size_t i = 0; i < poses.size(); i++) print_hex("KFPOSE", (int)i, &poses[i], sizeof poses[i]);
            const size_t px = (size_t)info.sbi_w * info.sbi_h;
            for (int i = 0; i < n; i++) {
                const ptam::SE3 p = relocaliser.KeyFramePose(i);
                print_hex("BANKPOSE", i, &p, sizeof p);
                std::vector<uint8_t> small(px);
                std::vector<float> tmpl(px), jacs(2 * px);
                ptam::check(ptam_sbi_bank_read(relocaliser.handle(), i, small.data(), tmpl.data(), jacs.data()), "ptam_sbi_bank_read");
                print_hex("SMALL", i, small.data(), px);
                print_hex("TMPL", i, tmpl.data(), 4 * px);
                print_hex("JACS", i, jacs.data(), 8 * px);
            }
            std::printf("PUBLISHKEYFRAMES generation %lld keyframes %d bank %d made %d takes %d tracked %d recovered %d failed %d best %d sbi %d %d\n",
                        generation, info.n_kf, n, n_made, takes, branches[PTAM_FRAME_TRACKED], branches[PTAM_FRAME_RECOVERED],
                        branches[PTAM_FRAME_RECOVERY_FAILED], last_best, info.sbi_w, info.sbi_h);
            if (generation != 3 || n != 2 || info.n_kf != 2 || branches[PTAM_FRAME_RECOVERED] < 1) rc = 6;
        }
    }
    return rc;
}
