// publish_map_demo.cc — the map handed from the mapmaker's thread to the tracker's on the device (ptam_shim.hpp): a ptam::ResidentMap
// in one context, a ptam::MapTracker in another, a ptam::MapSnapshot between them.  The mapmaker thread counts a tracked frame's
// outliers (NoteTracked), runs HandleBadPoints and publishes, carries the new keyframe's rows across the renumbering by their
// serials (PointSerials before, ResolveSerials after), inserts the keyframe and publishes again; the tracker thread meanwhile polls
// TakeMap and tracks a frame per pass until it holds the last generation.  Nothing table-sized crosses the host link on either side.
// At the end a fresh tracker takes the last generation, tracks one frame, and its iteration set goes back to the map's numbering
// through its serials (tests/test_gpu_map_publish_shim.py builds and runs it).
//   in:  the file of examples/insert_keyframe_demo.cc
//   out: int64 generation | int32 n_points, n_removed, n_made, n_rows_kept | n_points int64: the tracker's serials |
//        n_points int64: the map's | int32 n_set | n_set int64: the iteration set's serials | n_set int32: their indices in the map
#include <atomic>
#include <cstdio>
#include <thread>
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
        std::fprintf(stderr, "usage: publish_map_demo <map in> <lists out>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> h;
    std::vector<double> par;
    if (!f || !get(f, h, 8) || !get(f, par, 3)) return 3;
    const size_t K = (size_t)h[0], N = (size_t)h[1];
    const int width = h[5], height = h[6];
    std::vector<uint8_t> im_b, im_c, im_a, fixed, bad;
    std::vector<ptam::SE3> poses, new_pose;
    std::vector<ptam::Vec<3>> points;
    std::vector<ptam_map_refind_point> rpoints;
    std::vector<ptam_map_point_source> sources;
    std::vector<ptam_map_meas> meas;
    std::vector<int32_t> new_queue;
    std::vector<ptam_map_kf_row> rows;
    const size_t px = (size_t)width * height;
    if (!get(f, im_b, px) || !get(f, im_c, px) || !get(f, im_a, px) || !get(f, poses, K) || !get(f, fixed, K) || !get(f, points, N) ||
        !get(f, rpoints, N) || !get(f, sources, N) || !get(f, bad, N) || !get(f, meas, (size_t)h[2]) || !get(f, new_queue, (size_t)h[3]) ||
        !get(f, new_pose, 1) || !get(f, rows, (size_t)h[4]))
        return 3;
    std::fclose(f);
    const ptam::Vec<5> cam{1.0803, 1.43987, 0.519983, 0.548655, 0.244943};
    ptam::Context cm(cam, {width, height}), ct(cam, {width, height});   // the mapmaker's and the tracker's: one queue each
    ptam::KeyFrame kfb(cm), kfc(cm), kfa(cm), cur(ct);
    kfb.MakeKeyFrame_Lite(im_b.data(), width);
    kfc.MakeKeyFrame_Lite(im_c.data(), width);
    kfa.MakeKeyFrame_Lite(im_a.data(), width);
    kfa.MakeKeyFrame_Rest();
    cur.MakeKeyFrame_Lite(im_a.data(), width);
    std::vector<const ptam::KeyFrame*> kfs;
    for (size_t i = 0; i < K; i++) kfs.push_back(i < 2 ? &kfb : &kfc);
    FILE* g = std::fopen(argv[2], "wb");
    if (!g) return 4;
    const int cap = (int)N + 4096;
    int rc = 0;
    {
        ptam::ResidentMap map(cm);
        ptam::ReFinder finder(cm);
        ptam::MapSnapshot snapshot(cm, cap);
        ptam::MapTracker tracker(ct, cap);
        map.Upload(kfs, poses, fixed, points, rpoints, sources, bad, nullptr, nullptr, meas, {}, new_queue, {});
        map.Publish(snapshot);   // generation 1: the tracker has a map to start from
        int32_t n_removed = 0, n_made = 0, n_rows_kept = 0;
        std::atomic<int> failed{0};

        std::thread mapmaker([&] {
            try {
                // every fifth row's point was an outlier in 21 frames: HandleBadPoints removes it and renumbers the rest
                std::vector<int32_t> pts;
                for (size_t i = 0; i < rows.size(); i += 5)
                    for (int k = 0; k < 21; k++) pts.push_back(rows[i].point);
                map.NoteTracked(pts, std::vector<uint8_t>(pts.size(), 1));
                std::vector<int64_t> all = map.PointSerials(), row_serials;
                for (const ptam_map_kf_row& r : rows) row_serials.push_back(all[(size_t)r.point]);
                n_removed = map.HandleBadPoints(false).result.n_removed;
                map.Publish(snapshot);   // generation 2
                // the keyframe's rows in the numbering of now: serial order is index order, so they stay sorted by point
                const std::vector<int32_t> now = map.ResolveSerials(row_serials);
                std::vector<ptam_map_kf_row> kept;
                for (size_t i = 0; i < rows.size(); i++)
                    if (now[i] >= 0) {
                        kept.push_back(rows[i]);
                        kept.back().point = now[i];
                    }
                n_rows_kept = (int32_t)kept.size();
                ptam_rmap_insert_opts opts = ptam::ResidentMap::InsertOpts(par[0], par[1]);
                opts.epipolar.min_shi_tomasi = par[2];
                opts.target_kf = h[7];
                n_made = map.InsertKeyFrame(finder, kfa, new_pose[0], false, kept, opts).n_made;
                map.Publish(snapshot);   // generation 3
            } catch (const std::exception& e) {
                std::fprintf(stderr, "mapmaker: %s\n", e.what());
                failed = 1;
            }
        });
        std::thread tracking([&] {
            try {
                for (int pass = 0; pass < 100000 && !failed; pass++) {
                    const ptam_map_take_result t = tracker.TakeMap(snapshot);   // the per-frame poll: a mutex when nothing changed
                    tracker.TrackMap(cur, new_pose[0]);
                    if (t.generation == 3) break;
                }
            } catch (const std::exception& e) {
                std::fprintf(stderr, "tracker: %s\n", e.what());
                failed = 1;
            }
        });
        mapmaker.join();
        tracking.join();
        if (failed) rc = 5;

        if (!rc) {
            const ptam_map_take_result last = tracker.TakeMap(snapshot);
            const std::vector<int64_t> theirs = tracker.PointSerials(last.n_points), ours = map.PointSerials();
            // a fresh tracker on the last generation: one frame, and its iteration set in the map's numbering
            ptam::MapTracker fresh(ct, cap);
            const ptam_map_take_result t = fresh.TakeMap(snapshot);
            fresh.TrackMap(cur, new_pose[0]);
            const std::vector<int64_t> set = fresh.IterationSerials();
            const std::vector<int32_t> idx = map.ResolveSerials(set);
            const int64_t generation = last.generation;
            const int32_t counts[4] = {last.n_points, n_removed, n_made, n_rows_kept}, n_set = (int32_t)set.size();
            std::fwrite(&generation, sizeof generation, 1, g);
            std::fwrite(counts, sizeof counts, 1, g);
            put(g, theirs);
            put(g, ours);
            std::fwrite(&n_set, sizeof n_set, 1, g);
            put(g, set);
            put(g, idx);
            std::printf("PUBLISHMAP generation %lld points %d removed %d made %d rows %d new-to-fresh %d set %d same-lists %d\n", (long long)generation,
                        last.n_points, n_removed, n_made, n_rows_kept, t.n_new, n_set, (int)(theirs == ours));
        }
    }
    std::fclose(g);
    return rc;
}
