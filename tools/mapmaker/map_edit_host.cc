// map_edit_host.cc — the host work that ptam_map_apply_outliers / ptam_map_handle_bad_points / ptam_map_add_points replace, restated
// in plain C++ for timing with containers shaped like the reference's: std::map<MapPoint*, Measurement> per keyframe, the two
// std::set<KeyFrame*> per point, vpPoints / mvFailureQueue as vectors, mqNewQueue as a queue — the outlier loop of
// src/MapMaker.cc:916-932, HandleBadPoints :131-153 with Map::MoveBadPointsToTrash (src/Map.cc:20-30), and the table side of
// AddPointEpipolar :670-685.  The map is built from the tables outside the clock, once per repetition.
// Build: g++ -O2 -std=c++17 map_edit_host.cc -o map_edit_host (tools/mapmaker/time_map_edit.py does).  One thread.
//   map_edit_host <tables> <reps>   tables: the input file of examples/map_edit_demo.cc
//   prints: HOST outliers_ms bad_points_ms add_points_ms (medians) removed rows_after
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <queue>
#include <set>
#include <vector>

struct KeyFrame;
struct MapPoint {
    bool bBad = false;
    int nMEstimatorOutlierCount = 0, nMEstimatorInlierCount = 0;
    std::set<KeyFrame*> sMeasurementKFs, sNeverRetryKFs;
    double v3WorldPos[3];
};
struct Measurement {
    int nLevel, Source;
    double v2RootPos[2];
};
struct KeyFrame {
    std::map<MapPoint*, Measurement> mMeasurements;
};
struct Row {
    int32_t kf, point, level, source;
    double root[2];
};
struct Pair {
    int32_t kf, point;
};
struct Outlier {
    int32_t point, kf, action, meas;
};
struct Made {
    double pv[9], nc[9], src_root[2], target[2];
    int32_t level, cx, cy, candidate, corner, zmssd;
};
enum { SRC_TRACKER = 0, SRC_REFIND = 1, SRC_ROOT = 2, SRC_TRAIL = 3, SRC_EPIPOLAR = 4 };

struct Map {
    std::vector<KeyFrame*> vpKeyFrames;
    std::vector<MapPoint*> vpPoints, vpPointsTrash;
    std::queue<MapPoint*> mqNewQueue;
    std::vector<std::pair<KeyFrame*, MapPoint*>> mvFailureQueue;
    ~Map() {
        for (KeyFrame* k : vpKeyFrames) delete k;
        for (MapPoint* p : vpPoints) delete p;
        for (MapPoint* p : vpPointsTrash) delete p;
    }
};

template <class T>
static bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    std::vector<int32_t> h, n_out, n_in, new_queue;
    if (!f || !get(f, h, 12)) return 3;
    const int K = h[0], N = h[1], reps = std::atoi(argv[2]);
    std::vector<uint8_t> bad;
    std::vector<Row> meas;
    std::vector<Pair> never, failure;
    std::vector<Outlier> outliers;
    std::vector<Made> made;
    if (!get(f, bad, (size_t)N) || !get(f, n_out, (size_t)N) || !get(f, n_in, (size_t)N) || !get(f, meas, (size_t)h[2]) ||
        !get(f, never, (size_t)h[3]) || !get(f, new_queue, (size_t)h[4]) || !get(f, failure, (size_t)h[5]) || !get(f, outliers, (size_t)h[6]) ||
        !get(f, made, (size_t)h[7]))
        return 3;
    std::fclose(f);
    std::vector<double> t_out, t_bad, t_add;
    size_t removed = 0, rows = 0;
    for (int rep = 0; rep < reps; rep++) {
        Map m;
        for (int k = 0; k < K; k++) m.vpKeyFrames.push_back(new KeyFrame);
        for (int i = 0; i < N; i++) {
            MapPoint* p = new MapPoint;
            p->bBad = bad[(size_t)i] != 0;
            p->nMEstimatorOutlierCount = n_out[(size_t)i];
            p->nMEstimatorInlierCount = n_in[(size_t)i];
            m.vpPoints.push_back(p);
        }
        for (const Row& r : meas) {
            m.vpKeyFrames[(size_t)r.kf]->mMeasurements[m.vpPoints[(size_t)r.point]] = Measurement{r.level, r.source, {r.root[0], r.root[1]}};
            m.vpPoints[(size_t)r.point]->sMeasurementKFs.insert(m.vpKeyFrames[(size_t)r.kf]);
        }
        for (const Pair& q : never) m.vpPoints[(size_t)q.point]->sNeverRetryKFs.insert(m.vpKeyFrames[(size_t)q.kf]);
        for (int32_t i : new_queue) m.mqNewQueue.push(m.vpPoints[(size_t)i]);
        for (const Pair& q : failure) m.mvFailureQueue.emplace_back(m.vpKeyFrames[(size_t)q.kf], m.vpPoints[(size_t)q.point]);
        std::vector<std::pair<MapPoint*, KeyFrame*>> vOutliers;   // GetOutlierMeasurements through the two id maps
        for (const Outlier& o : outliers) vOutliers.emplace_back(m.vpPoints[(size_t)o.point], m.vpKeyFrames[(size_t)o.kf]);
        KeyFrame &kSrc = *m.vpKeyFrames[(size_t)h[8]], &kTarget = *m.vpKeyFrames[(size_t)h[9]];

        const auto t0 = std::chrono::steady_clock::now();
        for (auto& i : vOutliers) {   // :917-932
            MapPoint* pp = i.first;
            KeyFrame* pk = i.second;
            Measurement& mm = pk->mMeasurements[pp];
            if (pp->sMeasurementKFs.size() <= 2 || mm.Source == SRC_ROOT)
                pp->bBad = true;
            else {
                if (mm.Source == SRC_TRACKER || mm.Source == SRC_EPIPOLAR)
                    m.mvFailureQueue.emplace_back(pk, pp);
                else
                    pp->sNeverRetryKFs.insert(pk);
                pk->mMeasurements.erase(pp);
                pp->sMeasurementKFs.erase(pk);
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        for (MapPoint* p : m.vpPoints)   // :134-138
            if (p->nMEstimatorOutlierCount > 20 && p->nMEstimatorOutlierCount > p->nMEstimatorInlierCount) p->bBad = true;
        for (MapPoint* p : m.vpPoints)   // :142-151
            if (p->bBad)
                for (KeyFrame* k : m.vpKeyFrames)
                    if (k->mMeasurements.count(p)) k->mMeasurements.erase(p);
        for (int i = (int)m.vpPoints.size() - 1; i >= 0; i--)   // Map.cc:23-29
            if (m.vpPoints[(size_t)i]->bBad) {
                m.vpPointsTrash.push_back(m.vpPoints[(size_t)i]);
                m.vpPoints.erase(m.vpPoints.begin() + i);
            }
        const auto t2 = std::chrono::steady_clock::now();
        for (const Made& r : made) {   // :651-685
            MapPoint* pNew = new MapPoint;
            for (int j = 0; j < 3; j++) pNew->v3WorldPos[j] = r.pv[j];
            m.vpPoints.push_back(pNew);
            m.mqNewQueue.push(pNew);
            Measurement mm{r.level, SRC_ROOT, {r.src_root[0], r.src_root[1]}};
            kSrc.mMeasurements[pNew] = mm;
            mm.Source = h[10];
            mm.v2RootPos[0] = r.target[0];
            mm.v2RootPos[1] = r.target[1];
            kTarget.mMeasurements[pNew] = mm;
            pNew->sMeasurementKFs.insert(&kSrc);
            pNew->sMeasurementKFs.insert(&kTarget);
        }
        const auto t3 = std::chrono::steady_clock::now();
        t_out.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        t_bad.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
        t_add.push_back(std::chrono::duration<double, std::milli>(t3 - t2).count());
        removed = m.vpPointsTrash.size();
        rows = 0;
        for (KeyFrame* k : m.vpKeyFrames) rows += k->mMeasurements.size();
    }
    std::printf("HOST %.3f %.3f %.3f %zu %zu\n", median(t_out), median(t_bad), median(t_add), removed, rows);
    return 0;
}
