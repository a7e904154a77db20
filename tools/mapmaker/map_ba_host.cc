// map_ba_host.cc — the host side that ptam_map_bundle_adjust replaces, restated in plain C++ for timing: MapMaker::BundleAdjustAll /
// BundleAdjustRecent and the marshalling half of BundleAdjust (src/MapMaker.cc:768-882) with the reference's containers —
// std::set<KeyFrame*> / std::set<MapPoint*>, the four translation std::maps, std::map<MapPoint*, Measurement> per keyframe — over
// the same tables as the device call.  Bundle::AddCamera / AddPoint / AddMeas become appends to the arrays the bulk Add* calls take.
// Build: g++ -O2 -std=c++17 map_ba_host.cc -o map_ba_host (tools/mapmaker/time_map_ba.py does).  One thread.
//   map_ba_host <tables> <reps>   tables: int32 mode, K, N, M | K x 12 doubles | K bytes bFixed | N x 3 doubles | M x 32-byte rows
//   prints: HOST <mode> median_ms min_ms cameras points measurements
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <vector>

struct MapPoint {
    double v3WorldPos[3];
};
struct Measurement {
    int nLevel, Source;
    double v2RootPos[2];
};
struct KeyFrame {
    double se3CfromW[12];
    bool bFixed;
    std::map<MapPoint*, Measurement> mMeasurements;
};
struct Row {
    int32_t kf, point, level, source;
    double root[2];
};
struct Added {   // what Bundle::Add* would receive, in call order
    std::vector<double> cam_pose, pts, found, sig;
    std::vector<uint8_t> cam_fixed;
    std::vector<int32_t> cam, pt;
};

static void centre(const double* P, double c[3]) {
    for (int i = 0; i < 3; i++) c[i] = -(P[i] * P[9] + P[3 + i] * P[10] + P[6 + i] * P[11]);
}
static double dist(const KeyFrame& a, const KeyFrame& b) {   // :696-703
    double ca[3], cb[3];
    centre(a.se3CfromW, ca);
    centre(b.se3CfromW, cb);
    const double d[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]};
    return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

static void bundle_adjust_marshal(std::vector<KeyFrame*>& vpKeyFrames, const std::set<KeyFrame*>& sAdjustSet,
                                  const std::set<KeyFrame*>& sFixedSet, const std::set<MapPoint*>& sMapPoints, Added& b) {
    std::map<MapPoint*, int> mPoint_BundleID;   // :846-849
    std::map<int, MapPoint*> mBundleID_Point;
    std::map<KeyFrame*, int> mView_BundleID;
    std::map<int, KeyFrame*> mBundleID_View;
    int nc = 0, np = 0;
    for (KeyFrame* it : sAdjustSet) {   // :852-861
        b.cam_pose.insert(b.cam_pose.end(), it->se3CfromW, it->se3CfromW + 12);
        b.cam_fixed.push_back(it->bFixed);
        mView_BundleID[it] = nc;
        mBundleID_View[nc++] = it;
    }
    for (KeyFrame* it : sFixedSet) {
        b.cam_pose.insert(b.cam_pose.end(), it->se3CfromW, it->se3CfromW + 12);
        b.cam_fixed.push_back(1);
        mView_BundleID[it] = nc;
        mBundleID_View[nc++] = it;
    }
    for (MapPoint* p : sMapPoints) {   // :864-868
        b.pts.insert(b.pts.end(), p->v3WorldPos, p->v3WorldPos + 3);
        mPoint_BundleID[p] = np;
        mBundleID_Point[np++] = p;
    }
    for (KeyFrame* kf : vpKeyFrames) {   // :871-882
        if (mView_BundleID.count(kf) == 0) continue;
        const int nKF = mView_BundleID[kf];
        for (auto& m : kf->mMeasurements) {
            if (mPoint_BundleID.count(m.first) == 0) continue;
            b.cam.push_back(nKF);
            b.pt.push_back(mPoint_BundleID[m.first]);
            b.found.push_back(m.second.v2RootPos[0]);
            b.found.push_back(m.second.v2RootPos[1]);
            const int ls = 1 << m.second.nLevel;
            b.sig.push_back((double)(ls * ls));
        }
    }
}

static void recent(std::vector<KeyFrame*>& kfs, Added& b) {   // :788-828
    if (kfs.size() < 8) return;
    std::set<KeyFrame*> sAdjustSet;
    KeyFrame* pkfNewest = kfs.back();
    sAdjustSet.insert(pkfNewest);
    std::vector<std::pair<double, KeyFrame*>> v;   // NClosestKeyFrames :711-730
    for (KeyFrame* k : kfs)
        if (k != pkfNewest) v.emplace_back(dist(*pkfNewest, *k), k);
    std::partial_sort(v.begin(), v.begin() + 4, v.end());
    for (int i = 0; i < 4; i++)
        if (!v[(size_t)i].second->bFixed) sAdjustSet.insert(v[(size_t)i].second);
    std::set<MapPoint*> sMapPoints;
    for (KeyFrame* k : sAdjustSet)
        for (auto& m : k->mMeasurements) sMapPoints.insert(m.first);
    std::set<KeyFrame*> sFixedSet;
    for (KeyFrame* k : kfs) {
        if (sAdjustSet.count(k)) continue;
        for (auto& m : k->mMeasurements)
            if (sMapPoints.count(m.first)) {
                sFixedSet.insert(k);
                break;
            }
    }
    bundle_adjust_marshal(kfs, sAdjustSet, sFixedSet, sMapPoints, b);
}

static void all(std::vector<KeyFrame*>& kfs, std::vector<MapPoint>& pts, Added& b) {   // :768-783
    std::set<KeyFrame*> sAdj, sFixed;
    for (KeyFrame* k : kfs) (k->bFixed ? sFixed : sAdj).insert(k);
    std::set<MapPoint*> sMapPoints;
    for (MapPoint& p : pts) sMapPoints.insert(&p);
    bundle_adjust_marshal(kfs, sAdj, sFixed, sMapPoints, b);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int32_t h[4];
    if (!f || std::fread(h, 4, 4, f) != 4) return 3;
    const int mode = h[0], K = h[1], N = h[2], M = h[3], reps = std::atoi(argv[2]);
    std::vector<KeyFrame> kf((size_t)K);   // (contiguous: pointer order = index order, as the device call assumes)
    std::vector<MapPoint> mp((size_t)N);
    std::vector<uint8_t> fixed((size_t)K);
    std::vector<Row> rows((size_t)M);
    for (auto& k : kf)
        if (std::fread(k.se3CfromW, 8, 12, f) != 12) return 3;
    if (K && std::fread(fixed.data(), 1, (size_t)K, f) != (size_t)K) return 3;
    for (auto& p : mp)
        if (std::fread(p.v3WorldPos, 8, 3, f) != 3) return 3;
    if (M && std::fread(rows.data(), sizeof(Row), (size_t)M, f) != (size_t)M) return 3;
    std::fclose(f);
    for (int k = 0; k < K; k++) kf[(size_t)k].bFixed = fixed[(size_t)k] != 0;
    for (const Row& r : rows) kf[(size_t)r.kf].mMeasurements[&mp[(size_t)r.point]] = Measurement{r.level, r.source, {r.root[0], r.root[1]}};
    std::vector<KeyFrame*> vpKeyFrames;
    for (auto& k : kf) vpKeyFrames.push_back(&k);
    std::vector<double> t;
    Added last;
    for (int r = 0; r < reps; r++) {
        Added b;
        const auto t0 = std::chrono::steady_clock::now();
        if (mode == 1)
            recent(vpKeyFrames, b);
        else
            all(vpKeyFrames, mp, b);
        t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (r == reps - 1) last = std::move(b);
    }
    std::sort(t.begin(), t.end());
    std::printf("HOST %d %.4f %.4f %zu %zu %zu\n", mode, t[t.size() / 2], t[0], last.cam_fixed.size(), last.pts.size() / 3, last.cam.size());
    return 0;
}
