// map_refind_host.cc — the host side that ptam_map_refind replaces, restated in plain C++ for timing: the loops of
// MapMaker::ReFindInSingleKeyFrame / ReFindNewlyMade / ReFindFromFailureQueue (src/MapMaker.cc:1028-1081) with the reference's
// containers — std::set<KeyFrame*> sMeasurementKFs / sNeverRetryKFs per point, std::map<MapPoint*, Measurement> per keyframe —
// doing the set tests of :947-948 and filling one ptam_refind_pair per pair for ptam_refind_pairs; and what follows that call:
// the results folded back into the sets (:953-1018) and the sorted (kf, point) table rebuilt for the next table call.
// Build: g++ -O2 -std=c++17 -shared -fPIC -I include map_refind_host.cc -o libmap_refind_host.so (tools/mapmaker/time_map_refind.py
// does, and loads it beside the product library).  One thread.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "ptam_hip.h"

struct KeyFrame;
struct MapPoint {
    ptam_map_refind_point p;
    std::set<KeyFrame*> sMeasurementKFs, sNeverRetryKFs;
};
struct Measurement {
    int nLevel, Source;
    double v2RootPos[2];
};
struct KeyFrame {
    const ptam_kf* dev;
    double se3CfromW[12];
    std::map<MapPoint*, Measurement> mMeasurements;
};
struct Map {   // (contiguous: pointer order = index order, as the device call assumes)
    std::vector<KeyFrame> kfs;
    std::vector<MapPoint> pts;
};

static std::vector<ptam_refind_pair> g_pairs;   // the pair list of the last mrh_pairs
static std::vector<KeyFrame*> g_kf;             // ... and each pair's keyframe, as the host's loop has it at hand
static void fill(const Map& m, KeyFrame& k, MapPoint& p, std::vector<ptam_refind_pair>& out) {
    ptam_refind_pair r;
    std::memset(&r, 0, sizeof r);
    r.kf = k.dev;
    std::memcpy(r.kf_pose, k.se3CfromW, sizeof r.kf_pose);
    r.point = p.p.pv;
    r.source.src_kf = m.kfs[(size_t)p.p.src_kf].dev;
    r.source.src_level = p.p.src_level;
    r.source.center_x = p.p.center_x;
    r.source.center_y = p.p.center_y;
    r.point_id = &p - m.pts.data();
    r.skip = p.sMeasurementKFs.count(&k) || p.sNeverRetryKFs.count(&k);   // :947-948
    out.push_back(r);
    g_kf.push_back(&k);
}

extern "C" {

void* mrh_create(int n_kf, const ptam_kf* const* kfs, const double* poses, int n_points, const ptam_map_refind_point* points, int n_meas,
                 const ptam_map_meas* meas, int n_never, const ptam_map_pair* never) {
    Map* m = new Map;
    m->kfs.resize((size_t)n_kf);
    m->pts.resize((size_t)n_points);
    for (int k = 0; k < n_kf; k++) {
        m->kfs[(size_t)k].dev = kfs[k];
        std::memcpy(m->kfs[(size_t)k].se3CfromW, poses + 12 * k, 96);
    }
    for (int p = 0; p < n_points; p++) m->pts[(size_t)p].p = points[p];
    for (int i = 0; i < n_meas; i++) {
        KeyFrame& k = m->kfs[(size_t)meas[i].kf];
        MapPoint& p = m->pts[(size_t)meas[i].point];
        k.mMeasurements[&p] = Measurement{meas[i].level, meas[i].source, {meas[i].root_pos[0], meas[i].root_pos[1]}};
        p.sMeasurementKFs.insert(&k);
    }
    for (int i = 0; i < n_never; i++) m->pts[(size_t)never[i].point].sNeverRetryKFs.insert(&m->kfs[(size_t)never[i].kf]);
    return m;
}
void mrh_destroy(void* h) { delete (Map*)h; }

// the callers' loops up to the PatchFinder: -> the pair list (kept inside), its length
int mrh_pairs(void* h, int mode, int n_work, const void* work) {
    Map& m = *(Map*)h;
    g_pairs.clear();
    g_kf.clear();
    if (mode == PTAM_MAP_REFIND_KEYFRAME) {   // :1031-1037
        KeyFrame& k = m.kfs[(size_t) * (const int32_t*)work];
        std::vector<MapPoint*> vToFind;
        for (MapPoint& p : m.pts) vToFind.push_back(&p);
        for (MapPoint* p : vToFind) fill(m, k, *p, g_pairs);
    } else if (mode == PTAM_MAP_REFIND_NEW_POINTS) {   // :1053-1063
        const int32_t* w = (const int32_t*)work;
        for (int e = 0; e < n_work; e++) {
            MapPoint& p = m.pts[(size_t)w[e]];
            if (p.p.bad) continue;
            for (KeyFrame& k : m.kfs) fill(m, k, p, g_pairs);
        }
    } else {   // :1074-1078
        const ptam_map_pair* w = (const ptam_map_pair*)work;
        std::vector<std::pair<KeyFrame*, MapPoint*>> q;
        for (int e = 0; e < n_work; e++) q.emplace_back(&m.kfs[(size_t)w[e].kf], &m.pts[(size_t)w[e].point]);
        std::sort(q.begin(), q.end());
        for (size_t i = 0; i < q.size(); i++) {
            fill(m, *q[i].first, *q[i].second, g_pairs);
            if (i > 0 && q[i] == q[i - 1]) g_pairs.back().skip = 1;   // (its first visit has put it into one of the sets)
        }
    }
    return (int)g_pairs.size();
}
const ptam_refind_pair* mrh_pair_data() { return g_pairs.data(); }

// after ptam_refind_pairs: the inserts of :953-1018 and the sorted table for the next ptam_map_* call -> its length
int mrh_fold(void* h, int n, const ptam_refind_result* res, ptam_map_meas* table_out) {
    Map& m = *(Map*)h;
    for (int i = 0; i < n; i++) {
        if (g_pairs[(size_t)i].skip) continue;
        MapPoint& p = m.pts[(size_t)g_pairs[(size_t)i].point_id];
        KeyFrame* k = g_kf[(size_t)i];
        if (res[i].found) {
            k->mMeasurements[&p] = Measurement{res[i].level, PTAM_MAP_SRC_REFIND, {res[i].root_pos[0], res[i].root_pos[1]}};
            p.sMeasurementKFs.insert(k);
        } else
            p.sNeverRetryKFs.insert(k);
    }
    int n_rows = 0;
    for (KeyFrame& k : m.kfs)
        for (auto& e : k.mMeasurements) {
            ptam_map_meas& r = table_out[n_rows++];
            r.kf = (int32_t)(&k - m.kfs.data());
            r.point = (int32_t)(e.first - m.pts.data());
            r.level = e.second.nLevel;
            r.source = e.second.Source;
            r.root_pos[0] = e.second.v2RootPos[0];
            r.root_pos[1] = e.second.v2RootPos[1];
        }
    return n_rows;
}

}   // extern "C"
