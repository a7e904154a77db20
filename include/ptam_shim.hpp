// ptam_shim.hpp — header-only C++ shim that re-creates the reference's class surface for the hot
// path on top of the C ABI of ptam_hip.h, so the two-thread SLAM loop of cggos/ptam_cg can switch
// KeyFrame::MakeKeyFrame_Lite / PatchFinder::FindPatchCoarse / Tracker::CalcPoseUpdate + pose loop /
// Bundle to the MI355X path by changing includes (INTEGRATION.md shows the edits).
//
// TooN / libCVD are not available to this repo, so the shim uses POD stand-ins with the same
// meaning: ptam::SE3 (R row-major + t) for TooN::SE3<>, ptam::ImageRef for CVD::ImageRef,
// ptam::Vec<N> for TooN::Vector<N>.  A maintainer with TooN at hand converts with two memcpy's
// (see INTEGRATION.md §3).  Each method cites the reference declaration it mirrors.
#ifndef PTAM_SHIM_HPP
#define PTAM_SHIM_HPP

#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ptam_hip.h"

namespace ptam {

static_assert(sizeof(bool) == 1, "abort flag is passed as one byte");

struct ImageRef {   // CVD::ImageRef
    int x, y;
};
template <int N>
using Vec = std::array<double, N>;   // TooN::Vector<N>

struct SE3 {   // TooN::SE3<> : camera-from-world
    double R[9];   // row-major
    double t[3];
    static SE3 Identity() {
        SE3 s{};
        s.R[0] = s.R[4] = s.R[8] = 1.0;
        return s;
    }
    void to12(double* p) const {
        std::memcpy(p, R, sizeof R);
        std::memcpy(p + 9, t, sizeof t);
    }
    static SE3 from12(const double* p) {
        SE3 s;
        std::memcpy(s.R, p, sizeof s.R);
        std::memcpy(s.t, p + 9, sizeof s.t);
        return s;
    }
};

inline void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ptam_last_error());
}

// One per calling thread (tracker thread / mapmaker thread): replaces the per-owner ATANCamera copies
// of the reference (include/MapMaker.h:61, include/Tracker.h) and owns the HIP stream.
class Context {
public:
    // vParams = Camera.Parameters (config/camera.cfg:7), irSize = ATANCamera::SetImageSize
    Context(const Vec<5>& vParams, ImageRef irSize, int device = 0) {
        ptam_cam_params p{vParams[0], vParams[1], vParams[2], vParams[3], vParams[4], irSize.x, irSize.y};
        check(ptam_ctx_create(&p, device, &h_), "ptam_ctx_create");
        size_ = irSize;
    }
    ~Context() { ptam_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    ptam_ctx* handle() const { return h_; }
    ImageRef size() const { return size_; }
    void SetHalfSampleVariant(int v) { check(ptam_ctx_set_halfsample(h_, v), "set_halfsample"); }

private:
    ptam_ctx* h_ = nullptr;
    ImageRef size_{0, 0};
};

// struct Level (include/KeyFrame.h:55-124): host views are fetched lazily from the device
struct Level {
    int w = 0, h = 0;
    std::vector<uint8_t> im;                 // CVD::Image<CVD::byte>
    std::vector<ImageRef> vCorners;          // FAST corners, raster order
    std::vector<int> vCornerRowLUT;
    static int LevelScale(int nLevel) { return 1 << nLevel; }                                   // :85-88
    static double LevelZeroPos(double dLevelPos, int nLevel) { return (dLevelPos + 0.5) * LevelScale(nLevel) - 0.5; }
    static double LevelNPos(double dRootPos, int nLevel) { return (dRootPos + 0.5) / LevelScale(nLevel) - 0.5; }
};

// struct KeyFrame (include/KeyFrame.h:130-149)
class KeyFrame {
public:
    explicit KeyFrame(Context& c) : ctx_(&c) { check(ptam_kf_create(c.handle(), c.size().x, c.size().y, &h_), "ptam_kf_create"); }
    ~KeyFrame() { ptam_kf_destroy(h_); }
    KeyFrame(const KeyFrame& o) : ctx_(o.ctx_) {   // Level::operator= deep copy (:66-75), device side
        check(ptam_kf_clone(ctx_->handle(), o.h_, &h_), "ptam_kf_clone");
    }
    KeyFrame& operator=(const KeyFrame& o) {
        if (this != &o) {
            ptam_kf* n = nullptr;
            check(ptam_kf_clone(o.ctx_->handle(), o.h_, &n), "ptam_kf_clone");
            ptam_kf_destroy(h_);
            h_ = n;
            ctx_ = o.ctx_;
            fetched_ = 0;
        }
        return *this;
    }
    // the same deep copy into THIS keyframe's own memory (same image size): no allocation — the pooled clone of the tracker's
    // current keyframe for MapMaker::AddKeyFrame (ptam_kf_copy).  Asynchronous on the context's queue.
    KeyFrame& CopyFrom(const KeyFrame& o) {
        check(ptam_kf_copy(ctx_->handle(), o.h_, h_), "ptam_kf_copy");
        fetched_ = 0;
        return *this;
    }
    // void MakeKeyFrame_Lite(CVD::BasicImage<CVD::byte>& im)   include/KeyFrame.h:141, src/KeyFrame.cc:18
    void MakeKeyFrame_Lite(const uint8_t* im, int stride) {
        check(ptam_make_keyframe_lite(ctx_->handle(), h_, im, stride), "ptam_make_keyframe_lite");
        fetched_ = 0;
    }
    // void MakeKeyFrame_Rest()   include/KeyFrame.h:142, src/KeyFrame.cc:61-79; the keyframe's SmallBlurryImage (:80-81) is Relocaliser::AddKeyFrame
    void MakeKeyFrame_Rest() { check(ptam_make_keyframe_rest(ctx_->handle(), h_), "ptam_make_keyframe_rest"); }
    // aLevels[l] host view (pixels, vCorners, vCornerRowLUT)
    const Level& aLevels(int l) {
        if (!(fetched_ & (1u << l))) {
            Level& L = lev_[l];
            int n = 0;
            check(ptam_kf_level_info(ctx_->handle(), h_, l, &L.w, &L.h, &n), "ptam_kf_level_info");
            L.im.resize((size_t)L.w * L.h);
            L.vCorners.resize(n);
            L.vCornerRowLUT.resize(L.h);
            static_assert(sizeof(ImageRef) == sizeof(ptam_int2), "layout");
            check(ptam_kf_read_level(ctx_->handle(), h_, l, L.im.data(), reinterpret_cast<ptam_int2*>(L.vCorners.data()),
                                     L.vCornerRowLUT.data()),
                  "ptam_kf_read_level");
            fetched_ |= 1u << l;
        }
        return lev_[l];
    }
    ptam_kf* handle() const { return h_; }
    SE3 se3CfromW = SE3::Identity();
    bool bFixed = false;

private:
    Context* ctx_;
    ptam_kf* h_ = nullptr;
    Level lev_[PTAM_LEVELS];
    unsigned fetched_ = 0;
};

// class PatchFinder (include/PatchFinder.h:51-137): coarse search stage
class PatchFinder {
public:
    explicit PatchFinder(Context& c) : ctx_(&c) {}
    // template + level as left by MakeTemplateCoarseCont / NoWarp (src/PatchFinder.cc:98-148)
    void SetTemplate(const uint8_t tmpl64[64], int nSearchLevel, bool bBad = false) {
        std::memcpy(tmpl_, tmpl64, 64);
        mnSearchLevel = nSearchLevel;
        mbTemplateBad = bBad;
    }
    // void MakeTemplateCoarseCont(MapPoint& p)  include/PatchFinder.h:70, src/PatchFinder.cc:98-127.
    // The MapPoint fields it reads are passed explicitly: pPatchSourceKF, nSourceLevel, irCenter; mm2WarpInverse and
    // mnSearchLevel are what CalcSearchLevelAndWarpMatrix left (TrackMapPVS returns both per point).  `pPointId`
    // stands for the MapPoint's address in the reuse test ("same point and the warp moved < 0.07": keep the template).
    void MakeTemplateCoarseCont(const void* pPointId, KeyFrame& kfSource, int nSourceLevel, ImageRef irCenter,
                                const double mm2WarpInverse[4], int nSearchLevel) {
        mnSearchLevel = nSearchLevel;
        if (nSearchLevel < 0) {   // CalcSearchLevelAndWarpMatrix returned -1 and set mbTemplateBad (src/PatchFinder.cc:78-81)
            mbTemplateBad = true;
            return;
        }
        // m2 = M2Inverse(mm2WarpInverse) * LevelScale(mnSearchLevel)   (include/Tools.h:54-65)
        const double det = mm2WarpInverse[0] * mm2WarpInverse[3] - mm2WarpInverse[2] * mm2WarpInverse[1];
        const double inv = 1.0 / det, sc = (double)(1 << nSearchLevel);
        const double m2[4] = {mm2WarpInverse[3] * inv * sc, -mm2WarpInverse[1] * inv * sc, -mm2WarpInverse[2] * inv * sc,
                              mm2WarpInverse[0] * inv * sc};
        bool refresh = pPointId != mpLastTemplateMapPoint;
        for (int i = 0; !refresh && i < 2; i++) {   // columns of m2 against the last warp matrix
            const double d0 = m2[i] - mm2LastWarpMatrix[i], d1 = m2[2 + i] - mm2LastWarpMatrix[2 + i];
            if (d0 * d0 + d1 * d1 > 0.07 * 0.07) refresh = true;
        }
        if (!refresh) return;
        ptam_template_query q{kfSource.handle(), nSourceLevel, nSearchLevel, irCenter.x, irCenter.y,
                              {mm2WarpInverse[0], mm2WarpInverse[1], mm2WarpInverse[2], mm2WarpInverse[3]}};
        ptam_template_result r;
        check(ptam_make_templates_batch(ctx_->handle(), 1, &q, tmpl_, &r), "ptam_make_templates_batch");
        mbTemplateBad = r.bad != 0;
        mpLastTemplateMapPoint = pPointId;
        for (int i = 0; i < 4; i++) mm2LastWarpMatrix[i] = r.m2[i];
    }
    // the batched form for SearchForPoints: every template of a frame in one launch (no reuse test: callers that want
    // it keep (point id, m2) per point and drop the unchanged queries before the call)
    static void MakeTemplatesBatch(Context& c, const std::vector<ptam_template_query>& q, std::vector<uint8_t>& templates64,
                                   std::vector<ptam_template_result>& out) {
        templates64.resize(q.size() * 64);
        out.resize(q.size());
        check(ptam_make_templates_batch(c.handle(), (int)q.size(), q.data(), templates64.data(), out.data()),
              "ptam_make_templates_batch");
    }
    // bool FindPatchCoarse(CVD::ImageRef ir, KeyFrame& kf, unsigned int nRange)  include/PatchFinder.h:78
    bool FindPatchCoarse(ImageRef irPos, KeyFrame& kf, unsigned int nRange) {
        ptam_patch_query q{irPos.x, irPos.y, mbTemplateBad ? -1 : mnSearchLevel, nRange};
        ptam_patch_result r;
        check(ptam_find_patch_coarse_batch(ctx_->handle(), kf.handle(), 1, &q, tmpl_, &r), "ptam_find_patch_coarse_batch");
        mbFound = r.found != 0;
        if (mbFound) mv2CoarsePos = {r.pos[0], r.pos[1]};
        return mbFound;
    }
    // the batched form SearchForPoints (src/Tracker.cc:867-912) should use: one launch for all patches
    static void FindPatchCoarseBatch(Context& c, KeyFrame& kf, const std::vector<ptam_patch_query>& q,
                                     const std::vector<uint8_t>& templates64, std::vector<ptam_patch_result>& out) {
        out.resize(q.size());
        check(ptam_find_patch_coarse_batch(c.handle(), kf.handle(), (int)q.size(), q.data(), templates64.data(), out.data()),
              "ptam_find_patch_coarse_batch");
    }
    // the corner scan of MapMaker::AddPointEpipolar (src/MapMaker.cc:598-637) for every candidate of a source
    // keyframe level at once: MakeTemplateCoarseNoWarp + band / segment test over kTarget's in-plane corners +
    // ZMSSDAtPoint; result[i].best indexes kTarget.aLevels(nLevel).vCorners.  The caller keeps the line geometry
    // (:541-596) and fills one ptam_epipolar_query per candidate; max_dist_sq = (OnePixelDist * (4 + nLevelScale))^2.
    static void EpipolarSearchBatch(Context& c, KeyFrame& kSrc, KeyFrame& kTarget, int nLevel,
                                    const std::vector<ptam_epipolar_query>& q, std::vector<ptam_epipolar_result>& out) {
        out.resize(q.size());
        check(ptam_epipolar_search_batch(c.handle(), kSrc.handle(), kTarget.handle(), nLevel, (int)q.size(), q.data(), out.data()),
              "ptam_epipolar_search_batch");
    }
    // int ZMSSDAtPoint(CVD::BasicImage<CVD::byte>&, const CVD::ImageRef&)   include/PatchFinder.h:79
    int ZMSSDAtPoint(KeyFrame& kf, int nLevel, ImageRef ir) {
        ptam_int2 p{ir.x, ir.y};
        int32_t v = 0;
        check(ptam_zmssd_at_points(ctx_->handle(), kf.handle(), nLevel, 1, &p, tmpl_, &v), "ptam_zmssd_at_points");
        return v;
    }
    // void MakeSubPixTemplate(); bool IterateSubPixToConvergence(KeyFrame&, int nMaxIts)
    //   include/PatchFinder.h:83-87, src/PatchFinder.cc:219-318 — starts at the coarse position
    bool IterateSubPixToConvergence(KeyFrame& kf, int nMaxIts) {
        ptam_subpix_query q{{mv2CoarsePos[0], mv2CoarsePos[1]}, mnSearchLevel, nMaxIts};
        ptam_subpix_result r;
        check(ptam_subpix_batch(ctx_->handle(), kf.handle(), 1, &q, tmpl_, &r), "ptam_subpix_batch");
        mv2SubPixPos = {r.pos[0], r.pos[1]};
        return r.converged != 0;
    }
    Vec<2> GetSubPixPos() const { return mv2SubPixPos; }
    Vec<2> GetCoarsePosAsVector() const { return mv2CoarsePos; }
    int GetLevel() const { return mnSearchLevel; }
    bool TemplateBad() const { return mbTemplateBad; }

private:
    Context* ctx_;
    uint8_t tmpl_[64] = {0};
    int mnSearchLevel = 0;
    bool mbTemplateBad = false, mbFound = false;
    const void* mpLastTemplateMapPoint = nullptr;            // include/PatchFinder.h:135-136
    double mm2LastWarpMatrix[4] = {9999.9, 0, 0, 9999.9};    // src/PatchFinder.cc:21-22
    Vec<2> mv2CoarsePos{0, 0}, mv2SubPixPos{0, 0};
};

// void MapMaker::AddSomeMapPoints(int nLevel)   src/MapMaker.cc:448-457, for every level of opts.levels in turn, in ONE device call
// (ptam_add_map_points_epipolar; beside PatchFinder::EpipolarSearchBatch, whose corner scan it shares): ThinCandidates against
// kSrc's measurements `busy` and the points made at earlier levels, then AddPointEpipolar for every kept candidate.  The new
// points come back in the order the reference pushes them onto vpPoints / mqNewQueue; the map bookkeeping stays the caller's.
struct BusyMeasurement {   // kSrc.mMeasurements: (nLevel, v2RootPos)
    int nLevel;
    Vec<2> v2RootPos;
};
inline std::vector<ptam_new_map_point> AddMapPointsEpipolar(Context& c, KeyFrame& kSrc, const SE3& se3Src, KeyFrame& kTarget,
                                                           const SE3& se3Target, const ptam_epipolar_opts& opts,
                                                           const std::vector<BusyMeasurement>& busy,
                                                           std::vector<ptam_epipolar_level_stats>* stats = nullptr) {
    int cap = 0;
    for (int i = 0; i < opts.n_levels && i < PTAM_LEVELS; i++) {
        int n = 0;
        if (opts.levels[i] >= 0 && opts.levels[i] < PTAM_LEVELS)
            check(ptam_kf_rest_info(c.handle(), kSrc.handle(), opts.levels[i], &n), "ptam_kf_rest_info");
        cap += n;
    }
    std::vector<int32_t> lv(busy.size());
    std::vector<double> xy(2 * busy.size());
    for (size_t i = 0; i < busy.size(); i++) {
        lv[i] = busy[i].nLevel;
        xy[2 * i] = busy[i].v2RootPos[0];
        xy[2 * i + 1] = busy[i].v2RootPos[1];
    }
    double ps[12], pt[12];
    se3Src.to12(ps);
    se3Target.to12(pt);
    std::vector<ptam_new_map_point> out((size_t)cap);
    std::vector<ptam_epipolar_level_stats> st(PTAM_LEVELS);
    int32_t n = 0;
    check(ptam_add_map_points_epipolar(c.handle(), kSrc.handle(), ps, kTarget.handle(), pt, &opts, (int)busy.size(), lv.data(), xy.data(),
                                       out.data(), cap, &n, st.data()),
          "ptam_add_map_points_epipolar");
    out.resize((size_t)n);
    if (stats) stats->assign(st.begin(), st.begin() + opts.n_levels);
    return out;
}

// Tracker::TrailTracking_Start() / int TrailTracking_Advance()   src/Tracker.cc:352-432, with the list mlTrails and
// mPreviousFrameKF kept on the device (ptam_trails_*).  The caller's TrackForInitialMap (:311-347) keeps its stage enum, the
// `nGoodTrails < 10 -> Reset()` test and the spacebar; Matches() is the vMatches table of InitFromStereo (src/MapMaker.cc:272-279),
// Homography() the Compute call on it (:281-293) without the download.
class TrailTracker {
public:
    explicit TrailTracker(Context& c, int nMaxInitialTrails = 1000 /* Tracker.MaxInitialTrails */, double dMinShiTomasi = 70.0)
        : max_(nMaxInitialTrails), min_st_(dMinShiTomasi) {
        check(ptam_trails_create(c.handle(), nMaxInitialTrails, &h_), "ptam_trails_create");
    }
    ~TrailTracker() { ptam_trails_destroy(h_); }
    TrailTracker(const TrailTracker&) = delete;
    TrailTracker& operator=(const TrailTracker&) = delete;
    // kf must have had MakeKeyFrame_Rest (:354); returns the number of trails
    int Start(KeyFrame& kf) {
        int n = 0;
        check(ptam_trails_start(h_, kf.handle(), min_st_, max_, &n), "ptam_trails_start");
        return n;
    }
    // returns nGoodTrails; the trails alive afterwards: Alive()
    int Advance(KeyFrame& kf) {
        int good = 0;
        check(ptam_trails_advance(h_, kf.handle(), &good, &alive_), "ptam_trails_advance");
        return good;
    }
    int Alive() const { return alive_; }
    // MakeKeyFrame_Lite of vdFrames[i] (null: vCurrent[i] is made already) and Advance for every camera as ONE chain on the first
    // tracker's queue (ptam_trails_advance_batch): Contexts of their own on one device.  -> nGoodTrails per camera; Alive() each
    static std::vector<int> AdvanceBatch(const std::vector<TrailTracker*>& vTrails, const std::vector<KeyFrame*>& vCurrent,
                                         const std::vector<const uint8_t*>& vdFrames) {
        const size_t n = vTrails.size();
        if (n == 0 || vCurrent.size() != n || (!vdFrames.empty() && vdFrames.size() != n)) throw std::runtime_error("AdvanceBatch: sizes differ");
        std::vector<ptam_trails*> t(n);
        std::vector<ptam_kf*> k(n);
        for (size_t i = 0; i < n; i++) t[i] = vTrails[i]->h_, k[i] = vCurrent[i]->handle();
        std::vector<int32_t> good(n), alive(n);
        check(ptam_trails_advance_batch((int)n, t.data(), k.data(), vdFrames.empty() ? nullptr : vdFrames.data(), good.data(), alive.data()),
              "ptam_trails_advance_batch");
        for (size_t i = 0; i < n; i++) vTrails[i]->alive_ = alive[i];
        return std::vector<int>(good.begin(), good.end());
    }
    std::vector<ptam_trail> Trails() {   // mlTrails: irInitialPos, irCurrentPos
        std::vector<ptam_trail> v((size_t)max_);
        int n = 0;
        check(ptam_trails_read(h_, v.data(), max_, &n), "ptam_trails_read");
        v.resize((size_t)n);
        return v;
    }
    std::vector<ptam_homography_match> Matches() {
        std::vector<ptam_homography_match> v((size_t)max_);
        int n = 0;
        check(ptam_trails_matches(h_, v.data(), max_, &n), "ptam_trails_matches");
        v.resize((size_t)n);
        return v;
    }
    // HomographyInit::Compute(vMatches, dMaxPixelError, se3) on the match table of the live trails, which stays on the device
    // (ptam_trails_homography); opts (nullable): the number of trials and the draw.  pInfo (nullable): scores, counts, status.
    bool Homography(double dMaxPixelError, SE3& se3SecondFromFirst, const ptam_homography_opts* opts = nullptr,
                    ptam_homography_info* pInfo = nullptr) {
        ptam_homography_opts o;
        if (opts)
            o = *opts;
        else
            ptam_homography_opts_default(&o);
        o.max_pixel_error = dMaxPixelError;
        double p[12];
        ptam_homography_info info;
        check(ptam_trails_homography(h_, &o, p, &info, nullptr), "ptam_trails_homography");
        if (pInfo) *pInfo = info;
        if (info.status != PTAM_HOMOG_OK) return false;
        se3SecondFromFirst = SE3::from12(p);
        return true;
    }
    ptam_trails* handle() const { return h_; }

private:
    ptam_trails* h_ = nullptr;
    int max_, alive_ = 0;
    double min_st_;
};

// class HomographyInit (include/HomographyInit.h:39-66): bool Compute(std::vector<HomographyMatch> vMatches, double dMaxPixelError,
// SE3<>& se3SecondFromFirst), src/HomographyInit.cc:35-63, in one device call (ptam_homography_init).  HomographyMatch is
// ptam_homography_match (v2CamPlaneFirst, v2CamPlaneSecond, m2PixelProjectionJac row-major).  The reference draws its quadruples
// with rand(); here the draw is seeded (SetSeed, splitmix64: ptam_hip.h) or handed in (SetSamples: 4 indices per trial).
using HomographyMatch = ptam_homography_match;
class HomographyInit {
public:
    explicit HomographyInit(Context& c) : ctx_(&c) { ptam_homography_opts_default(&opts_); }
    void SetSeed(uint64_t seed) {
        opts_.seed = seed;
        samples_.clear();
    }
    void SetTrials(int nTrials) {
        opts_.trials = nTrials;
        samples_.clear();
    }
    void SetSamples(const std::vector<int32_t>& vSamples) {
        samples_ = vSamples;
        opts_.trials = (int)(samples_.size() / 4);
    }
    bool Compute(std::vector<HomographyMatch> vMatches, double dMaxPixelError, SE3& se3SecondFromFirst) {
        ptam_homography_opts o = opts_;
        o.max_pixel_error = dMaxPixelError;
        o.samples = samples_.empty() ? nullptr : samples_.data();
        double p[12];
        inliers_.assign(vMatches.size(), 0);
        check(ptam_homography_init(ctx_->handle(), (int)vMatches.size(), vMatches.data(), &o, p, &info_, inliers_.data()),
              "ptam_homography_init");
        if (info_.status != PTAM_HOMOG_OK) return false;
        se3SecondFromFirst = SE3::from12(p);
        return true;
    }
    const ptam_homography_info& Info() const { return info_; }        // of the last Compute
    const std::vector<uint8_t>& Inliers() const { return inliers_; }   // 1: the match is in mvHomographyInliers

private:
    Context* ctx_;
    ptam_homography_opts opts_;
    ptam_homography_info info_{};
    std::vector<int32_t> samples_;
    std::vector<uint8_t> inliers_;
};

// CalibImage (include/CalibImage.h) without the checkerboard finder: the corners come from the caller's detector.
struct CalibGridCorner {
    ImageRef irGridPos;
    struct {
        Vec<2> v2Pos;
    } Params;
};
struct CalibImage {
    std::vector<CalibGridCorner> mvGridCorners;
    SE3 mse3CamFromWorld = SE3::Identity();   // as of the calibrator's last call
};
// CameraCalibrator's optimiser (src/CameraCalibrator.cc:156-165, 215-269) on the device, ptam_calib_*: AddImage is the
// push_back + GuessInitialPose of Run (:105-106), OptimizeOneStep the call of :114.  The camera lives on the device; Params()
// reads it.  After every call mvCalibImgs[i].mse3CamFromWorld is the device's pose of image i.
class CameraCalibrator {
public:
    CameraCalibrator(Context& c, int nMaxImages = 64, int nMaxCornersTotal = 64 * 256) : ctx_(&c) {
        check(ptam_calib_create(c.handle(), nMaxImages, nMaxCornersTotal, &h_), "ptam_calib_create");
    }
    ~CameraCalibrator() { ptam_calib_destroy(h_); }
    CameraCalibrator(const CameraCalibrator&) = delete;
    CameraCalibrator& operator=(const CameraCalibrator&) = delete;
    ptam_calibrator* handle() const { return h_; }

    void Reset(bool bDisableDistortion = false) {   // *mCamera.mgvvCameraParams = ATANCamera::mvDefaultParams
        check(ptam_calib_reset(h_, nullptr, bDisableDistortion ? 1 : 0), "ptam_calib_reset");
        mvCalibImgs.clear();
        result_ = ptam_calib_result{};
    }
    void Reset(const Vec<5>& vParams, bool bDisableDistortion = false) {
        check(ptam_calib_reset(h_, vParams.data(), bDisableDistortion ? 1 : 0), "ptam_calib_reset");
        mvCalibImgs.clear();
        result_ = ptam_calib_result{};
    }
    // false: the image's initial pose was refused (ptam_hip.h) and the image is not kept
    bool AddImage(const CalibImage& c) {
        std::vector<ptam_calib_corner> v(c.mvGridCorners.size());
        for (size_t i = 0; i < v.size(); i++) {
            const CalibGridCorner& g = c.mvGridCorners[i];
            v[i] = ptam_calib_corner{g.irGridPos.x, g.irGridPos.y, g.Params.v2Pos[0], g.Params.v2Pos[1]};
        }
        const int32_t first[2] = {0, (int32_t)v.size()};
        int32_t status = PTAM_CALIB_GUESS_REFUSED;
        check(ptam_calib_add_images(h_, 1, first, v.data(), &status), "ptam_calib_add_images");
        if (status != PTAM_CALIB_GUESS_OK) return false;
        mvCalibImgs.push_back(c);
        ReadPoses();
        return true;
    }
    bool OptimizeOneStep() { return Optimize(1); }
    // nSteps x OptimizeOneStep in one device call; false: nothing to adjust (PTAM_CALIB_NO_MEASUREMENTS)
    bool Optimize(int nSteps) {
        rms_.assign((size_t)(nSteps > 0 ? nSteps : 0), 0.0);
        check(ptam_calib_optimize(h_, nSteps, &result_, rms_.data()), "ptam_calib_optimize");
        ReadPoses();
        return result_.status == PTAM_CALIB_OK;
    }
    double MeanPixelError() const { return result_.rms; }   // mdMeanPixelError of the last step
    Vec<5> Params() const {
        Vec<5> v;
        check(ptam_calib_params(h_, v.data()), "ptam_calib_params");
        return v;
    }
    const ptam_calib_result& Result() const { return result_; }
    const std::vector<double>& RMSHistory() const { return rms_; }
    // the one line GVars reads from camera.cfg (GV2.PrintVar("Camera.Parameters", ofs), :190-200)
    static std::string ConfigLine(const Vec<5>& v) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "Camera.Parameters=[ %.17g %.17g %.17g %.17g %.17g ]\n", v[0], v[1], v[2], v[3], v[4]);
        return buf;
    }
    bool SaveCalib(const std::string& sPath = "camera.cfg") const {
        FILE* f = std::fopen(sPath.c_str(), "w");
        if (!f) return false;
        const std::string s = ConfigLine(Params());
        const bool ok = std::fwrite(s.data(), 1, s.size(), f) == s.size();
        return std::fclose(f) == 0 && ok;
    }
    std::vector<CalibImage> mvCalibImgs;

private:
    void ReadPoses() {
        if (mvCalibImgs.empty()) return;
        std::vector<double> p(mvCalibImgs.size() * 12);
        check(ptam_calib_read_poses(h_, p.data()), "ptam_calib_read_poses");
        for (size_t i = 0; i < mvCalibImgs.size(); i++) mvCalibImgs[i].mse3CamFromWorld = SE3::from12(&p[i * 12]);
    }
    Context* ctx_;
    ptam_calibrator* h_ = nullptr;
    ptam_calib_result result_{};
    std::vector<double> rms_;
};

// The point loop of MapMaker::InitFromStereo (src/MapMaker.cc:310-367) in ONE device call (ptam_init_points_from_trails):
// se3 = HomographyInit's pose scaled to WiggleScale (:296-297).  The made points come back in vpPoints order with both
// measurements (src_root_pos: SRC_ROOT in kF, target_pos: SRC_TRAIL in kS); pvStatus (nullable): PTAM_INIT_* per match.
inline std::vector<ptam_new_map_point> InitPointsFromTrails(Context& c, KeyFrame& kF, KeyFrame& kS, const SE3& se3,
                                                           const std::vector<ptam_trail>& vTrailMatches,
                                                           std::vector<int32_t>* pvStatus = nullptr, int nSubPixMaxIts = 10) {
    double p[12];
    se3.to12(p);
    std::vector<ptam_new_map_point> out(vTrailMatches.size());
    std::vector<int32_t> st(vTrailMatches.size());
    int32_t n = 0;
    check(ptam_init_points_from_trails(c.handle(), kF.handle(), kS.handle(), p, (int)vTrailMatches.size(), vTrailMatches.data(),
                                       nSubPixMaxIts, out.data(), st.data(), &n),
          "ptam_init_points_from_trails");
    out.resize((size_t)n);
    if (pvStatus) *pvStatus = st;
    return out;
}

// void MapMaker::BundleAdjustRecent() / BundleAdjustAll()   src/MapMaker.cc:768-933, set choice + Bundle + write-back in ONE device
// call (ptam_map_bundle_adjust) on the map as flat tables: vKFPoses / vFixed in vpKeyFrames order (the newest last), vPoints in
// vpPoints order, vMeas = every keyframe's mMeasurements sorted by (kf, point).  With accepted > 0 the poses and points are updated
// in place; the outliers come back in GetOutlierMeasurements order with the action the caller applies (ptam_hip.h).
struct MapBundleAdjustResult {
    ptam_map_ba_result result;
    std::vector<ptam_map_outlier> outliers;
    std::vector<int32_t> cam_kf, point_ids;   // bundle camera / point id -> table index
};
static_assert(sizeof(SE3) == 96 && sizeof(Vec<3>) == 24, "tables are handed over as flat doubles");
inline MapBundleAdjustResult MapBundleAdjust(Context& c, int mode, std::vector<SE3>& vKFPoses, const std::vector<uint8_t>& vFixed,
                                             std::vector<Vec<3>>& vPoints, const std::vector<ptam_map_meas>& vMeas,
                                             bool* pbAbortSignal = nullptr, const ptam_ba_opts* opts = nullptr) {
    if (vFixed.size() != vKFPoses.size()) throw std::runtime_error("MapBundleAdjust: one bFixed per keyframe");
    MapBundleAdjustResult r{};
    r.outliers.resize(vMeas.size());
    r.cam_kf.resize(vKFPoses.size());
    r.point_ids.resize(vPoints.size());
    check(ptam_map_bundle_adjust(c.handle(), opts, mode, (int)vKFPoses.size(), reinterpret_cast<double*>(vKFPoses.data()), vFixed.data(),
                                 (int)vPoints.size(), reinterpret_cast<double*>(vPoints.data()), (int)vMeas.size(), vMeas.data(),
                                 reinterpret_cast<const volatile unsigned char*>(pbAbortSignal), &r.result, r.outliers.data(),
                                 (int)vMeas.size(), r.cam_kf.data(), r.point_ids.data()),
          "ptam_map_bundle_adjust");
    r.outliers.resize((size_t)r.result.n_outliers);
    r.cam_kf.resize((size_t)(r.result.n_adjust + r.result.n_fixed));
    r.point_ids.resize((size_t)r.result.n_points);
    return r;
}

// SE3<> MapMaker::CalcPlaneAligner()   src/MapMaker.cc:1100-1195 on the point table in one device call (ptam_calc_plane_aligner).
// The reference draws its triples with rand(); here the draw is opts->seed (splitmix64: ptam_hip.h) or opts->samples.  A status
// other than PTAM_PLANE_OK comes with the identity, as the reference's "too few points" does.
struct PlaneAligner {
    SE3 se3 = SE3::Identity();
    ptam_plane_info info{};
    std::vector<uint8_t> inliers;   // 1: the point is in vv3Inliers
};
inline ptam_plane_opts PlaneOptsOrDefault(const ptam_plane_opts* opts) {
    ptam_plane_opts o;
    ptam_plane_opts_default(&o);
    return opts ? *opts : o;
}
inline PlaneAligner CalcPlaneAligner(Context& c, const std::vector<Vec<3>>& vPoints, const ptam_plane_opts* opts = nullptr) {
    const ptam_plane_opts o = PlaneOptsOrDefault(opts);
    PlaneAligner r;
    r.inliers.assign(vPoints.size(), 0);
    double p[12];
    check(ptam_calc_plane_aligner(c.handle(), (int)vPoints.size(), reinterpret_cast<const double*>(vPoints.data()), &o, p, &r.info,
                                  r.inliers.data()),
          "ptam_calc_plane_aligner");
    r.se3 = SE3::from12(p);
    return r;
}

// void MapMaker::ApplyGlobalTransformationToMap(SE3<> se3NewFromOld)   src/MapMaker.cc:463-472 on the map tables in one device call
// (ptam_map_apply_global_transform): poses and points are updated in place.  With pvSources (pPatchSourceKF as an index, the _NC
// vectors) every point's RefreshPixelVectors runs too and the rows ptam_tracker_set_map takes come back; without, nothing does.
inline std::vector<ptam_pvs_point> ApplyGlobalTransformationToMap(Context& c, const SE3& se3NewFromOld, std::vector<SE3>& vKFPoses,
                                                                 std::vector<Vec<3>>& vPoints,
                                                                 const std::vector<ptam_map_point_source>* pvSources = nullptr) {
    if (pvSources && pvSources->size() != vPoints.size()) throw std::runtime_error("ApplyGlobalTransformationToMap: one source per point");
    std::vector<ptam_pvs_point> out(pvSources ? vPoints.size() : 0);
    double p[12];
    se3NewFromOld.to12(p);
    check(ptam_map_apply_global_transform(c.handle(), p, (int)vKFPoses.size(), reinterpret_cast<double*>(vKFPoses.data()),
                                          (int)vPoints.size(), reinterpret_cast<double*>(vPoints.data()),
                                          pvSources ? pvSources->data() : nullptr, pvSources ? out.data() : nullptr),
          "ptam_map_apply_global_transform");
    return out;
}

// ApplyGlobalTransformationToMap(CalcPlaneAligner())   src/MapMaker.cc:397 as ONE device call (ptam_map_align_to_plane).  The tables
// move only when the status is PTAM_PLANE_OK; pvOut (with pvSources) receives the refreshed rows unless it is PTAM_PLANE_DEGENERATE.
inline PlaneAligner AlignMapToPlane(Context& c, std::vector<SE3>& vKFPoses, std::vector<Vec<3>>& vPoints,
                                    const std::vector<ptam_map_point_source>* pvSources = nullptr,
                                    std::vector<ptam_pvs_point>* pvOut = nullptr, const ptam_plane_opts* opts = nullptr) {
    if ((pvSources == nullptr) != (pvOut == nullptr)) throw std::runtime_error("AlignMapToPlane: sources and rows come together");
    if (pvSources && pvSources->size() != vPoints.size()) throw std::runtime_error("AlignMapToPlane: one source per point");
    const ptam_plane_opts o = PlaneOptsOrDefault(opts);
    PlaneAligner r;
    r.inliers.assign(vPoints.size(), 0);
    if (pvOut) pvOut->assign(vPoints.size(), ptam_pvs_point{});
    double p[12];
    check(ptam_map_align_to_plane(c.handle(), &o, (int)vKFPoses.size(), reinterpret_cast<double*>(vKFPoses.data()), (int)vPoints.size(),
                                  reinterpret_cast<double*>(vPoints.data()), pvSources ? pvSources->data() : nullptr,
                                  pvOut ? pvOut->data() : nullptr, p, &r.info, r.inliers.data()),
          "ptam_map_align_to_plane");
    r.se3 = SE3::from12(p);
    return r;
}

// void MapMaker::RefreshSceneDepth(KeyFrame* pKF)   src/MapMaker.cc:1202-1219 for every keyframe of the table in one device call
// (ptam_map_scene_depth): vMeas as MapBundleAdjust takes it.  dSceneDepthMean / dSceneDepthSigma per keyframe; n_meas where the
// reference asserts.
inline std::vector<ptam_scene_depth> RefreshSceneDepth(Context& c, const std::vector<SE3>& vKFPoses, const std::vector<Vec<3>>& vPoints,
                                                       const std::vector<ptam_map_meas>& vMeas) {
    std::vector<ptam_scene_depth> out(vKFPoses.size());
    check(ptam_map_scene_depth(c.handle(), (int)vKFPoses.size(), reinterpret_cast<const double*>(vKFPoses.data()), (int)vPoints.size(),
                               reinterpret_cast<const double*>(vPoints.data()), (int)vMeas.size(), vMeas.data(), out.data()),
          "ptam_map_scene_depth");
    return out;
}

// TrackMap's potentially-visible-set loop (src/Tracker.cc:453-478): TData.Project + GetProjectionDerivs
// + Finder.CalcSearchLevelAndWarpMatrix for every map point, one launch.
inline void TrackMapPVS(Context& c, const std::vector<ptam_pvs_point>& vMapPoints, const SE3& se3CamFromWorld,
                        std::vector<ptam_pvs_result>& out, int anPVSSize[PTAM_LEVELS] = nullptr) {
    double pose[12];
    se3CamFromWorld.to12(pose);
    out.resize(vMapPoints.size());
    int32_t counts[4];
    check(ptam_track_pvs(c.handle(), (int)vMapPoints.size(), vMapPoints.data(), pose, out.data(), counts), "ptam_track_pvs");
    if (anPVSSize)
        for (int l = 0; l < PTAM_LEVELS; l++) anPVSSize[l] = counts[l];
}

// The part of TrackerData (include/Tracker.h:41-145) the pose loop reads
struct TrackerDataLite {
    Vec<3> v3WorldPos;       // Point.v3WorldPos
    Vec<2> v2Found;          // v2Found (L0 pixels)
    double dSqrtInvNoise;    // 1 / 2^level
    bool bOutlier = false;   // set where Tracker::CalcPoseUpdate would ++nMEstimatorOutlierCount
};

// Tracker::TrackMap's ten Gauss-Newton pose iterations (src/Tracker.cc:613-643; :552-568 when bCoarse),
// including every CalcPoseUpdate (:928-1005), in one device launch.
inline SE3 TrackMapPoseIterations(Context& c, std::vector<TrackerDataLite>& vTD, const SE3& se3CamFromWorld,
                                  bool bCoarse = false, int nEstimator = PTAM_EST_TUKEY) {
    std::vector<ptam_pose_meas> m(vTD.size());
    for (size_t i = 0; i < vTD.size(); i++) {
        std::memcpy(m[i].world, vTD[i].v3WorldPos.data(), 24);
        std::memcpy(m[i].found, vTD[i].v2Found.data(), 16);
        m[i].sqrt_inv_noise = vTD[i].dSqrtInvNoise;
    }
    ptam_gn_opts o;
    ptam_gn_opts_default(&o);
    o.estimator = nEstimator;
    if (bCoarse) {
        o.nonlinear_mask = 0x3ff;
        o.override_sigma_sq = 1.0;
        o.mark_outliers_iter = -1;
    }
    double pose[12];
    se3CamFromWorld.to12(pose);
    std::vector<int32_t> flags(vTD.size());
    check(ptam_pose_gn(c.handle(), (int)m.size(), m.data(), nullptr, pose, &o, flags.data(), nullptr), "ptam_pose_gn");
    for (size_t i = 0; i < vTD.size(); i++) vTD[i].bOutlier = flags[i] != 0;
    return SE3::from12(pose);
}

// The fine stage of a tracked frame with nothing but the pose crossing PCIe: SearchForPoints over the potentially
// visible set (src/Tracker.cc:867-912: FindPatchCoarse per point, every found patch becomes a measurement with
// v2Found = coarse position and dSqrtInvNoise = 1 / LevelScale) followed by the ten pose iterations (:613-643).
// Queries / templates / world positions are device buffers the caller filled (ptam_dev_upload, or the outputs of
// ptam_track_pvs / ptam_make_templates_batch kept resident); results stay resident for the caller to read lazily
// (outlier flags + source indices route nMEstimatorOutlierCount back to the map points).
class ResidentFrameTracker {
public:
    ResidentFrameTracker(Context& c, int nCapacity) : c_(c), cap_(nCapacity) {
        alloc(&res_, sizeof(ptam_patch_result) * (size_t)cap_);
        alloc(&meas_, sizeof(ptam_pose_meas) * (size_t)cap_);
        alloc(&src_, 4 * (size_t)cap_);
        alloc(&flags_, 4 * (size_t)cap_);
        alloc(&count_, 32);
        alloc(&pose_, 96);
    }
    ~ResidentFrameTracker() {
        for (void* p : {res_, meas_, src_, flags_, count_, pose_})
            if (p) ptam_dev_free(c_.handle(), p);
    }
    ResidentFrameTracker(const ResidentFrameTracker&) = delete;
    ResidentFrameTracker& operator=(const ResidentFrameTracker&) = delete;

    // d_world: 3 doubles per query every nWorldStrideBytes (sizeof(ptam_pvs_point) reads them out of the PVS input)
    SE3 SearchAndUpdatePose(KeyFrame& kfCurrent, int n, const ptam_patch_query* d_queries, const uint8_t* d_templates,
                            const void* d_world, int nWorldStrideBytes, const SE3& se3Predicted, int nEstimator = PTAM_EST_TUKEY) {
        check(ptam_find_patch_coarse_batch_dev(c_.handle(), kfCurrent.handle(), n, d_queries, d_templates,
                                               (ptam_patch_result*)res_), "ptam_find_patch_coarse_batch_dev");
        int32_t* cnt = (int32_t*)count_;
        check(ptam_gather_pose_meas_dev(c_.handle(), n, d_queries, (const ptam_patch_result*)res_, nullptr, d_world,
                                        nWorldStrideBytes, (ptam_pose_meas*)meas_, (int32_t*)src_, cnt, cnt + 2),
              "ptam_gather_pose_meas_dev");
        ptam_gn_opts o;
        ptam_gn_opts_default(&o);
        o.estimator = nEstimator;
        double in[12], out[12];
        se3Predicted.to12(in);
        check(ptam_pose_gn_dev_counted(c_.handle(), n, cnt, (const ptam_pose_meas*)meas_, nullptr, (double*)pose_, &o,
                                       (int32_t*)flags_, nullptr, in, out), "ptam_pose_gn_dev_counted");
        return SE3::from12(out);
    }
    // measurements of the last frame: count, manMeasFound per level (src/Tracker.cc:892), and per measurement the query it
    // came from and whether iteration 9 weighted it to zero
    int ReadBack(std::vector<int32_t>& vnSourceQuery, std::vector<int32_t>& vnOutlier, int anMeasFound[PTAM_LEVELS] = nullptr) {
        int32_t head[8];
        check(ptam_dev_download(c_.handle(), head, count_, sizeof head), "ptam_dev_download");
        const int n = head[0];
        vnSourceQuery.resize(n);
        vnOutlier.resize(n);
        if (n > 0) {
            check(ptam_dev_download(c_.handle(), vnSourceQuery.data(), src_, 4 * (size_t)n), "ptam_dev_download");
            check(ptam_dev_download(c_.handle(), vnOutlier.data(), flags_, 4 * (size_t)n), "ptam_dev_download");
        }
        if (anMeasFound)
            for (int l = 0; l < PTAM_LEVELS; l++) anMeasFound[l] = head[2 + l];
        return n;
    }

private:
    void alloc(void** p, size_t bytes) { check(ptam_dev_alloc(c_.handle(), bytes, p), "ptam_dev_alloc"); }
    Context& c_;
    int cap_;
    void *res_ = nullptr, *meas_ = nullptr, *src_ = nullptr, *flags_ = nullptr, *count_ = nullptr, *pose_ = nullptr;
};

// class SmallBlurryImage (include/ImageProcess.h, src/ImageProcess.cc:255-495), device-resident.  The Jacobians are made with the
// image (there is no MakeJacs to call); the camera is the Context's.
class SmallBlurryImage {
public:
    explicit SmallBlurryImage(Context& c) { check(ptam_sbi_create(c.handle(), c.size().x, c.size().y, &h_), "ptam_sbi_create"); }
    // SmallBlurryImage(KeyFrame &kf, double dBlur = 2.5)
    SmallBlurryImage(Context& c, KeyFrame& kf, double dBlur = 2.5) : SmallBlurryImage(c) { MakeFromKF(kf, dBlur); }
    ~SmallBlurryImage() { ptam_sbi_destroy(h_); }
    SmallBlurryImage(const SmallBlurryImage&) = delete;
    SmallBlurryImage& operator=(const SmallBlurryImage&) = delete;
    // void MakeFromKF(KeyFrame &kf, double dBlur = 2.5)   src/ImageProcess.cc:279
    void MakeFromKF(KeyFrame& kf, double dBlur = 2.5) { check(ptam_sbi_make(h_, kf.handle(), dBlur), "ptam_sbi_make"); }
    // std::pair<SE3<>, double> CalcSBIRotation(SmallBlurryImage *pSBIRef, ATANCamera camera, int nIterations = 6)   :485
    std::pair<SE3, double> CalcSBIRotation(SmallBlurryImage* pSBIRef, int nIterations = 6, ptam_sbi_alignment* pAlignment = nullptr) {
        ptam_sbi_alignment a;
        check(ptam_sbi_calc_rotation(h_, pSBIRef->h_, nIterations, &a), "ptam_sbi_calc_rotation");
        if (pAlignment) *pAlignment = a;
        SE3 r = SE3::Identity();
        std::memcpy(r.R, a.rotation, sizeof r.R);
        return {r, a.score};
    }
    ImageRef GetSize() const {   // mirSize
        ImageRef s{0, 0};
        check(ptam_sbi_size(h_, &s.x, &s.y), "ptam_sbi_size");
        return s;
    }
    ptam_sbi* handle() const { return h_; }

private:
    ptam_sbi* h_ = nullptr;
};

// class Relocaliser (include/Relocaliser.h, src/Relocaliser.cc:12-38).  The reference walks Map::vpKeyFrames and their pSBI; here
// the map's keyframes are handed over as they are made (AddKeyFrame = the pSBI lines of MakeKeyFrame_Rest, src/KeyFrame.cc:80-81).
class Relocaliser {
public:
    Relocaliser(Context& c, int nMaxKeyFrames) : scratch_(c) {
        check(ptam_sbi_bank_create(c.handle(), c.size().x, c.size().y, nMaxKeyFrames, &h_), "ptam_sbi_bank_create");
    }
    ~Relocaliser() { ptam_sbi_bank_destroy(h_); }
    Relocaliser(const Relocaliser&) = delete;
    Relocaliser& operator=(const Relocaliser&) = delete;
    int AddKeyFrame(KeyFrame& k, double dBlur = 2.5) {   // k.se3CfromW is copied
        int i = -1;
        check(ptam_sbi_bank_add(h_, k.handle(), dBlur, &i), "ptam_sbi_bank_add");
        double p[12];
        k.se3CfromW.to12(p);
        poses_.insert(poses_.end(), p, p + 12);
        check(ptam_sbi_bank_set_poses(h_, i, 1, p), "ptam_sbi_bank_set_poses");
        return i;
    }
    int AddKeyFrames(const std::vector<KeyFrame*>& vKeyFrames, double dBlur = 2.5) {   // a map handed over at once: one launch
        std::vector<const ptam_kf*> h;
        for (KeyFrame* k : vKeyFrames) h.push_back(k->handle());
        int i = -1;
        check(ptam_sbi_bank_add_batch(h_, (int)h.size(), h.data(), dBlur, &i), "ptam_sbi_bank_add_batch");
        for (KeyFrame* k : vKeyFrames) {
            double p[12];
            k->se3CfromW.to12(p);
            poses_.insert(poses_.end(), p, p + 12);
        }
        check(ptam_sbi_bank_set_poses(h_, i, (int)h.size(), &poses_[12 * (size_t)i]), "ptam_sbi_bank_set_poses");
        return i;
    }
    // after a bundle adjustment: the bank keeps the pose on the device and in its mirror (MapTracker::TrackFramesRecoverBatch forms
    // mse3Best there and walks the mirror for the closest keyframe); AttemptRecovery's own table follows
    void SetKeyFramePose(int i, const SE3& se3CfromW) {
        se3CfromW.to12(&poses_[12 * (size_t)i]);
        check(ptam_sbi_bank_set_poses(h_, i, 1, &poses_[12 * (size_t)i]), "ptam_sbi_bank_set_poses");
    }
    // Map::vpKeyFrames of the snapshot's current generation (MapSnapshot::EnableKeyFrames) becomes the bank, device to device: with
    // a ResidentMap this replaces AddKeyFrame / SetKeyFramePose.  Call it beside MapTracker::TakeMap, once per frame: a generation the
    // bank holds already costs one mutex hold.  AttemptRecovery's own table follows the take.
    ptam_keyframes_take_result TakeKeyFrames(class MapSnapshot& snapshot);   // (defined behind MapSnapshot)
    void Clear() {   // Tracker::Reset / a new map: AddKeyFrame works again after a take
        check(ptam_sbi_bank_clear(h_), "ptam_sbi_bank_clear");
        poses_.clear();
    }
    int KeyFrameCount() const {
        int n = 0;
        check(ptam_sbi_bank_count(h_, &n), "ptam_sbi_bank_count");
        return n;
    }
    SE3 KeyFramePose(int i) const {
        double p[12];
        check(ptam_sbi_bank_poses(h_, i, 1, p), "ptam_sbi_bank_poses");
        return SE3::from12(p);
    }
    ptam_sbi_bank* handle() const { return h_; }
    ptam_sbi* scratch() const { return scratch_.handle(); }
    // bool AttemptRecovery(KeyFrame &k)   src/Relocaliser.cc:12; Reloc2.MaxScore = 9e6
    bool AttemptRecovery(KeyFrame& kCurrent, double dMaxScore = 9e6, double dBlur = 2.5) {
        check(ptam_relocalise(h_, scratch_.handle(), kCurrent.handle(), poses_.data(), dBlur, dMaxScore, &last_, nullptr), "ptam_relocalise");
        return last_.good != 0;
    }
    SE3 BestPose() const { return SE3::from12(last_.pose); }   // mse3Best
    int mnBest() const { return last_.best; }
    double mdBestScore() const { return last_.best_ssd; }
    const ptam_reloc_result& Last() const { return last_; }

private:
    SmallBlurryImage scratch_;
    ptam_sbi_bank* h_ = nullptr;
    std::vector<double> poses_;
    ptam_reloc_result last_{};
};

// mpSBILastFrame / mpSBIThisFrame of the Tracker (src/Tracker.cc:94-108), for MapTracker::TrackFrame with the estimator
class RotationEstimator {
public:
    explicit RotationEstimator(Context& c, double dBlur = 0.75) {   // Tracker.RotationEstimatorBlur
        check(ptam_rotation_estimator_create(c.handle(), c.size().x, c.size().y, dBlur, &h_), "ptam_rotation_estimator_create");
    }
    ~RotationEstimator() { ptam_rotation_estimator_destroy(h_); }
    RotationEstimator(const RotationEstimator&) = delete;
    RotationEstimator& operator=(const RotationEstimator&) = delete;
    void Reset() { check(ptam_rotation_estimator_reset(h_), "ptam_rotation_estimator_reset"); }   // Tracker::Reset
    ptam_rotation_estimator* handle() const { return h_; }

private:
    ptam_rotation_estimator* h_ = nullptr;
};

// The tracker's state around TrackMap (src/Tracker.cc:52-62): the motion model, mnLostFrames, mTrackingQuality, mnFrame and
// mnLastKeyFrameDropped, for MapTracker::TrackFramesRecoverBatch
struct TrackState : ptam_track_state {
    explicit TrackState(const SE3& se3CfromW = SE3::Identity()) { Reset(se3CfromW); }
    void Reset(const SE3& se3CfromW) {   // Tracker::Reset
        double p[12];
        se3CfromW.to12(p);
        ptam_track_state_reset(this, p);
    }
    bool IsLost() const { return lost_frames >= 3; }                      // :129 / :168
    bool IsGood() const { return quality == PTAM_TRACK_GOOD; }
    void KeyFrameAdded() { last_keyframe_dropped = frame; }               // :165
    // AssessTrackingQuality :1062-1107 on a frame's counts
    void Assess(const ptam_trackmap_result& r, double dClosestKeyFrameDist, const ptam_track_state_opts* pOpts = nullptr) {
        ptam_assess_tracking_quality(this, r.attempted, r.found, dClosestKeyFrameDist, pOpts);
    }
};

// The map as the tracker wants it, in device memory (ptam_map_snapshot, ptam_hip.h): ResidentMap::Publish fills it on the mapmaker's
// thread, MapTracker::TakeMap copies from it on the tracker's.  Three slots and a mutex on the host: neither thread waits for the
// other's device work, and nothing table-sized crosses the host link.  Create it before the threads start; it must outlive both.
class MapSnapshot {
public:
    MapSnapshot(Context& c, int nMaxPoints) { check(ptam_map_snapshot_create(c.handle(), nMaxPoints, &h_), "ptam_map_snapshot_create"); }
    ~MapSnapshot() { ptam_map_snapshot_destroy(h_); }
    MapSnapshot(const MapSnapshot&) = delete;
    MapSnapshot& operator=(const MapSnapshot&) = delete;
    void Reserve(int nMaxPoints) { check(ptam_map_snapshot_reserve(h_, nMaxPoints), "ptam_map_snapshot_reserve"); }
    // the current generation (0: never published into), its map and its point count
    ptam_map_snapshot_info_t Info() const {
        ptam_map_snapshot_info_t r{};
        check(ptam_map_snapshot_info(h_, &r), "ptam_map_snapshot_info");
        return r;
    }
    // Every Publish also carries Map::vpKeyFrames as the relocaliser reads it — se3CfromW and pSBI (src/KeyFrame.cc:80-81) of every
    // keyframe — for Relocaliser::TakeKeyFrames.  The publisher's thread, before the threads start or between two Publish calls.
    void EnableKeyFrames(int nMaxKeyFrames, double dBlur = 2.5) {
        check(ptam_snapshot_keyframes_enable(h_, nMaxKeyFrames, dBlur), "ptam_snapshot_keyframes_enable");
    }
    ptam_snapshot_keyframes_info_t KeyFrames() const {
        ptam_snapshot_keyframes_info_t r{};
        check(ptam_snapshot_keyframes_info(h_, &r), "ptam_snapshot_keyframes_info");
        return r;
    }
    ptam_map_snapshot* handle() const { return h_; }

private:
    ptam_map_snapshot* h_ = nullptr;
};

inline ptam_keyframes_take_result Relocaliser::TakeKeyFrames(MapSnapshot& snapshot) {
    ptam_keyframes_take_result r{};
    check(ptam_sbi_bank_take_keyframes(h_, snapshot.handle(), &r), "ptam_sbi_bank_take_keyframes");
    if (r.changed) {
        poses_.resize(12 * (size_t)r.n_kf);
        if (r.n_kf > 0) check(ptam_sbi_bank_poses(h_, 0, r.n_kf, poses_.data()), "ptam_sbi_bank_poses");
    }
    return r;
}

// One tracked frame for the mapmaker, in device memory (ptam_frame_report, ptam_hip.h): the found entries of the frame's iteration
// set as records sorted by point serial.  MapTracker::ReportFrame fills it on the tracker's thread (one launch, one wait); the host
// hands it over — a queue and a pool of reports are the caller's, as mvpKeyFrameQueue is the reference's — and ResidentMap::NoteTracked /
// InsertKeyFrame consume it on the mapmaker's thread without a record crossing the host link.  No lock is kept: do not refill or
// destroy a report that the other thread is still consuming.
class FrameReport {
public:
    FrameReport(Context& c, int nMaxRecords) { check(ptam_frame_report_create(c.handle(), nMaxRecords, &h_), "ptam_frame_report_create"); }
    ~FrameReport() { ptam_frame_report_destroy(h_); }
    FrameReport(const FrameReport&) = delete;
    FrameReport& operator=(const FrameReport&) = delete;
    // map_id (0: empty), the caller's tag, n_records, n_entries, n_outliers
    ptam_frame_report_info_t Info() const {
        ptam_frame_report_info_t r{};
        check(ptam_frame_report_info(h_, &r), "ptam_frame_report_info");
        return r;
    }
    // the records, for drawing and for hosts that keep MapPoint objects; nCount < 0: from nFirst to the end
    std::vector<ptam_frame_record> Read(int nFirst = 0, int nCount = -1) const {
        if (nCount < 0) nCount = Info().n_records - nFirst;
        std::vector<ptam_frame_record> v((size_t)(nCount > 0 ? nCount : 0));
        check(ptam_frame_report_read(h_, nFirst, nCount, v.data()), "ptam_frame_report_read");
        return v;
    }
    // the same device core for a host whose tracker is not a MapTracker: its map's serial list, its iteration set in its numbering
    void FromHost(int64_t nMapId, const std::vector<int64_t>& vPointSerials, const std::vector<ptam_trackmap_meas>& vEntries) {
        check(ptam_frame_report_from_host(h_, nMapId, (int)vPointSerials.size(), vPointSerials.data(), (int)vEntries.size(), vEntries.data()),
              "ptam_frame_report_from_host");
    }
    ptam_frame_report* handle() const { return h_; }

private:
    ptam_frame_report* h_ = nullptr;
};

// Tracker::TrackMap (src/Tracker.cc:442-696) as one device-resident chain: the map (world positions, pixel vectors, patch
// sources) lives on the device between frames; a frame is one call that returns the refined pose, mbDidCoarse, the
// per-level manMeasAttempted / manMeasFound counters and the scene-depth sums.  The caller keeps what is host logic in the
// reference: the bTryCoarse heuristics (:505-516), the motion model, the tracking-quality assessment, and the two random
// orders per frame (SetShuffle: permutations of the map indices that replace std::random_shuffle, :483-484 and :598).
class MapTracker {
public:
    MapTracker(Context& c, int nMaxPoints) : c_(c) { check(ptam_tracker_create(c.handle(), nMaxPoints, &h_), "ptam_tracker_create"); }
    ~MapTracker() { ptam_tracker_destroy(h_); }
    MapTracker(const MapTracker&) = delete;
    MapTracker& operator=(const MapTracker&) = delete;
    // vSources[i]: src_kf / src_level / center_x / center_y of map point i (MapPoint::pPatchSourceKF, nSourceLevel, irCenter)
    void SetMap(const std::vector<ptam_pvs_point>& vMapPoints, const std::vector<ptam_template_query>& vSources) {
        check(ptam_tracker_set_map(h_, (int)vMapPoints.size(), vMapPoints.data(), vSources.data()), "ptam_tracker_set_map");
    }
    // The map after the mapmaker changed it: vPrevIndex[i] = index of point i in the map handed over last time, -1 for a new
    // point.  Persisting points keep their TrackerData (PatchFinder template, warp, mbTemplateBad) as in the reference.
    void UpdateMap(const std::vector<ptam_pvs_point>& vMapPoints, const std::vector<ptam_template_query>& vSources,
                   const std::vector<int32_t>& vPrevIndex) {
        if (vSources.size() != vMapPoints.size() || vPrevIndex.size() != vMapPoints.size()) throw std::runtime_error("UpdateMap: sizes differ");
        check(ptam_tracker_update_map(h_, (int)vMapPoints.size(), vMapPoints.data(), vSources.data(), vPrevIndex.data()), "ptam_tracker_update_map");
    }
    // The map after the mapmaker published it (ResidentMap::Publish), device to device: points the tracker knows by their serial
    // keep their TrackerData, whatever was removed or appended in between and however many publishes the tracker skipped.
    // changed == 0: the tracker holds this generation already and nothing was done — call it every frame.  When the point count
    // changed the shuffles are the identity again: SetShuffle before the next frame.
    ptam_map_take_result TakeMap(MapSnapshot& snapshot) {
        ptam_map_take_result r{};
        check(ptam_tracker_take_map(h_, snapshot.handle(), &r), "ptam_tracker_take_map");
        return r;
    }
    // the serials of the map's points after TakeMap (none after SetMap / UpdateMap); nCount < 0: nTotal points from nFirst on
    std::vector<int64_t> PointSerials(int nTotal, int nFirst = 0, int nCount = -1) {
        if (nCount < 0) nCount = nTotal - nFirst;
        std::vector<int64_t> v((size_t)(nCount > 0 ? nCount : 0));
        check(ptam_tracker_point_serials(h_, nFirst, nCount, v.data()), "ptam_tracker_point_serials");
        return v;
    }
    void SetShuffle(const std::vector<int32_t>& vLevels, const std::vector<int32_t>& vFine) {
        check(ptam_tracker_set_shuffle(h_, vLevels.data(), vFine.data()), "ptam_tracker_set_shuffle");
    }
    // The two orders drawn on the device instead (ptam_tracker_draw_shuffles): asynchronous on the tracker's queue, nothing the size
    // of the map is made or sent by the host.  ShuffleOrder is what they are, in host code.
    void DrawShuffles(uint64_t nSeed, uint64_t nFrame) { check(ptam_tracker_draw_shuffles(h_, nSeed, nFrame), "ptam_tracker_draw_shuffles"); }
    static std::vector<int32_t> ShuffleOrder(uint64_t nSeed, uint64_t nFrame, int nWhich, int nPoints) {
        std::vector<int32_t> v((size_t)(nPoints > 0 ? nPoints : 0));
        check(ptam_shuffle_order_host(nSeed, nFrame, nWhich, nPoints, v.data()), "ptam_shuffle_order_host");
        return v;
    }
    // the orders the next frame will use, however they were set (nPoints: the map's size)
    void ReadShuffle(int nPoints, std::vector<int32_t>& vLevels, std::vector<int32_t>& vFine) {
        vLevels.assign((size_t)(nPoints > 0 ? nPoints : 1), 0);
        vFine.assign(vLevels.size(), 0);
        check(ptam_tracker_read_shuffle(h_, vLevels.data(), vFine.data()), "ptam_tracker_read_shuffle");
        vLevels.resize((size_t)(nPoints > 0 ? nPoints : 0));
        vFine.resize(vLevels.size());
    }
    ptam_trackmap_result TrackMap(KeyFrame& kfCurrent, const SE3& se3Predicted, const ptam_trackmap_opts* pOpts = nullptr) {
        double in[12];
        se3Predicted.to12(in);
        ptam_trackmap_result r;
        check(ptam_track_map(h_, kfCurrent.handle(), in, pOpts, &r), "ptam_track_map");
        return r;
    }
    // The frame arrives with its image (device-resident, stride == width): MakeKeyFrame_Lite of it into kfCurrent + TrackMap
    ptam_trackmap_result TrackFrame(KeyFrame& kfCurrent, const uint8_t* dFrame, const SE3& se3Predicted, const ptam_trackmap_opts* pOpts = nullptr) {
        double in[12];
        se3Predicted.to12(in);
        ptam_trackmap_result r;
        check(ptam_track_map_frame(h_, kfCurrent.handle(), dFrame, in, pOpts, &r), "ptam_track_map_frame");
        return r;
    }
    // The tracking branch of Tracker::TrackFrame (src/Tracker.cc:94, :134-137) for a camera that moves: MakeKeyFrame_Lite of the
    // device-resident frame, PredictPoseWithMotionModel, the bTryCoarse heuristics, TrackMap, UpdateMotionModel.  `motion` is the
    // tracker's model (ptam_motion_reset at Tracker::Reset; motion.just_recovered = 1 after a recovery); motion.pose is
    // mse3CamFromWorld afterwards.
    ptam_trackmap_result TrackFrame(KeyFrame& kfCurrent, const uint8_t* dFrame, ptam_motion_model& motion, const ptam_trackmap_opts* pOpts = nullptr) {
        ptam_trackmap_result r;
        check(ptam_track_frame(h_, kfCurrent.handle(), dFrame, &motion, pOpts, &r), "ptam_track_frame");
        return r;
    }
    // The same with Tracker.UseRotationEstimator = 1, the reference's default (:94-108, :1016-1028): the prediction's rotation comes
    // from the SmallBlurryImages of this frame and the last (ptam_track_frame_sbi).  After Relocaliser::AttemptRecovery succeeded:
    // ptam_motion_recover(&motion, pose) (:196-207), then this.
    ptam_trackmap_result TrackFrame(KeyFrame& kfCurrent, const uint8_t* dFrame, ptam_motion_model& motion, RotationEstimator& estimator,
                                    const ptam_trackmap_opts* pOpts = nullptr, ptam_sbi_alignment* pAlignment = nullptr) {
        ptam_trackmap_result r;
        check(ptam_track_frame_sbi(h_, kfCurrent.handle(), dFrame, &motion, estimator.handle(), pOpts, &r, pAlignment), "ptam_track_frame_sbi");
        return r;
    }
    // Several cameras (or agents) on one device: ONE chain of launches for all their frames, results as the single calls give
    // them (ptam_track_map_frames_batch).  The trackers live in different Contexts with the same camera model and image size;
    // SetShuffle each of them first.
    static std::vector<ptam_trackmap_result> TrackFramesBatch(const std::vector<MapTracker*>& vTrackers, const std::vector<KeyFrame*>& vCurrent,
                                                              const std::vector<const uint8_t*>& vdFrames, const std::vector<SE3>& vPredicted,
                                                              const ptam_trackmap_opts* pOpts = nullptr) {
        const size_t n = vTrackers.size();
        if (n == 0 || vCurrent.size() != n || vdFrames.size() != n || vPredicted.size() != n) throw std::runtime_error("TrackFramesBatch: sizes differ");
        std::vector<ptam_tracker*> t(n);
        std::vector<ptam_kf*> k(n);
        std::vector<double> poses(12 * n);
        for (size_t i = 0; i < n; i++) {
            t[i] = vTrackers[i]->h_;
            k[i] = vCurrent[i]->handle();
            vPredicted[i].to12(&poses[12 * i]);
        }
        std::vector<ptam_trackmap_result> r(n);
        check(ptam_track_map_frames_batch((int)n, t.data(), k.data(), vdFrames.data(), poses.data(), pOpts, r.data()), "ptam_track_map_frames_batch");
        return r;
    }
    // The same for cameras that move: per camera the motion model (vMotion[i], advanced in place), the bTryCoarse heuristics and —
    // where vEstimators[i] is not null — the rotation estimator, i.e. TrackFrame(kf, dFrame, motion[, estimator]) for every camera,
    // in one chain of launches with one wait per camera (ptam_track_frames_batch).  vEstimators may be empty (no camera has one).
    // pvInfo (nullable): per camera the pose TrackMap started from, the alignment and the heuristics as applied.  A call that
    // throws leaves every model and every estimator as it was.
    static std::vector<ptam_trackmap_result> TrackFramesBatch(const std::vector<MapTracker*>& vTrackers, const std::vector<KeyFrame*>& vCurrent,
                                                              const std::vector<const uint8_t*>& vdFrames, std::vector<ptam_motion_model>& vMotion,
                                                              const std::vector<RotationEstimator*>& vEstimators, const ptam_trackmap_opts* pOpts = nullptr,
                                                              std::vector<ptam_track_frame_info>* pvInfo = nullptr) {
        const size_t n = vTrackers.size();
        if (n == 0 || vCurrent.size() != n || vdFrames.size() != n || vMotion.size() != n || (!vEstimators.empty() && vEstimators.size() != n))
            throw std::runtime_error("TrackFramesBatch: sizes differ");
        std::vector<ptam_tracker*> t(n);
        std::vector<ptam_kf*> k(n);
        std::vector<ptam_rotation_estimator*> e(n, nullptr);
        for (size_t i = 0; i < n; i++) {
            t[i] = vTrackers[i]->h_;
            k[i] = vCurrent[i]->handle();
            if (!vEstimators.empty() && vEstimators[i]) e[i] = vEstimators[i]->handle();
        }
        std::vector<ptam_trackmap_result> r(n);
        if (pvInfo) pvInfo->assign(n, ptam_track_frame_info{});
        check(ptam_track_frames_batch((int)n, t.data(), k.data(), vdFrames.data(), vMotion.data(), vEstimators.empty() ? nullptr : e.data(), pOpts,
                                      r.data(), pvInfo ? pvInfo->data() : nullptr),
              "ptam_track_frames_batch");
        return r;
    }
    // Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) for every camera, in one chain of launches with one wait per camera
    // (ptam_track_frames_recover_batch): a camera whose state says lost runs vRelocalisers[i]'s AttemptRecovery inside the chain and is
    // tracked from mse3Best in the same call when it is good; AssessTrackingQuality and the keyframe decision follow per camera.
    // vStates advance in place.  vEstimators and vRelocalisers may be empty, their entries null (a relocaliser: of a camera that is
    // not lost — with one, vInfo carries the closest keyframe).  A call that throws leaves every state, estimator and bank as it was.
    static std::vector<ptam_trackmap_result> TrackFramesRecoverBatch(const std::vector<MapTracker*>& vTrackers, const std::vector<KeyFrame*>& vCurrent,
                                                                     const std::vector<const uint8_t*>& vdFrames, std::vector<TrackState>& vStates,
                                                                     const std::vector<RotationEstimator*>& vEstimators,
                                                                     const std::vector<Relocaliser*>& vRelocalisers,
                                                                     std::vector<ptam_track_frame_state_info>& vInfo, const ptam_trackmap_opts* pOpts = nullptr,
                                                                     const ptam_track_state_opts* pStateOpts = nullptr) {
        const size_t n = vTrackers.size();
        if (n == 0 || vCurrent.size() != n || vdFrames.size() != n || vStates.size() != n || (!vEstimators.empty() && vEstimators.size() != n) ||
            (!vRelocalisers.empty() && vRelocalisers.size() != n))
            throw std::runtime_error("TrackFramesRecoverBatch: sizes differ");
        std::vector<ptam_tracker*> t(n);
        std::vector<ptam_kf*> k(n);
        std::vector<ptam_rotation_estimator*> e(n, nullptr);
        std::vector<ptam_sbi_bank*> b(n, nullptr);
        std::vector<ptam_sbi*> s(n, nullptr);
        std::vector<ptam_track_state> st(vStates.begin(), vStates.end());
        for (size_t i = 0; i < n; i++) {
            t[i] = vTrackers[i]->h_;
            k[i] = vCurrent[i]->handle();
            if (!vEstimators.empty() && vEstimators[i]) e[i] = vEstimators[i]->handle();
            if (!vRelocalisers.empty() && vRelocalisers[i]) b[i] = vRelocalisers[i]->handle(), s[i] = vRelocalisers[i]->scratch();
        }
        std::vector<ptam_trackmap_result> r(n);
        vInfo.assign(n, ptam_track_frame_state_info{});
        check(ptam_track_frames_recover_batch((int)n, t.data(), k.data(), vdFrames.data(), st.data(), e.data(), b.data(), s.data(), pOpts, pStateOpts,
                                              r.data(), vInfo.data()),
              "ptam_track_frames_recover_batch");
        for (size_t i = 0; i < n; i++) static_cast<ptam_track_state&>(vStates[i]) = st[i];
        return r;
    }
    // TrackFramesRecoverBatch with every camera's FrameReport filled inside the chain (vReports[i] may be null) and, with vSeeds, the
    // frames' two orders drawn there (frame index: the state's frame) — one call and one wait per camera for what SetShuffle,
    // TrackFramesRecoverBatch and ReportFramesBatch are together (ptam_track_frames_report_batch).  vReportInfo: per camera the report's
    // info and whether it was filled in the chain.  -> false where a report was too small for its frame: everything is delivered, that
    // report is empty.
    static bool TrackFramesReportBatch(const std::vector<MapTracker*>& vTrackers, const std::vector<KeyFrame*>& vCurrent,
                                       const std::vector<const uint8_t*>& vdFrames, std::vector<TrackState>& vStates,
                                       const std::vector<RotationEstimator*>& vEstimators, const std::vector<Relocaliser*>& vRelocalisers,
                                       const std::vector<FrameReport*>& vReports, const std::vector<int64_t>& vTags, const std::vector<uint64_t>& vSeeds,
                                       std::vector<ptam_trackmap_result>& vResults, std::vector<ptam_track_frame_state_info>& vInfo,
                                       std::vector<ptam_track_report_info>& vReportInfo, const ptam_trackmap_opts* pOpts = nullptr,
                                       const ptam_track_state_opts* pStateOpts = nullptr) {
        const size_t n = vTrackers.size();
        if (n == 0 || vCurrent.size() != n || vdFrames.size() != n || vStates.size() != n || (!vEstimators.empty() && vEstimators.size() != n) ||
            (!vRelocalisers.empty() && vRelocalisers.size() != n) || (!vReports.empty() && vReports.size() != n) ||
            (!vTags.empty() && vTags.size() != n) || (!vSeeds.empty() && vSeeds.size() != n))
            throw std::runtime_error("TrackFramesReportBatch: sizes differ");
        std::vector<ptam_tracker*> t(n);
        std::vector<ptam_kf*> k(n);
        std::vector<ptam_rotation_estimator*> e(n, nullptr);
        std::vector<ptam_sbi_bank*> b(n, nullptr);
        std::vector<ptam_sbi*> s(n, nullptr);
        std::vector<ptam_frame_report*> rp(n, nullptr);
        std::vector<ptam_track_state> st(vStates.begin(), vStates.end());
        for (size_t i = 0; i < n; i++) {
            t[i] = vTrackers[i]->h_;
            k[i] = vCurrent[i]->handle();
            if (!vEstimators.empty() && vEstimators[i]) e[i] = vEstimators[i]->handle();
            if (!vRelocalisers.empty() && vRelocalisers[i]) b[i] = vRelocalisers[i]->handle(), s[i] = vRelocalisers[i]->scratch();
            if (!vReports.empty() && vReports[i]) rp[i] = vReports[i]->handle();
        }
        vResults.assign(n, ptam_trackmap_result{});
        vInfo.assign(n, ptam_track_frame_state_info{});
        vReportInfo.assign(n, ptam_track_report_info{});
        const int rc = ptam_track_frames_report_batch((int)n, t.data(), k.data(), vdFrames.data(), st.data(), e.data(), b.data(), s.data(), pOpts,
                                                      pStateOpts, vResults.data(), vInfo.data(), rp.data(), vTags.empty() ? nullptr : vTags.data(),
                                                      vSeeds.empty() ? nullptr : vSeeds.data(), vReportInfo.data());
        bool delivered = rc == PTAM_OK;   // ... or PTAM_E_ARG with a report marked too small (a refused call writes no info)
        for (size_t i = 0; i < n && rc == PTAM_E_ARG; i++) delivered = delivered || vReportInfo[i].report_too_small != 0;
        if (!delivered) check(rc, "ptam_track_frames_report_batch");
        for (size_t i = 0; i < n; i++) static_cast<ptam_track_state&>(vStates[i]) = st[i];
        return rc == PTAM_OK;
    }
    // vIterationSet of the last frame: what :667-676 turns into mCurrentKF.mMeasurements and what routes the outlier flags
    // back to MapPoint::nMEstimatorOutlierCount
    std::vector<ptam_trackmap_meas> IterationSet() {
        int n = 0;
        check(ptam_tracker_read_iteration_set(h_, nullptr, 0, &n), "ptam_tracker_read_iteration_set");
        std::vector<ptam_trackmap_meas> v((size_t)n);
        if (n > 0) check(ptam_tracker_read_iteration_set(h_, v.data(), n, &n), "ptam_tracker_read_iteration_set");
        return v;
    }
    // the serial of every entry of IterationSet(), in its order: ResidentMap::ResolveSerials turns them into the map's numbering
    // of the moment, for NoteTracked and the rows of InsertKeyFrame (the map came from TakeMap)
    std::vector<int64_t> IterationSerials() {
        int n = 0;
        check(ptam_tracker_read_iteration_serials(h_, nullptr, 0, &n), "ptam_tracker_read_iteration_serials");
        std::vector<int64_t> v((size_t)n);
        if (n > 0) check(ptam_tracker_read_iteration_serials(h_, v.data(), n, &n), "ptam_tracker_read_iteration_serials");
        return v;
    }
    // The frame tracked last into `report`, on the device (the map came from TakeMap): what CalcPoseUpdate's counts (:989-997) and
    // mCurrentKF.mMeasurements (:667-676) are made from.  One launch and one wait; nTag: e.g. the frame number.
    ptam_frame_report_info_t ReportFrame(FrameReport& report, int64_t nTag = 0) {
        ptam_frame_report* r = report.handle();
        check(ptam_tracker_report_frames(1, &h_, &r, &nTag), "ptam_tracker_report_frames");
        return report.Info();
    }
    // ... for the cameras of a batch: still one launch and one wait
    static void ReportFramesBatch(const std::vector<MapTracker*>& vTrackers, const std::vector<FrameReport*>& vReports,
                                  const std::vector<int64_t>& vTags = {}) {
        const size_t n = vTrackers.size();
        if (n == 0 || vReports.size() != n || (!vTags.empty() && vTags.size() != n)) throw std::runtime_error("ReportFramesBatch: sizes differ");
        std::vector<ptam_tracker*> t(n);
        std::vector<ptam_frame_report*> r(n);
        for (size_t i = 0; i < n; i++) {
            t[i] = vTrackers[i]->h_;
            r[i] = vReports[i]->handle();
        }
        check(ptam_tracker_report_frames((int)n, t.data(), r.data(), vTags.empty() ? nullptr : vTags.data()), "ptam_tracker_report_frames");
    }

private:
    Context& c_;
    ptam_tracker* h_ = nullptr;
};

// MapMaker::ReFind_Common (src/MapMaker.cc:943-1020) over the candidate points of one keyframe (the loop body of
// ReFindInSingleKeyFrame :1027-1042): out[i].found -> add Measurement{nLevel = level, v2RootPos = root_pos, bSubPix =
// sub_pix, Source = SRC_REFIND} and insert into sMeasurementKFs; out[i].never_retry -> insert into sNeverRetryKFs.
// The caller filters the points exactly as :947-948 does (already measured / never retry) before the call.
inline std::vector<ptam_refind_result> ReFindInKeyFrame(Context& c, KeyFrame& k, const SE3& se3CfromW,
                                                        const std::vector<ptam_pvs_point>& vPoints,
                                                        const std::vector<ptam_template_query>& vSources) {
    double pose[12];
    se3CfromW.to12(pose);
    std::vector<ptam_refind_result> out(vPoints.size());
    check(ptam_refind_batch(c.handle(), k.handle(), pose, (int)vPoints.size(), vPoints.data(), vSources.data(), out.data()),
          "ptam_refind_batch");
    return out;
}

// The `static PatchFinder Finder` of MapMaker::ReFind_Common (src/MapMaker.cc:977) and the loops that drive it pair by pair:
// ReFindNewlyMade (:1046-1066: one new point against every keyframe in turn) and ReFindFromFailureQueue (:1070-1082: the
// sorted (keyframe, point) pairs).  The caller lists the pairs in the reference's order — with `skip` set where :947-948
// would return at once — and applies out[i] as for ReFindInKeyFrame above.  One ReFinder per MapMaker: its state (last
// template, last warp, mbTemplateBad) carries from call to call exactly like the static's.
class ReFinder {
public:
    explicit ReFinder(Context& c) : c_(c) { check(ptam_refinder_create(c.handle(), &h_), "ptam_refinder_create"); }
    ~ReFinder() { ptam_refinder_destroy(h_); }
    ReFinder(const ReFinder&) = delete;
    ReFinder& operator=(const ReFinder&) = delete;
    std::vector<ptam_refind_result> Find(const std::vector<ptam_refind_pair>& vPairs, std::vector<int32_t>* pvTemplateKept = nullptr) {
        std::vector<ptam_refind_result> out(vPairs.size());
        if (pvTemplateKept) pvTemplateKept->assign(vPairs.size(), 0);
        check(ptam_refind_pairs(c_.handle(), h_, (int)vPairs.size(), vPairs.data(), out.data(), pvTemplateKept ? pvTemplateKept->data() : nullptr),
              "ptam_refind_pairs");
        return out;
    }
    ptam_refinder* handle() const { return h_; }

private:
    Context& c_;
    ptam_refinder* h_ = nullptr;
};

// int MapMaker::ReFindInSingleKeyFrame(KeyFrame&) / void ReFindNewlyMade() / void ReFindFromFailureQueue()   src/MapMaker.cc:1028-1081
// in ONE device call (ptam_map_refind) for a host that keeps its map as tables: vpKeyFrames in map order with their se3CfromW,
// vPoints in vpPoints order (patch source as a keyframe index), vMeas as MapBundleAdjust takes it, vNever = every sNeverRetryKFs
// entry, both sorted by (kf, point).  pWork / nWork per mode (ptam_hip.h): the keyframe index | the new points in queue order |
// the failure queue as it stands.  The set tests of :947-948, the pair records and the search run on the device through
// `finder`.  The caller applies vFound[i] (k.mMeasurements[&p] = {level, root_pos, bSubPix = vFoundSubPix[i], SRC_REFIND};
// p.sMeasurementKFs.insert(&k)) and vNeverNew[i] (p.sNeverRetryKFs.insert(&k)) — or simply takes vMeas / vNever, which come back
// merged and sorted when bMerge is set.  pbStop: mvpKeyFrameQueue.empty() turned false (:1053), looked at between passes.
struct MapReFindResult {
    ptam_map_refind_result result;
    std::vector<ptam_map_meas> vFound;       // visiting order
    std::vector<int32_t> vFoundSubPix;
    std::vector<ptam_map_pair> vNeverNew;    // visiting order
};
inline MapReFindResult MapReFind(Context& c, ReFinder& finder, int mode, const std::vector<const KeyFrame*>& vpKeyFrames,
                                 const std::vector<SE3>& vKFPoses, const std::vector<ptam_map_refind_point>& vPoints,
                                 std::vector<ptam_map_meas>& vMeas, std::vector<ptam_map_pair>& vNever, const void* pWork, int nWork,
                                 bool bMerge = true, const bool* pbStop = nullptr, const ptam_map_refind_opts* opts = nullptr) {
    if (vpKeyFrames.size() != vKFPoses.size()) throw std::runtime_error("MapReFind: one pose per keyframe");
    std::vector<const ptam_kf*> kfs;
    for (const KeyFrame* k : vpKeyFrames) kfs.push_back(k ? k->handle() : nullptr);
    const size_t cap = mode == PTAM_MAP_REFIND_KEYFRAME ? (nWork > 0 ? vPoints.size() : 0)
                       : mode == PTAM_MAP_REFIND_NEW_POINTS ? kfs.size() * (size_t)(nWork > 0 ? nWork : 0) : (size_t)(nWork > 0 ? nWork : 0);
    MapReFindResult r{};
    r.vFound.resize(cap);
    r.vFoundSubPix.resize(cap);
    r.vNeverNew.resize(cap);
    std::vector<ptam_map_meas> mm(bMerge ? vMeas.size() + cap : 0);
    std::vector<ptam_map_pair> nm(bMerge ? vNever.size() + cap : 0);
    check(ptam_map_refind(c.handle(), finder.handle(), opts, mode, (int)kfs.size(), kfs.data(), reinterpret_cast<const double*>(vKFPoses.data()),
                          (int)vPoints.size(), vPoints.data(), (int)vMeas.size(), vMeas.data(), (int)vNever.size(), vNever.data(), nWork, pWork,
                          reinterpret_cast<const volatile unsigned char*>(pbStop), &r.result, r.vFound.data(), r.vFoundSubPix.data(),
                          r.vNeverNew.data(), (int)cap, bMerge ? mm.data() : nullptr, bMerge ? nm.data() : nullptr),
          "ptam_map_refind");
    r.vFound.resize((size_t)r.result.n_found);
    r.vFoundSubPix.resize((size_t)r.result.n_found);
    r.vNeverNew.resize((size_t)r.result.n_never);
    if (bMerge) {
        mm.resize(vMeas.size() + r.vFound.size());
        nm.resize(vNever.size() + r.vNeverNew.size());
        vMeas.swap(mm);
        vNever.swap(nm);
    }
    return r;
}

// The edits of the tables between the calls above, each in ONE device call, for a host that keeps its map as tables (ptam_hip.h).
//
// The outlier loop of MapMaker::BundleAdjust   src/MapMaker.cc:916-932 (ptam_map_apply_outliers): vOutliers as MapBundleAdjust
// returned them for this vMeas.  vBad (bBad per point), vMeas, vNever and vFailureQueue (mvFailureQueue) are updated in place:
// POINT_BAD sets vBad, FAILURE_QUEUE appends the pair to the queue and erases the row, NEVER_RETRY moves the pair into vNever.
inline ptam_map_outliers_result ApplyBundleOutliers(Context& c, int nKeyFrames, std::vector<uint8_t>& vBad, std::vector<ptam_map_meas>& vMeas,
                                                    std::vector<ptam_map_pair>& vNever, std::vector<ptam_map_pair>& vFailureQueue,
                                                    const std::vector<ptam_map_outlier>& vOutliers) {
    ptam_map_outliers_result r{};
    std::vector<ptam_map_meas> mo(vMeas.size());
    std::vector<ptam_map_pair> no(vNever.size() + vOutliers.size()), fo(vFailureQueue.size() + vOutliers.size());
    check(ptam_map_apply_outliers(c.handle(), nKeyFrames, (int)vBad.size(), (int)vMeas.size(), vMeas.data(), (int)vNever.size(), vNever.data(),
                                  (int)vFailureQueue.size(), vFailureQueue.data(), (int)vOutliers.size(), vOutliers.data(), vBad.data(), &r,
                                  mo.data(), no.data(), fo.data()),
          "ptam_map_apply_outliers");
    mo.resize((size_t)r.n_meas_out);
    no.resize((size_t)r.n_never_out);
    fo.resize((size_t)r.n_failure_out);
    vMeas.swap(mo);
    vNever.swap(no);
    vFailureQueue.swap(fo);
    return r;
}

// void MapMaker::HandleBadPoints()   src/MapMaker.cc:131-153 with Map::MoveBadPointsToTrash (src/Map.cc:20-30)
// (ptam_map_handle_bad_points).  vBad: bBad per point; pOutlierCount / pInlierCount (nullable together): nMEstimatorOutlierCount /
// nMEstimatorInlierCount per point.  vMeas, vNever, vNewQueue (mqNewQueue as point indices) and vFailureQueue are rewritten in
// place with the removed points gone and the later ones renumbered; every column (a point-side table: data, bytes per row) is
// compacted in place, and the caller shrinks it to result.n_kept rows — vBad included if it is handed over as a column.
// vKept[j] = survivor j's old index = the prevIndex of MapTracker::UpdateMap; vNewIndex[i] = -1 for a removed point.
struct HandleBadPointsResult {
    ptam_map_bad_points_result result;
    std::vector<int32_t> vNewIndex, vKept;
};
inline HandleBadPointsResult HandleBadPoints(Context& c, int nKeyFrames, const std::vector<uint8_t>& vBad, const int32_t* pOutlierCount,
                                             const int32_t* pInlierCount, std::vector<ptam_map_meas>& vMeas, std::vector<ptam_map_pair>& vNever,
                                             std::vector<int32_t>& vNewQueue, std::vector<ptam_map_pair>& vFailureQueue,
                                             const std::vector<ptam_map_column>& vColumns = {}) {
    HandleBadPointsResult r{};
    r.vNewIndex.resize(vBad.size());
    r.vKept.resize(vBad.size());
    std::vector<ptam_map_meas> mo(vMeas.size());
    std::vector<ptam_map_pair> no(vNever.size()), fo(vFailureQueue.size());
    std::vector<int32_t> qo(vNewQueue.size());
    check(ptam_map_handle_bad_points(c.handle(), nKeyFrames, (int)vBad.size(), vBad.data(), pOutlierCount, pInlierCount, (int)vMeas.size(),
                                     vMeas.data(), (int)vNever.size(), vNever.data(), (int)vNewQueue.size(), vNewQueue.data(),
                                     (int)vFailureQueue.size(), vFailureQueue.data(), (int)vColumns.size(), vColumns.data(), &r.result,
                                     r.vNewIndex.data(), r.vKept.data(), mo.data(), no.data(), qo.data(), fo.data()),
          "ptam_map_handle_bad_points");
    r.vKept.resize((size_t)r.result.n_kept);
    mo.resize((size_t)r.result.n_meas_out);
    no.resize((size_t)r.result.n_never_out);
    qo.resize((size_t)r.result.n_new_out);
    fo.resize((size_t)r.result.n_failure_out);
    vMeas.swap(mo);
    vNever.swap(no);
    vNewQueue.swap(qo);
    vFailureQueue.swap(fo);
    return r;
}

// The table side of MapMaker::AddPointEpipolar   src/MapMaker.cc:670-685 (nTargetSource PTAM_MAP_SRC_EPIPOLAR, vMade from
// AddMapPointsEpipolar) and of InitFromStereo's point loop :352-362 (PTAM_MAP_SRC_TRAIL, vMade from InitPointsFromTrails)
// (ptam_map_add_points): new point i gets index nPoints + i, vMeas gets its two rows in place, the point-side rows of the new
// points come back for the caller to append to its tables; their indices are mqNewQueue's new entries, in order.
struct AddPointsResult {
    std::vector<ptam_map_refind_point> vPoints;
    std::vector<ptam_map_point_source> vSources;
};
inline AddPointsResult AddPointsToTables(Context& c, int nKeyFrames, int nPoints, std::vector<ptam_map_meas>& vMeas, int nSrcKF, int nTargetKF,
                                         const std::vector<ptam_new_map_point>& vMade, int nTargetSource = PTAM_MAP_SRC_EPIPOLAR) {
    AddPointsResult r{};
    r.vPoints.resize(vMade.size());
    r.vSources.resize(vMade.size());
    std::vector<ptam_map_meas> mo(vMeas.size() + 2 * vMade.size());
    check(ptam_map_add_points(c.handle(), nKeyFrames, nPoints, (int)vMeas.size(), vMeas.data(), nSrcKF, nTargetKF, nTargetSource, (int)vMade.size(),
                              vMade.data(), mo.data(), r.vPoints.data(), r.vSources.data()),
          "ptam_map_add_points");
    vMeas.swap(mo);
    return r;
}

// The map of the calls above kept in device memory from call to call (ptam_rmap, ptam_hip.h): Upload once, then one method per
// step of MapMaker::run()  src/MapMaker.cc:57-114 — each does what the function of the same name above does, on the resident
// tables, and moves only its small arguments and results over the host link.  Download fetches a table or a row range of it
// (table: PTAM_RMAP_*; T: the row type, e.g. ptam_map_meas, Vec<3>, SE3).  Move-only.
class ResidentMap {
public:
    explicit ResidentMap(Context& c) { check(ptam_rmap_create(c.handle(), &h_), "ptam_rmap_create"); }
    ~ResidentMap() { ptam_rmap_destroy(h_); }
    ResidentMap(const ResidentMap&) = delete;
    ResidentMap& operator=(const ResidentMap&) = delete;
    ResidentMap(ResidentMap&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ResidentMap& operator=(ResidentMap&& o) noexcept {
        if (this != &o) {
            ptam_rmap_destroy(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    void Reserve(int nKeyFrames, int nPoints, int nMeas, int nNever, int nNewQueue, int nFailureQueue) {
        check(ptam_rmap_reserve(h_, nKeyFrames, nPoints, nMeas, nNever, nNewQueue, nFailureQueue), "ptam_rmap_reserve");
    }
    ptam_rmap_counts_t Counts() const {
        ptam_rmap_counts_t n{};
        check(ptam_rmap_counts(h_, &n), "ptam_rmap_counts");
        return n;
    }
    // every table of the map; vpKeyFrames may be empty (no handles are kept), pOutlierCount / pInlierCount null together (zeros)
    void Upload(const std::vector<const KeyFrame*>& vpKeyFrames, const std::vector<SE3>& vKFPoses, const std::vector<uint8_t>& vFixed,
                const std::vector<Vec<3>>& vPoints, const std::vector<ptam_map_refind_point>& vRefindPoints,
                const std::vector<ptam_map_point_source>& vSources, const std::vector<uint8_t>& vBad, const int32_t* pOutlierCount,
                const int32_t* pInlierCount, const std::vector<ptam_map_meas>& vMeas, const std::vector<ptam_map_pair>& vNever,
                const std::vector<int32_t>& vNewQueue, const std::vector<ptam_map_pair>& vFailureQueue) {
        if (vFixed.size() != vKFPoses.size() || (!vpKeyFrames.empty() && vpKeyFrames.size() != vKFPoses.size()))
            throw std::runtime_error("ResidentMap::Upload: one bFixed (and one handle, if any) per keyframe");
        if (vRefindPoints.size() != vPoints.size() || vSources.size() != vPoints.size() || vBad.size() != vPoints.size())
            throw std::runtime_error("ResidentMap::Upload: one row per point in every point-side table");
        std::vector<const ptam_kf*> kfs;
        for (const KeyFrame* k : vpKeyFrames) kfs.push_back(k->handle());
        check(ptam_rmap_upload(h_, (int)vKFPoses.size(), kfs.empty() ? nullptr : kfs.data(), reinterpret_cast<const double*>(vKFPoses.data()),
                               vFixed.data(), (int)vPoints.size(), reinterpret_cast<const double*>(vPoints.data()), vRefindPoints.data(),
                               vSources.data(), vBad.data(), pOutlierCount, pInlierCount, (int)vMeas.size(), vMeas.data(), (int)vNever.size(),
                               vNever.data(), (int)vNewQueue.size(), vNewQueue.data(), (int)vFailureQueue.size(), vFailureQueue.data()),
              "ptam_rmap_upload");
    }
    template <class T>
    std::vector<T> Download(int table, int first = 0, int count = -1) const {
        static const size_t row[PTAM_RMAP_TABLES] = {96, 1, 24, sizeof(ptam_map_refind_point), sizeof(ptam_map_point_source), 1, 4, 4,
                                                     sizeof(ptam_map_meas), sizeof(ptam_map_pair), 4, sizeof(ptam_map_pair)};
        if (table < 0 || table >= PTAM_RMAP_TABLES || sizeof(T) != row[table]) throw std::runtime_error("ResidentMap::Download: row type");
        const ptam_rmap_counts_t n = Counts();
        const int rows[PTAM_RMAP_TABLES] = {n.n_kf, n.n_kf, n.n_points, n.n_points, n.n_points, n.n_points, n.n_points, n.n_points,
                                            n.n_meas, n.n_never, n.n_new, n.n_failure};
        if (count < 0) count = rows[table] - first;
        std::vector<T> v((size_t)(count > 0 ? count : 0));
        check(ptam_rmap_download(h_, table, first, count, v.data()), "ptam_rmap_download");
        return v;
    }
    void Traffic(unsigned long long& nBytesUp, unsigned long long& nBytesDown) const {
        check(ptam_rmap_traffic(h_, &nBytesUp, &nBytesDown), "ptam_rmap_traffic");
    }
    // MapBundleAdjust on the resident tables: the adjusted poses and points stay on the device
    MapBundleAdjustResult BundleAdjust(int mode, const ptam_ba_opts* opts = nullptr, const volatile unsigned char* abort_flag = nullptr) {
        MapBundleAdjustResult r{};
        const ptam_rmap_counts_t n = Counts();
        r.outliers.resize((size_t)n.n_meas);
        r.cam_kf.resize((size_t)n.n_kf);
        r.point_ids.resize((size_t)n.n_points);
        check(ptam_rmap_bundle_adjust(h_, opts, mode, abort_flag, &r.result, r.outliers.data(), n.n_meas, r.cam_kf.data(), r.point_ids.data()),
              "ptam_rmap_bundle_adjust");
        r.outliers.resize((size_t)r.result.n_outliers);
        r.cam_kf.resize((size_t)(r.result.n_adjust + r.result.n_fixed));
        r.point_ids.resize((size_t)r.result.n_points);
        return r;
    }
    // MapReFind on the resident tables (the keyframe handles are those of Upload / AddKeyFrame).  pWork == nullptr with
    // PTAM_MAP_REFIND_NEW_POINTS / _FAILURE_QUEUE: the resident queue is the work and is popped / cleared.  The merged tables stay
    // on the device; the found rows and new never pairs come down only when bLists is set.
    MapReFindResult ReFind(ReFinder& finder, int mode, const void* pWork = nullptr, int nWork = 0, bool bLists = false,
                           const bool* pbStop = nullptr, const ptam_map_refind_opts* opts = nullptr) {
        const ptam_rmap_counts_t n = Counts();
        const size_t w = pWork ? (size_t)(nWork > 0 ? nWork : 0) : (size_t)(mode == PTAM_MAP_REFIND_NEW_POINTS ? n.n_new : n.n_failure);
        const size_t cap = !bLists ? 0 : mode == PTAM_MAP_REFIND_KEYFRAME ? (w > 0 ? (size_t)n.n_points : 0)
                           : mode == PTAM_MAP_REFIND_NEW_POINTS ? (size_t)n.n_kf * w : w;
        MapReFindResult r{};
        r.vFound.resize(cap);
        r.vFoundSubPix.resize(cap);
        r.vNeverNew.resize(cap);
        check(ptam_rmap_refind(h_, finder.handle(), opts, mode, pWork ? nWork : 0, pWork, reinterpret_cast<const volatile unsigned char*>(pbStop),
                               &r.result, bLists ? r.vFound.data() : nullptr, bLists ? r.vFoundSubPix.data() : nullptr,
                               bLists ? r.vNeverNew.data() : nullptr, (int)cap),
              "ptam_rmap_refind");
        if (bLists) {
            r.vFound.resize((size_t)r.result.n_found);
            r.vFoundSubPix.resize((size_t)r.result.n_found);
            r.vNeverNew.resize((size_t)r.result.n_never);
        }
        return r;
    }
    // BundleAdjust followed by ApplyBundleOutliers on the list it routed, as one call: the list stays on the device
    struct BundleAdjustRoutedResult {
        ptam_map_ba_result result;
        ptam_map_outliers_result outliers;
    };
    BundleAdjustRoutedResult BundleAdjustRouted(int mode, const ptam_ba_opts* opts = nullptr, const volatile unsigned char* abort_flag = nullptr) {
        BundleAdjustRoutedResult r{};
        check(ptam_rmap_bundle_adjust_routed(h_, opts, mode, abort_flag, &r.result, &r.outliers), "ptam_rmap_bundle_adjust_routed");
        return r;
    }
    // ReFind(pWork == nullptr) with the visiting order decided on the device: ReFindNewlyMade (PTAM_MAP_REFIND_NEW_POINTS) or
    // ReFindFromFailureQueue (PTAM_MAP_REFIND_FAILURE_QUEUE) straight from the resident queue, which is popped / cleared
    ptam_map_refind_result ReFindQueue(ReFinder& finder, int mode, const bool* pbStop = nullptr, const ptam_map_refind_opts* opts = nullptr) {
        ptam_map_refind_result r{};
        check(ptam_rmap_refind_queue(h_, finder.handle(), opts, mode, reinterpret_cast<const volatile unsigned char*>(pbStop), &r),
              "ptam_rmap_refind_queue");
        return r;
    }
    // ApplyGlobalTransformationToMap on the resident poses, points and point rows; the ptam_pvs_point rows when bRows is set
    std::vector<ptam_pvs_point> ApplyGlobalTransformationToMap(const SE3& se3NewFromOld, bool bRows = true) {
        std::vector<ptam_pvs_point> rows(bRows ? (size_t)Counts().n_points : 0);
        check(ptam_rmap_apply_global_transform(h_, reinterpret_cast<const double*>(&se3NewFromOld), bRows && !rows.empty() ? rows.data() : nullptr),
              "ptam_rmap_apply_global_transform");
        return rows;
    }
    ptam_map_outliers_result ApplyBundleOutliers(const std::vector<ptam_map_outlier>& vOutliers) {
        ptam_map_outliers_result r{};
        check(ptam_rmap_apply_outliers(h_, (int)vOutliers.size(), vOutliers.data(), &r), "ptam_rmap_apply_outliers");
        return r;
    }
    // vKept (the prevIndex of MapTracker::UpdateMap) comes down when bKept is set; vNewIndex stays empty
    HandleBadPointsResult HandleBadPoints(bool bKept = true) {
        HandleBadPointsResult r{};
        if (bKept) r.vKept.resize((size_t)Counts().n_points);
        check(ptam_rmap_handle_bad_points(h_, &r.result, bKept ? r.vKept.data() : nullptr, nullptr), "ptam_rmap_handle_bad_points");
        if (bKept) r.vKept.resize((size_t)r.result.n_kept);
        return r;
    }
    void AddPointsToTables(int nSrcKF, int nTargetKF, const std::vector<ptam_new_map_point>& vMade, int nTargetSource = PTAM_MAP_SRC_EPIPOLAR) {
        check(ptam_rmap_add_points(h_, nSrcKF, nTargetKF, nTargetSource, (int)vMade.size(), vMade.data()), "ptam_rmap_add_points");
    }
    // the table side of MapMaker::AddKeyFrameFromTopOfQueue   src/MapMaker.cc:501-506: vRows sorted by point
    void AddKeyFrame(const KeyFrame* pK, const SE3& se3CfromW, bool bFixed, const std::vector<ptam_map_kf_row>& vRows) {
        check(ptam_rmap_add_keyframe(h_, pK ? pK->handle() : nullptr, reinterpret_cast<const double*>(&se3CfromW), bFixed, (int)vRows.size(),
                                     vRows.data()),
              "ptam_rmap_add_keyframe");
    }
    // the tracker's iteration set: nMEstimatorOutlierCount++ / nMEstimatorInlierCount++   src/Tracker.cc:987-998
    void NoteTracked(const std::vector<int32_t>& vPoints, const std::vector<uint8_t>& vOutlier) {
        if (vPoints.size() != vOutlier.size()) throw std::runtime_error("ResidentMap::NoteTracked: one flag per point");
        check(ptam_rmap_note_tracked(h_, (int)vPoints.size(), vPoints.data(), vOutlier.data()), "ptam_rmap_note_tracked");
    }
    // ... from frame reports: every record resolved by its serial on the device, so the reports may be older than the last
    // HandleBadPoints (n_gone counts the records of removed points)
    ptam_rmap_note_result NoteTracked(const std::vector<FrameReport*>& vReports) {
        std::vector<ptam_frame_report*> r;
        for (FrameReport* p : vReports) r.push_back(p->handle());
        ptam_rmap_note_result res{};
        check(ptam_rmap_note_reports(h_, (int)r.size(), r.data(), &res), "ptam_rmap_note_reports");
        return res;
    }
    ptam_rmap_note_result NoteTracked(FrameReport& report) { return NoteTracked(std::vector<FrameReport*>{&report}); }
    std::vector<ptam_scene_depth> RefreshSceneDepth() {
        std::vector<ptam_scene_depth> v((size_t)Counts().n_kf);
        check(ptam_rmap_scene_depth(h_, v.data()), "ptam_rmap_scene_depth");
        return v;
    }
    // MapMaker::ClosestKeyFrame / NClosestKeyFrames   src/MapMaker.cc:711-752 on the resident poses: the min(n, keyframes - 1) others
    // nearest to keyframe nKF by (KeyFrameLinearDist, index); pvDist: their distances
    std::vector<int32_t> ClosestKeyFrames(int nKF, int n = 1, std::vector<double>* pvDist = nullptr) {
        const int cap = std::max(std::min(n, Counts().n_kf - 1), 1);
        std::vector<int32_t> v((size_t)cap);
        std::vector<double> d((size_t)cap);
        int32_t got = 0;
        check(ptam_rmap_closest_keyframes(h_, nKF, n, v.data(), d.data(), &got), "ptam_rmap_closest_keyframes");
        v.resize((size_t)got);
        d.resize((size_t)got);
        if (pvDist) *pvDist = d;
        return v;
    }
    // MapMaker::AddKeyFrameFromTopOfQueue   src/MapMaker.cc:493-518 after pK's MakeKeyFrame_Rest, as one call: the keyframe's rows
    // (vRows sorted by point), ReFindInSingleKeyFrame, ClosestKeyFrame, AddSomeMapPoints at opts.epipolar.levels; the new points
    // stay on the device: Download<ptam_map_refind_point>(PTAM_RMAP_REFIND_POINTS, first_point, n_made) are the tracker's rows
    static ptam_rmap_insert_opts InsertOpts(double dDepthMean, double dDepthSigma) {
        ptam_rmap_insert_opts o{};
        ptam_epipolar_opts_default(&o.epipolar);
        o.epipolar.depth_mean = dDepthMean;
        o.epipolar.depth_sigma = dDepthSigma;
        o.target_kf = -1;
        return o;
    }
    ptam_rmap_insert_result InsertKeyFrame(ReFinder& finder, const KeyFrame& k, const SE3& se3CfromW, bool bFixed,
                                           const std::vector<ptam_map_kf_row>& vRows, const ptam_rmap_insert_opts& opts) {
        ptam_rmap_insert_result r{};
        check(ptam_rmap_insert_keyframe(h_, finder.handle(), k.handle(), reinterpret_cast<const double*>(&se3CfromW), bFixed, (int)vRows.size(),
                                        vRows.data(), &opts, &r),
              "ptam_rmap_insert_keyframe");
        return r;
    }
    // ... with the keyframe's rows taken from the frame report of the frame that became the keyframe: resolved, filtered and appended
    // on the device.  pnRows / pnGone: the rows appended, the records whose points are gone.
    ptam_rmap_insert_result InsertKeyFrame(ReFinder& finder, const KeyFrame& k, const SE3& se3CfromW, bool bFixed, FrameReport& report,
                                           const ptam_rmap_insert_opts& opts, int32_t* pnRows = nullptr, int32_t* pnGone = nullptr) {
        ptam_rmap_insert_result r{};
        check(ptam_rmap_insert_keyframe_report(h_, finder.handle(), k.handle(), reinterpret_cast<const double*>(&se3CfromW), bFixed, report.handle(),
                                               &opts, &r, pnRows, pnGone),
              "ptam_rmap_insert_keyframe_report");
        return r;
    }
    // MapMaker::InitFromStereo   src/MapMaker.cc:268-405 as one call: kF / kS the caller's clones of the two keyframes (they become the
    // map's keyframes 0 and 1 and must outlive it), the live trails read on the device.  Returns false where the reference does (no
    // homography, zero baseline, too few points: the previous map stays; stopped: the map is empty); LastInit() says which.
    using InitOpts = ptam_rmap_init_opts;
    static InitOpts InitOptsDefault() {
        InitOpts o;
        ptam_rmap_init_opts_default(&o);
        return o;
    }
    bool InitFromStereo(KeyFrame& kF, KeyFrame& kS, TrailTracker& trails, SE3& se3TrackerPose, const InitOpts& opts,
                        const volatile bool* stop = nullptr) {
        check(ptam_rmap_init_from_stereo(h_, kF.handle(), kS.handle(), trails.handle(), 0, nullptr, &opts,
                                         reinterpret_cast<const volatile unsigned char*>(stop), &init_),
              "ptam_rmap_init_from_stereo");
        return InitDone(kF, kS, se3TrackerPose);
    }
    // ... from the reference's vTrailMatches argument
    bool InitFromStereo(KeyFrame& kF, KeyFrame& kS, const std::vector<ptam_trail>& vTrailMatches, SE3& se3TrackerPose, const InitOpts& opts,
                        const volatile bool* stop = nullptr) {
        check(ptam_rmap_init_from_stereo(h_, kF.handle(), kS.handle(), nullptr, (int)vTrailMatches.size(), vTrailMatches.data(), &opts,
                                         reinterpret_cast<const volatile unsigned char*>(stop), &init_),
              "ptam_rmap_init_from_stereo");
        return InitDone(kF, kS, se3TrackerPose);
    }
    const ptam_rmap_init_result& LastInit() const { return init_; }
    // ApplyGlobalTransformationToMap(CalcPlaneAligner())   src/MapMaker.cc:397 on the resident tables; pvRows: the tracker's rows
    PlaneAligner AlignToPlane(const ptam_plane_opts* opts = nullptr, std::vector<ptam_pvs_point>* pvRows = nullptr) {
        const ptam_plane_opts o = PlaneOptsOrDefault(opts);
        PlaneAligner a;
        double p[12];
        if (pvRows) pvRows->resize((size_t)Counts().n_points);
        check(ptam_rmap_align_to_plane(h_, &o, p, &a.info, pvRows ? pvRows->data() : nullptr), "ptam_rmap_align_to_plane");
        a.se3 = SE3::from12(p);
        return a;
    }
    void Clear() { check(ptam_rmap_clear(h_), "ptam_rmap_clear"); }   // MapMaker::Reset
    // The map as it stands into the snapshot, as its next generation (the mapmaker's thread): after HandleBadPoints, InsertKeyFrame and
    // every accepted bundle.  vKept no longer has to come down for the tracker.  The keyframes need handles (Upload / AddKeyFrame).
    ptam_map_publish_result Publish(MapSnapshot& snapshot) {
        ptam_map_publish_result r{};
        check(ptam_rmap_publish(h_, snapshot.handle(), &r), "ptam_rmap_publish");
        return r;
    }
    // the serial column: one int64 per point, strictly increasing with the index, never reused by this map
    std::vector<int64_t> PointSerials(int nFirst = 0, int nCount = -1) const {
        if (nCount < 0) nCount = Counts().n_points - nFirst;
        std::vector<int64_t> v((size_t)(nCount > 0 ? nCount : 0));
        check(ptam_rmap_point_serials(h_, nFirst, nCount, v.data()), "ptam_rmap_point_serials");
        return v;
    }
    // serials (any order) -> the points' current indices, -1 for a removed point; pnGone: how many of those
    std::vector<int32_t> ResolveSerials(const std::vector<int64_t>& vSerials, int32_t* pnGone = nullptr) {
        std::vector<int32_t> v(vSerials.size());
        check(ptam_rmap_resolve_serials(h_, (int)vSerials.size(), vSerials.data(), v.data(), pnGone), "ptam_rmap_resolve_serials");
        return v;
    }
    ptam_rmap* handle() const { return h_; }

private:
    bool InitDone(KeyFrame& kF, KeyFrame& kS, SE3& se3TrackerPose) {
        if (init_.status != PTAM_INIT_MAP_OK) return false;
        kF.se3CfromW = SE3::Identity();
        kS.se3CfromW = se3TrackerPose = SE3::from12(init_.tracker_pose);
        return true;
    }
    ptam_rmap* h_ = nullptr;
    ptam_rmap_init_result init_{};
};

// class MapMaker   include/MapMaker.h:61, src/MapMaker.cc:57-114 — the mapmaker's thread over a ResidentMap (ptam_mapmaker): the keyframe
// queue, the mbBundleConverged_* flags and one iteration of run() as Step().  AddKeyFrame, NoteFrame, QueueSize, RequestReset,
// ResetDone and Released may be called from the tracker's thread; Step and Run belong to the thread of the map's context.  A
// keyframe clone and a report handed over stay alive until their tag comes back from Released().
class MapMaker {
public:
    MapMaker(ResidentMap& map, ReFinder& finder, MapSnapshot* snapshot = nullptr, const ptam_mapmaker_opts* opts = nullptr) {
        check(ptam_mapmaker_create(map.handle(), finder.handle(), snapshot ? snapshot->handle() : nullptr, opts, &h_), "ptam_mapmaker_create");
    }
    ~MapMaker() { ptam_mapmaker_destroy(h_); }
    MapMaker(const MapMaker&) = delete;
    MapMaker& operator=(const MapMaker&) = delete;
    static ptam_mapmaker_opts DefaultOpts() {
        ptam_mapmaker_opts o;
        check(ptam_mapmaker_opts_default(&o), "ptam_mapmaker_opts_default");
        return o;
    }
    // void MapMaker::AddKeyFrame(KeyFrame &k)   src/MapMaker.cc:480-488: k is the caller's clone
    void AddKeyFrame(const KeyFrame& k, const SE3& se3CfromW, bool bFixed, FrameReport& report, double dSceneDepthMean, double dSceneDepthSigma,
                     int64_t nTag) {
        check(ptam_mapmaker_add_keyframe(h_, k.handle(), reinterpret_cast<const double*>(&se3CfromW), bFixed, report.handle(), dSceneDepthMean,
                                         dSceneDepthSigma, nTag),
              "ptam_mapmaker_add_keyframe");
    }
    void NoteFrame(FrameReport& report, int64_t nTag) { check(ptam_mapmaker_note_frame(h_, report.handle(), nTag), "ptam_mapmaker_note_frame"); }
    int QueueSize() const {
        int32_t n = 0;
        check(ptam_mapmaker_queue_size(h_, &n), "ptam_mapmaker_queue_size");
        return n;
    }
    void RequestReset() { check(ptam_mapmaker_request_reset(h_), "ptam_mapmaker_request_reset"); }
    bool ResetDone() const {
        int32_t n = 0;
        check(ptam_mapmaker_reset_done(h_, &n), "ptam_mapmaker_reset_done");
        return n != 0;
    }
    // bool MapMaker::InitFromStereo(kF, kS, vMatches, se3TrackerPose)   src/MapMaker.cc:268-405, left for the next Step() by the tracker's
    // thread: kFirst / kSecond are the caller's clones (the map names them until the next reset), pOpts nullable (the defaults)
    void RequestInit(const KeyFrame& kFirst, KeyFrame& kSecond, const std::vector<ptam_trail>& vMatches, const ptam_rmap_init_opts* pOpts,
                     int64_t nTag) {
        check(ptam_mapmaker_request_init(h_, kFirst.handle(), kSecond.handle(), (int)vMatches.size(), vMatches.data(), pOpts, nTag),
              "ptam_mapmaker_request_init");
    }
    // PTAM_MM_INIT_NONE / _PENDING / _DONE; DONE: *pResult (nullable) is the request's result, se3TrackerPose in tracker_pose
    int InitPoll(ptam_rmap_init_result* pResult = nullptr) const {
        int32_t s = 0;
        check(ptam_mapmaker_init_poll(h_, &s, pResult), "ptam_mapmaker_init_poll");
        return s;
    }
    std::vector<int64_t> Released() {
        std::vector<int64_t> out, buf(64);
        for (int32_t n = 64; n == 64;) {
            check(ptam_mapmaker_released(h_, 64, buf.data(), &n), "ptam_mapmaker_released");
            out.insert(out.end(), buf.begin(), buf.begin() + n);
        }
        return out;
    }
    // the body of run()'s loop, once (:86-112)
    ptam_mapmaker_step_result Step() {
        ptam_mapmaker_step_result r;
        check(ptam_mapmaker_step(h_, &r), "ptam_mapmaker_step");
        return r;
    }
    // void MapMaker::run()   src/MapMaker.cc:57-114, until `stop` is set, with the reference's sleep(5) (:69)
    void Run(const std::atomic<bool>& stop) {
        while (!stop.load()) {
            std::this_thread::sleep_for(std::chrono::milliseconds(5));
            Step();
        }
    }
    ptam_mapmaker* handle() const { return h_; }

private:
    ptam_mapmaker* h_ = nullptr;
};

// class Tracker   include/Tracker.h, src/Tracker.cc:86-188 for a map that is good (:127-176) — ptam_camera_tracker: one TrackFrame is
// ONE call that takes the published map and its keyframes, draws the frame's random orders, tracks or recovers, fills the frame's
// report inside the chain and hands the frame to the MapMaker (AddKeyFrame with a pooled clone of the current keyframe, or NoteFrame).
// It owns the MapTracker, the current KeyFrame, the rotation estimator, the relocaliser, the state and the pools; it borrows the
// snapshot and the MapMaker, which must outlive it, and lives on the tracker's thread in its own Context.  TrackForInitialMap
// (:181) comes with EnableSession() and PokeTracker(); without them start from ResidentMap::InitFromStereo, a Publish and Reset(the
// tracker's pose).
class Tracker {
public:
    // the reference's options with the Context's image size
    static ptam_camera_tracker_opts DefaultOpts(const Context& c) {
        ptam_camera_tracker_opts o;
        check(ptam_camera_tracker_opts_default(&o), "ptam_camera_tracker_opts_default");
        o.width = c.size().x, o.height = c.size().y;
        return o;
    }
    Tracker(Context& c, MapSnapshot& snapshot, MapMaker& mapmaker, const ptam_camera_tracker_opts* pOpts = nullptr) {
        const ptam_camera_tracker_opts o = pOpts ? *pOpts : DefaultOpts(c);
        check(ptam_camera_tracker_create(c.handle(), &o, snapshot.handle(), mapmaker.handle(), &h_), "ptam_camera_tracker_create");
    }
    ~Tracker() { ptam_camera_tracker_destroy(h_); }
    Tracker(const Tracker&) = delete;
    Tracker& operator=(const Tracker&) = delete;
    // void Tracker::TrackFrame(Image<byte> &imFrame, bool bDraw)   :86 — dFrame: the frame in device memory (stride == width)
    // With EnableSession the frame goes through the session entry: TrackForInitialMap (:181, :311-347) until a map exists, then the
    // same tracking branch; the poke of PokeTracker() is consumed by the frame.  Session(): what the last frame did.
    ptam_camera_track_result TrackFrame(const uint8_t* dFrame) {
        ptam_camera_track_result r;
        if (session_) {
            const uint8_t poke = poke_ ? 1 : 0;
            poke_ = false;
            check(ptam_camera_tracker_session_frames(1, &h_, &dFrame, &poke, &r, &last_), "ptam_camera_tracker_session_frames");
        } else
            check(ptam_camera_tracker_track_frames(1, &h_, &dFrame, &r), "ptam_camera_tracker_track_frames");
        return r;
    }
    // several cameras in ONE chain: Contexts of their own on one device, the same trackmap / state options
    static std::vector<ptam_camera_track_result> TrackFrames(const std::vector<Tracker*>& vTrackers, const std::vector<const uint8_t*>& vdFrames) {
        const size_t n = vTrackers.size();
        if (n == 0 || vdFrames.size() != n) throw std::runtime_error("TrackFrames: sizes differ");
        std::vector<ptam_camera_tracker*> h(n);
        bool session = false;
        for (size_t i = 0; i < n; i++) h[i] = vTrackers[i]->h_, session = session || vTrackers[i]->session_;
        std::vector<ptam_camera_track_result> r(n);
        if (!session) {
            check(ptam_camera_tracker_track_frames((int)n, h.data(), vdFrames.data(), r.data()), "ptam_camera_tracker_track_frames");
            return r;
        }
        std::vector<uint8_t> pokes(n);
        std::vector<ptam_camera_session_result> s(n);
        for (size_t i = 0; i < n; i++) pokes[i] = vTrackers[i]->poke_ ? 1 : 0, vTrackers[i]->poke_ = false;
        check(ptam_camera_tracker_session_frames((int)n, h.data(), vdFrames.data(), pokes.data(), r.data(), s.data()),
              "ptam_camera_tracker_session_frames");
        for (size_t i = 0; i < n; i++) vTrackers[i]->last_ = s[i];
        return r;
    }
    // TrackForInitialMap in the handle (ptam_camera_tracker_enable_session): pOpts nullable (1000 trails, 10 good, 70, the init defaults)
    void EnableSession(const ptam_camera_session_opts* pOpts = nullptr) {
        check(ptam_camera_tracker_enable_session(h_, pOpts), "ptam_camera_tracker_enable_session");
        session_ = true;
    }
    void PokeTracker() { poke_ = true; }   // the GUI command "PokeTracker" (src/Tracker.cc:283-287): mbUserPressedSpacebar for the next frame
    // the tracker's side of Tracker::Reset (:49-65); MapMaker::RequestReset is the caller's, before
    void Restart() {
        check(ptam_camera_tracker_restart(h_), "ptam_camera_tracker_restart");
        poke_ = false;
    }
    const ptam_camera_session_result& Session() const { return last_; }
    int Stage() const {   // mnInitialStage: PTAM_TRAIL_TRACKING_*
        int32_t s = 0;
        check(ptam_camera_tracker_stage(h_, &s), "ptam_camera_tracker_stage");
        return s;
    }
    TrackState State() const {
        TrackState s;
        check(ptam_camera_tracker_state(h_, &s), "ptam_camera_tracker_state");
        return s;
    }
    SE3 GetCurrentPose() const { return SE3::from12(State().model.pose); }   // mse3CamFromWorld
    int Quality() const { return State().quality; }                          // mTrackingQuality: PTAM_TRACK_BAD / PTAM_TRACK_GOOD
    int LostFrames() const { return State().lost_frames; }                   // mnLostFrames
    // void Tracker::Reset()   :52-62 (MapMaker::RequestReset is the caller's, before)
    void Reset(const SE3& se3CfromW = SE3::Identity()) {
        double p[12];
        se3CfromW.to12(p);
        check(ptam_camera_tracker_reset(h_, p), "ptam_camera_tracker_reset");
    }
    // free reports and free keyframe clones
    void Pool(int& nFreeReports, int& nFreeKeyFrames) const {
        int32_t a = 0, b = 0;
        check(ptam_camera_tracker_pool(h_, &a, &b), "ptam_camera_tracker_pool");
        nFreeReports = a, nFreeKeyFrames = b;
    }
    // the inner handles, for drawing: they stay the Tracker's
    ptam_tracker* tracker() const { return ptam_camera_tracker_tracker(h_); }
    ptam_kf* current_keyframe() const { return ptam_camera_tracker_current_keyframe(h_); }
    ptam_frame_report* last_report() const { return ptam_camera_tracker_last_report(h_); }
    ptam_camera_tracker* handle() const { return h_; }

private:
    ptam_camera_tracker* h_ = nullptr;
    bool session_ = false, poke_ = false;
    ptam_camera_session_result last_{};
};

// class Bundle (include/Bundle.h:106-152)
class Bundle {
public:
    explicit Bundle(Context& c, const ptam_ba_opts* opts = nullptr) { check(ptam_ba_create(c.handle(), opts, &h_), "ptam_ba_create"); }
    ~Bundle() { ptam_ba_destroy(h_); }
    Bundle(const Bundle&) = delete;
    Bundle& operator=(const Bundle&) = delete;
    int AddCamera(const SE3& se3CamFromWorld, bool bFixed) {   // :111
        double p[12];
        se3CamFromWorld.to12(p);
        int id = ptam_ba_add_camera(h_, p, bFixed);
        check(id, "ptam_ba_add_camera");
        return id;
    }
    int AddPoint(const Vec<3>& v3Pos) {   // :112
        int id = ptam_ba_add_point(h_, v3Pos.data());
        check(id, "ptam_ba_add_point");
        return id;
    }
    void AddMeas(int nCam, int nPoint, const Vec<2>& v2Pos, double dSigmaSquared) {   // :113
        check(ptam_ba_add_meas(h_, nCam, nPoint, v2Pos.data(), dSigmaSquared), "ptam_ba_add_meas");
    }
    // :114 ; returns mnAccepted (>= 0).  The reference's own -1 is dead code (Do_LM_Step returns true unconditionally,
    // src/Bundle.cc:550), so a negative value only leaves this shim for the one input the device path refuses: a duplicated
    // (camera, point) measurement (PTAM_E_ARG; the reference silently keeps the last one).  MapMaker treats a
    // negative return as "ditch the map" (src/MapMaker.cc:887-892) — harsh, but it keeps its thread alive, where an
    // exception thrown out of Compute() would not.  HIP / communicator failures still throw.
    int Compute(bool* pbAbortSignal) {
        int acc = 0;
        const int rc = ptam_ba_compute(h_, reinterpret_cast<const volatile unsigned char*>(pbAbortSignal), &acc);
        if (rc == PTAM_E_ARG) return -1;
        check(rc, "ptam_ba_compute");
        return acc;
    }
    bool Converged() const { return ptam_ba_converged(h_) != 0; }   // :115
    Vec<3> GetPoint(int n) const {                                   // :116
        Vec<3> v{};
        check(ptam_ba_get_point(h_, n, v.data()), "ptam_ba_get_point");
        return v;
    }
    SE3 GetCamera(int n) const {   // :117
        double p[12];
        check(ptam_ba_get_camera(h_, n, p), "ptam_ba_get_camera");
        return SE3::from12(p);
    }
    std::vector<std::pair<int, int>> GetOutlierMeasurements() const {   // :118 ; (point, camera)
        const int n = ptam_ba_get_outliers(h_, nullptr, 0);
        std::vector<int32_t> raw((size_t)2 * (n > 0 ? n : 0));
        if (n > 0) ptam_ba_get_outliers(h_, raw.data(), n);
        std::vector<std::pair<int, int>> out;
        for (int i = 0; i < n; i++) out.emplace_back(raw[2 * i], raw[2 * i + 1]);
        return out;
    }
    ptam_ba* handle() const { return h_; }

private:
    ptam_ba* h_ = nullptr;
};

}   // namespace ptam
#endif
