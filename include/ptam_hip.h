/*
 * ptam_hip.h — C ABI of libptam_hip.so: PTAM's tracking + bundle-adjustment hot path on
 * MI355X (gfx950), hand-written HIP kernels behind plain-C entry points.
 *
 * The reference (cggos/ptam_cg) has no FFI/plugin layer: its boundary for this path is the C++
 * class surface of KeyFrame / PatchFinder / Tracker / Bundle.  Each entry point below names the
 * reference interface it replaces (file:line, relative to the reference tree).  A header-only C++
 * shim that re-creates those class signatures over this ABI lives in ptam_shim.hpp.
 *
 * Conventions
 *   - every function returns an int status: PTAM_OK (0) or a negative PTAM_E_* code; algorithmic
 *     outcomes (found flags, accepted-iteration counts, the 32001 "out of border" ZMSSD sentinel,
 *     the -1 "bad template/level" sentinel) travel in out-parameters with the reference's values.
 *   - the caller keeps ownership of every host buffer; the library owns device memory behind
 *     opaque handles.  Bundle copies all inputs at add_* time like the reference
 *     (src/Bundle.cc:46-93).
 *   - a ptam_ctx is bound to ONE calling thread (own HIP stream + scratch).  The reference is
 *     entered from two threads (tracker: src/Tracker.cc:86, mapmaker: src/MapMaker.cc:57); give
 *     each its own ctx.  There is no global mutable state and no cached camera state
 *     (the reference's ATANCamera caches its last projection, include/ATANCamera.h:12-16).
 *   - poses are camera-from-world SE3 as 12 doubles: R row-major (9) then t (3).
 *   - images are 8-bit grey, row-major, `stride` bytes per row.
 *   - there is NO CPU fallback: if no gfx950 device / kernel image is available the create call
 *     fails with PTAM_E_HIP.
 */
#ifndef PTAM_HIP_H
#define PTAM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTAM_LEVELS 4                /* include/KeyFrame.h:34 */
#define PTAM_PATCH 8                 /* PatchFinder default nPatchSize, include/PatchFinder.h:55 */
#define PTAM_MAX_SSD (8 * 8 * 500)   /* src/PatchFinder.cc:18-19  -> 32000 */

enum {
    PTAM_OK = 0,
    PTAM_E_ARG = -1,      /* bad argument */
    PTAM_E_HIP = -2,      /* HIP runtime error (see ptam_last_error); a call that waits for a result: the device queue failed */
    PTAM_E_STATE = -3,    /* call out of order; a call that waits for a result (ptam_track_map*, ptam_track_frame, ptam_pose_gn*,
                             ptam_ba_compute): the device queue drained and the result never arrived — ptam_last_error names it */
    PTAM_E_LIMIT = -4,    /* size above a documented limit */
    PTAM_E_COMM = -5      /* collective failed */
};

/* libCVD halfSample rounding variant.  R = SSE2 pavgb/pavgw double rounding
 * (what an x86-64 libCVD build does for 16-byte aligned byte images), T = (a+b+c+d)/4 truncating. */
enum { PTAM_HALFSAMPLE_R = 0, PTAM_HALFSAMPLE_T = 1 };

/* cg::Tukey / Cauchy / Huber, include/Tools.h:128-228 */
enum { PTAM_EST_TUKEY = 0, PTAM_EST_CAUCHY = 1, PTAM_EST_HUBER = 2 };

typedef struct ptam_ctx ptam_ctx;
typedef struct ptam_kf ptam_kf;
typedef struct ptam_ba ptam_ba;

typedef struct { int32_t x, y; } ptam_int2;   /* CVD::ImageRef */

/* ATANCamera parameters: the 5-vector of config/camera.cfg:7 (normalised fx fy cx cy, w) and the
 * image size of ATANCamera::SetImageSize (src/ATANCamera.cc:21-25). */
typedef struct {
    double fx, fy, cx, cy, w;
    int32_t width, height;
} ptam_cam_params;

const char* ptam_last_error(void);           /* thread-local message of the last failure */
int ptam_device_count(int* n);

/* ---- context ------------------------------------------------------------------------------- */
/* replaces: ATANCamera(..) + RefreshParams (src/ATANCamera.cc:11-66); one per calling thread. */
int ptam_ctx_create(const ptam_cam_params* cam, int device, ptam_ctx** out);
int ptam_ctx_destroy(ptam_ctx* ctx);
int ptam_ctx_set_halfsample(ptam_ctx* ctx, int variant);
int ptam_ctx_sync(ptam_ctx* ctx);
void* ptam_ctx_stream(ptam_ctx* ctx);        /* the hipStream_t all of ctx's work is queued on */
/* derived camera constants (mdLargestRadius, mdMaxR, md2Tan, focal, centre: src/ATANCamera.cc:33-66) */
int ptam_ctx_camera_constants(ptam_ctx* ctx, double out[8]);

/* device memory helpers for callers that keep inputs resident (bench, shards) */
int ptam_dev_alloc(ptam_ctx* ctx, size_t bytes, void** dptr);
int ptam_dev_free(ptam_ctx* ctx, void* dptr);
int ptam_dev_upload(ptam_ctx* ctx, void* dptr, const void* host, size_t bytes);
int ptam_dev_download(ptam_ctx* ctx, void* host, const void* dptr, size_t bytes);

/* ---- KeyFrame::MakeKeyFrame_Lite  (src/KeyFrame.cc:18-54) ------------------------------------ */
int ptam_kf_create(ptam_ctx* ctx, int width, int height, ptam_kf** out);
int ptam_kf_destroy(ptam_kf* kf);
/* host image -> pyramid + FAST-10 (thresholds 10,15,15,10) + row LUTs, all on device. */
int ptam_make_keyframe_lite(ptam_ctx* ctx, ptam_kf* kf, const uint8_t* im, int stride);
/* same, image already resident on the device (stride == width) */
int ptam_make_keyframe_lite_dev(ptam_ctx* ctx, ptam_kf* kf, const uint8_t* d_im);
/* Level::operator= deep copy (include/KeyFrame.h:66-75) for the tracker->mapmaker hand-off
 * (src/MapMaker.cc:480-488), device to device. */
int ptam_kf_clone(ptam_ctx* ctx, const ptam_kf* src, ptam_kf** out);
/* The same copy into an EXISTING keyframe of the same image size: device to device on the context's queue, asynchronous, no
 * allocation (a keyframe pool for the hand-off: allocating under queued kernels costs milliseconds).  Afterwards dst reads
 * byte for byte as ptam_kf_clone(src) does: every level's image, corners and row LUT, and the MakeKeyFrame_Rest data if src
 * has it.  Whatever dst held is gone: its own rest data counts as not made (the next ptam_make_keyframe_rest /
 * ptam_mapmaker_step makes it, as for a fresh clone of a tracker's keyframe) and its in-plane corner cache is stale.
 * PTAM_E_ARG: another size, another device, src == dst. */
int ptam_kf_copy(ptam_ctx* ctx, const ptam_kf* src, ptam_kf* dst);
int ptam_kf_level_info(ptam_ctx* ctx, const ptam_kf* kf, int level, int* w, int* h, int* n_corners);
/* host read-back of aLevels[level].im / vCorners / vCornerRowLUT; NULL pointers are skipped.
 * px: w*h bytes; corners: n_corners entries (raster order); rowlut: h ints. */
int ptam_kf_read_level(ptam_ctx* ctx, const ptam_kf* kf, int level,
                       uint8_t* px, ptam_int2* corners, int32_t* rowlut);

/* ---- KeyFrame::MakeKeyFrame_Rest (src/KeyFrame.cc:61-79; its SmallBlurryImage, :80-81, is ptam_sbi_bank_add): libCVD fast_nonmax
 *      (score = largest threshold >= 10 at which the corner survives; kept iff no 8-neighbour corner
 *      scores strictly higher) and ImageProcess::ShiTomasiScoreAtPoint (src/ImageProcess.cc:20-47) on
 *      the maximal corners that lie >= 10 pixels inside the level.   */
int ptam_make_keyframe_rest(ptam_ctx* ctx, ptam_kf* kf);
int ptam_kf_rest_info(ptam_ctx* ctx, const ptam_kf* kf, int level, int* n_max_corners);
/* vMaxCorners (raster order) and, per maximal corner, its Shi-Tomasi score (-1.0 where the corner
 * is closer than 10 pixels to the border and the reference skips it).  Level::vCandidates is the
 * subset with score > MapMaker.CandidateMinShiTomasiScore (70; 400 in config/settings.cfg:27). */
int ptam_kf_read_rest(ptam_ctx* ctx, const ptam_kf* kf, int level, ptam_int2* max_corners, double* st_scores);

/* ---- PatchFinder::FindPatchCoarse / ZMSSDAtPoint  (src/PatchFinder.cc:160-211, 326-329;
 *      src/ImageProcess.cc:130-163) ------------------------------------------------------------- */
typedef struct {
    int32_t x, y;        /* irPos: predicted position, LEVEL-0 pixels (ir(v2Image), src/Tracker.cc:881) */
    int32_t level;       /* mnSearchLevel 0..3; < 0 = template bad, not searched */
    uint32_t range;      /* nRange in level-0 pixels */
} ptam_patch_query;

typedef struct {
    int32_t found;       /* mbFound */
    int32_t best_ssd;    /* nBestSSD; PTAM_MAX_SSD+1 when nothing scored */
    int32_t best_x, best_y;   /* irBest in search-level pixels (undefined when nothing scored: -1) */
    int32_t n_scored;    /* candidates that reached ZMSSDAtPoint */
    int32_t pad_;
    double pos[2];       /* mv2CoarsePos = LevelZeroPos(irBest, level), valid iff found */
} ptam_patch_result;

/* n queries, templates = n * 64 bytes (8x8 row-major, mimTemplate).  Host buffers. */
int ptam_find_patch_coarse_batch(ptam_ctx* ctx, const ptam_kf* kf, int n,
                                 const ptam_patch_query* queries, const uint8_t* templates,
                                 ptam_patch_result* results);
/* device-resident variant (queries/templates/results are device pointers), asynchronous */
int ptam_find_patch_coarse_batch_dev(ptam_ctx* ctx, const ptam_kf* kf, int n,
                                     const ptam_patch_query* d_queries, const uint8_t* d_templates,
                                     ptam_patch_result* d_results);
/* ZMSSDAtPoint of ONE template at n explicit points of a level (parity / epipolar use). */
int ptam_zmssd_at_points(ptam_ctx* ctx, const ptam_kf* kf, int level, int n,
                         const ptam_int2* points, const uint8_t* tmpl64, int32_t* ssd_out);

/* ---- PatchFinder::MakeSubPixTemplate + IterateSubPixToConvergence (src/PatchFinder.cc:219-318):
 *      inverse-compositional sub-pixel refinement of a coarse match (second half) */
typedef struct {
    double coarse_pos[2];   /* mv2CoarsePos, level-0 pixels (result of FindPatchCoarse) */
    int32_t level;          /* mnSearchLevel; < 0 = skip */
    int32_t max_its;        /* nMaxIts (8 in the tracker, src/Tracker.cc:583) */
} ptam_subpix_query;
typedef struct {
    int32_t converged;      /* return value of IterateSubPixToConvergence */
    int32_t iterations;     /* IterateSubPix calls made */
    double pos[2];          /* mv2SubPixPos */
    double mean_diff;       /* mdMeanDiff */
} ptam_subpix_result;
int ptam_subpix_batch(ptam_ctx* ctx, const ptam_kf* kf, int n, const ptam_subpix_query* queries,
                      const uint8_t* templates, ptam_subpix_result* results);

/* ---- PatchFinder::MakeTemplateCoarseCont (src/PatchFinder.cc:98-127): the 8x8 search template warped out
 *      of the map point's source keyframe by CVD::transform, then MakeTemplateSums.
 *      CVD::transform / CVD::sample are libCVD (not vendored by the reference): restated from its published
 *      source — positions advance by repeated addition (p += across per pixel, += down - 8*across per row),
 *      bilinear value (1-y)*((1-x)*a + x*b) + y*((1-x)*c + x*d) in double, converted to a byte by
 *      truncation; pixels whose source position leaves [0,w-1)x[0,h-1) become 0 and count as outside
 *      (checked per pixel only when the patch's bounding box is not wholly inside).
 *      The "same map point, warp moved < 0.07" reuse test (:103-111) is host state and stays with the
 *      caller (ptam::PatchFinder / host.PatchFinder keep mpLastTemplateMapPoint and mm2LastWarpMatrix). */
typedef struct {
    const ptam_kf* src_kf;      /* MapPoint::pPatchSourceKF */
    int32_t src_level;          /* MapPoint::nSourceLevel */
    int32_t search_level;       /* mnSearchLevel from CalcSearchLevelAndWarpMatrix; < 0 = template bad, skipped */
    int32_t center_x, center_y; /* MapPoint::irCenter, source-level pixels */
    double warp_inverse[4];     /* mm2WarpInverse row-major (ptam_pvs_result::warp_inverse) */
} ptam_template_query;
typedef struct {
    int32_t bad;                /* mbTemplateBad = (bool)nOutside (1 also when the query was skipped) */
    int32_t n_outside;          /* return value of CVD::transform */
    int32_t sum, sum_sq;        /* mnTemplateSum, mnTemplateSumSq */
    double m2[4];               /* the warp matrix used: M2Inverse(mm2WarpInverse) * LevelScale(mnSearchLevel) */
} ptam_template_result;
/* templates_out: n * 64 bytes (8x8 row-major), the layout ptam_find_patch_coarse_batch takes */
int ptam_make_templates_batch(ptam_ctx* ctx, int n, const ptam_template_query* queries, uint8_t* templates_out,
                              ptam_template_result* results);

/* ---- MapMaker::AddPointEpipolar: the corner scan (src/MapMaker.cc:598-637)   --------------
 * (ptam_add_map_points_epipolar below runs the whole of AddSomeMapPoints on the device; this batch call is its scan alone.)
 * Here the line geometry (:541-596) stays with the caller — it is per-candidate scalar code on poses and depth
 * statistics; what moves to the device is the O(candidates x corners) part: MakeTemplateCoarseNoWarp of the
 * candidate in the source keyframe (:599, src/PatchFinder.cc:137-148), the in-plane corner table of the target
 * level (:604-614), the band / segment test of every target corner (:620-630) and ZMSSDAtPoint of the survivors
 * (:631-635), first strict minimum in corner order. */
/* Level::vImplaneCorners: UnProject(ir(LevelZeroPos(corner, level))) of every FAST corner of the level, built once
 * per (keyframe, level) and cached on the device (bImplaneCornersCached).  out_xy (nullable): room for cap corners,
 * 2 doubles each; n_out (nullable): the corner count. */
int ptam_kf_implane_corners(ptam_ctx* ctx, ptam_kf* kf, int level, double* out_xy, int cap, int* n_out);
typedef struct {
    int32_t level_x, level_y;   /* candidate.irLevelPos in the SOURCE keyframe, level pixels */
    double normal[2];           /* v2Normal */
    double norm_dist;           /* dNormDist */
    double along[2];            /* v2AlongProjectedLine */
    double min_len, max_len;    /* dMinLen, dMaxLen (after the +-2.0 clamps) */
    double max_dist_sq;         /* dMaxDistSq = (OnePixelDist() * (4 + nLevelScale))^2 */
} ptam_epipolar_query;
typedef struct {
    int32_t best;               /* nBest: index into the target level's vCorners, -1 = none */
    int32_t best_zmssd;         /* nBestZMSSD (PTAM_MAX_SSD + 1 when none) */
    int32_t n_scored;           /* corners that reached ZMSSDAtPoint */
    int32_t template_bad;       /* Finder.TemplateBad() after MakeTemplateCoarseNoWarp */
} ptam_epipolar_result;
int ptam_epipolar_search_batch(ptam_ctx* ctx, const ptam_kf* src, ptam_kf* target, int level, int n,
                               const ptam_epipolar_query* queries, ptam_epipolar_result* results);
/* ATANCamera::OnePixelDist() (src/ATANCamera.cc:69-75) for max_dist_sq */
int ptam_ctx_one_pixel_dist(ptam_ctx* ctx, double* out);
/* A deliberate deviation made observable.  TrackerData::ProjectAndDerivs (include/Tracker.h:89-94) calls GetProjectionDerivs()
 * after Project() even when Project() bailed out before the camera model (:73-80: a point behind the camera or outside the model's
 * radius) — the derivatives it then reads are the camera's cache of whichever point was projected last.  Here such a point keeps
 * its own derivatives of the previous iteration.  *out = how often that happened in the pose loops
 * (ptam_pose_gn*, ptam_track_map*, ptam_track_frame) on this context's device since the library was loaded: 0 means every
 * tracked frame so far was also bit-for-bit what the reference's data flow gives. */
int ptam_ctx_cache_hazards(ptam_ctx* ctx, long long* out);

/* ---- TrackerData::Project / ProjectAndDerivs + ATANCamera (include/Tracker.h:70-94,
 *      src/ATANCamera.cc:109-121, 179-209) ------------------------------------------------------- */
typedef struct {
    double cam[3];       /* v3Cam */
    double image[2];     /* v2Image */
    double derivs[4];    /* m2CamDerivs row-major */
    int32_t in_image;    /* bInImage */
    int32_t pad_;
} ptam_projection;
int ptam_project_points(ptam_ctx* ctx, int n, const double* world_xyz, const double pose[12],
                        ptam_projection* out);

/* TrackerData::Project (include/Tracker.h:70-85) on EXISTING TrackerData, as TrackMap re-projects the points it is about to
 * search after the coarse pose update (src/Tracker.cc:573-574, :606-608): cam always, image once the camera model is reached
 * (a point that bails out earlier keeps its previous v2Image), derivs untouched (ProjectAndDerivs refreshes them only for
 * found points, include/Tracker.h:89-94), in_image = bInImage. */
int ptam_reproject_points(ptam_ctx* ctx, int n, const double* world_xyz, const double pose[12], ptam_projection* inout);

/* ---- Tracker::TrackMap potentially-visible-set loop (src/Tracker.cc:453-478) with
 *      PatchFinder::CalcSearchLevelAndWarpMatrix (src/PatchFinder.cc:52-84)   */
typedef struct {
    double world[3];          /* MapPoint::v3WorldPos */
    double pixel_right_w[3];  /* MapPoint::v3PixelRight_W */
    double pixel_down_w[3];   /* MapPoint::v3PixelDown_W */
} ptam_pvs_point;
typedef struct {
    ptam_projection proj;     /* TData.v3Cam / v2Image / m2CamDerivs / bInImage */
    double warp_inverse[4];   /* mm2WarpInverse row-major (valid iff proj.in_image) */
    int32_t level;            /* nSearchLevel 0..3, or -1 (not in image, or inappropriate warp) */
    int32_t pad_;
} ptam_pvs_result;
/* counts (nullable): number of points per search level = sizes of avPVS[0..3] */
int ptam_track_pvs(ptam_ctx* ctx, int n, const ptam_pvs_point* points, const double pose[12],
                   ptam_pvs_result* results, int32_t counts[4]);

/* ---- MapMaker::ReFind_Common (src/MapMaker.cc:943-1020) for a batch of map points against ONE keyframe — the loop of
 *      ReFindInSingleKeyFrame (:1027-1042), and per keyframe of ReFindNewlyMade / ReFindFromFailureQueue  (SURVEY §8f rank 4).
 *      Per point: projection into the keyframe with the visibility tests of :950-975, camera derivatives,
 *      CalcSearchLevelAndWarpMatrix (its verdict is not looked at by the reference: the template is made at the level the
 *      loop stopped at and only CVD::transform's outside count decides TemplateBad, :979-986), FindPatchCoarse with range 4
 *      (:988), and for level > 0 the sub-pixel refinement whose convergence flag the reference ignores (:1000-1006).
 *      The set bookkeeping (sMeasurementKFs / sNeverRetryKFs tests of :947-948, inserts) stays with the caller. */
typedef struct {
    int32_t found;          /* return value: a measurement {level, root_pos, sub_pix, SRC_REFIND} is to be added */
    int32_t level;          /* m.nLevel = Finder.GetLevel(); -1 when the point never reached the PatchFinder */
    int32_t sub_pix;        /* m.bSubPix */
    int32_t never_retry;    /* the point-keyframe pair goes into sNeverRetryKFs (every failure path of the reference) */
    double root_pos[2];     /* m.v2RootPos, level-0 pixels (valid iff found) */
} ptam_refind_result;
int ptam_refind_batch(ptam_ctx* ctx, const ptam_kf* kf, const double kf_pose[12], int n, const ptam_pvs_point* points,
                      const ptam_template_query* sources /* src_kf, src_level, center_x / center_y */, ptam_refind_result* out);

/* ---- MapMaker::ReFind_Common as the reference CALLS it (src/MapMaker.cc:1046-1082): a list of (keyframe, point) pairs taken
 *      in order through ONE PatchFinder — `static PatchFinder Finder` (:977) — whose MakeTemplateCoarseCont keeps the
 *      template, its sums and mbTemplateBad when it last warped THIS map point and neither column of the warp has moved by
 *      more than 0.07 since (src/PatchFinder.cc:98-127).  ReFindNewlyMade (:1046-1066) is one new point against every
 *      keyframe in turn: consecutive keyframes with nearly the same pose search with the template of the first.  And a warp
 *      CalcSearchLevelAndWarpMatrix rejects sets mbTemplateBad (:78-81), which a kept template does not clear — that pair
 *      (and the kept ones after it) goes into sNeverRetryKFs although an earlier pair searched with the same template.
 *      The finder object carries that state from call to call like the static does; pairs with `skip` set (:947-948: the
 *      point is already measured in the keyframe, or never to be retried) return false without touching it. */
typedef struct ptam_refinder ptam_refinder;
int ptam_refinder_create(ptam_ctx* ctx, ptam_refinder** out);
int ptam_refinder_destroy(ptam_refinder* f);
typedef struct {
    const ptam_kf* kf;            /* k */
    double kf_pose[12];           /* k.se3CfromW */
    ptam_pvs_point point;         /* p: world position and pixel vectors */
    ptam_template_query source;   /* p: patch source (src_kf, src_level, center_x / center_y; the other fields are ignored) */
    int64_t point_id;             /* identity of the MapPoint (the reference compares &p with mpLastTemplateMapPoint) */
    int32_t skip;                 /* :947-948 */
    int32_t pad_;
} ptam_refind_pair;
/* template_kept (nullable): 1 where the finder searched with the template it already had */
int ptam_refind_pairs(ptam_ctx* ctx, ptam_refinder* finder, int n, const ptam_refind_pair* pairs, ptam_refind_result* out,
                      int32_t* template_kept);

/* ---- MapMaker::AddSomeMapPoints (src/MapMaker.cc:448-457) for a list of levels: per visited level ThinCandidates (:415-441)
 *      and AddPointEpipolar (:529-688) for every remaining candidate, all on the device (the rest of SURVEY §8f rank 4).
 *      kSrc is the newest keyframe (:450), kTarget the caller's ClosestKeyFrame (:451).  Per visited level L:
 *        - candidates: the maximal corners of ptam_make_keyframe_rest with Shi-Tomasi score > min_shi_tomasi, raster order
 *          (src/KeyFrame.cc:66-76);
 *        - thinning: a candidate is kept iff (irB - irC).mag_squared() >= 100 for every busy position irB at level L or L + 1,
 *          irB = ir_rounded(v2RootPos / LevelScale(L)) (rounding half away from zero).  The busy positions are kSrc's
 *          measurements (nLevel, v2RootPos) passed by the caller, plus the SRC_ROOT measurement of every point this call has
 *          made at an earlier visited level (:679-683) — level 2 is thinned by the points just made at level 3;
 *        - per kept candidate, in the reference's order: the ray and line geometry with its early returns (:541-596, fp64,
 *          the reference's operation order without FMA contraction), the 0.001 push of a ray start behind kTarget (:573-574),
 *          the LargestRadiusInImage test (:588-589), MakeTemplateCoarseNoWarp and the corner scan (:598-637, as
 *          ptam_epipolar_search_batch), MakeSubPixTemplate + IterateSubPixToConvergence(kTarget, subpix_max_its) from
 *          LevelZeroPos(vIR[nBest]) (:640-645, as ptam_subpix_batch), Triangulate (:171-189: smallest right singular vector of
 *          the 4x4 system, v4[3] == 0 -> 1e-5) mapped to the world by kTarget^-1 (:649), the _NC vectors (:661-667) and
 *          MapPoint::RefreshPixelVectors (src/Map.cc:40-65).
 *      Points come out in visiting order of levels, then candidate order: the order of vpPoints / mqNewQueue, which
 *      ReFindNewlyMade (:1046-1066) walks.  The thinned candidate list is NOT written back into kSrc: the reference never
 *      reuses it (kSrc is always the newest keyframe, and its next keyframe becomes kSrc in turn).
 *      Synchronous like the other batch calls: one host sync, at the end. */
typedef struct {
    double depth_mean, depth_sigma;  /* kSrc.dSceneDepthMean / Sigma: ptam_motion_model.scene_depth_mean / _sigma (Tracker.cc:692-696) */
    double wiggle_scale;             /* MapMaker::mdWiggleScale (MapMaker.WiggleScale, 0.1) */
    double min_shi_tomasi;           /* MapMaker.CandidateMinShiTomasiScore: 70 (src/KeyFrame.cc:63), 400 in config/settings.cfg:27 */
    int32_t subpix_max_its;          /* IterateSubPixToConvergence(kTarget, 10) (:642) */
    int32_t n_levels;                /* 1..4 */
    int32_t levels[4];               /* visiting order: {3,0,1,2} AddKeyFrameFromTopOfQueue (:511-514), {0,3,1,2} InitFromStereo (:382-385) */
} ptam_epipolar_opts;
void ptam_epipolar_opts_default(ptam_epipolar_opts* o);   /* depth 1 +- 1, 0.1, 70, 10, {3,0,1,2} */

typedef struct {
    ptam_pvs_point point;            /* v3WorldPos, v3PixelRight_W, v3PixelDown_W: feeds ptam_tracker_update_map / refind as is */
    double center_nc[3], one_right_nc[3], one_down_nc[3];   /* v3Center_NC, v3OneRightFromCenter_NC, v3OneDownFromCenter_NC
                                                               (normalised); v3Normal_NC is (0,0,-1) */
    double src_root_pos[2];          /* kSrc measurement (SRC_ROOT, bSubPix): v2RootPos = LevelZeroPos(irCenter, level) */
    double target_pos[2];            /* kTarget measurement (SRC_EPIPOLAR) = Finder.GetSubPixPos() */
    int32_t level;                   /* nSourceLevel = nLevel of both measurements */
    int32_t center_x, center_y;      /* irCenter = candidate.irLevelPos */
    int32_t candidate;               /* index into the level's candidates BEFORE thinning */
    int32_t target_corner;           /* nBest in kTarget.aLevels[level].vCorners */
    int32_t best_zmssd;              /* nBestZMSSD */
} ptam_new_map_point;

typedef struct {                     /* per visited level, one count per return path of AddPointEpipolar */
    int32_t candidates;              /* vCandidates before ThinCandidates */
    int32_t kept_after_thinning;
    int32_t ray_rejected;            /* :569-572 facing backwards / ray end behind kTarget */
    int32_t line_rejected;           /* :581-584 projected line too short, :588-589 line outside LargestRadiusInImage */
    int32_t template_bad;            /* :600-601 */
    int32_t no_match;                /* :636-637 nBest == -1 */
    int32_t subpix_failed;           /* :643-644 */
    int32_t made;
} ptam_epipolar_level_stats;

/* src_pose / target_pose: kSrc.se3CfromW, kTarget.se3CfromW.  busy (n_busy >= 0): kSrc.mMeasurements' nLevel (0..3) and
 * v2RootPos (2 doubles each).  out: room for cap points; cap must be at least the sum of ptam_kf_rest_info over the visited
 * levels, else PTAM_E_ARG and nothing is written.  stats (nullable): opts->n_levels entries, in visiting order.
 * PTAM_E_STATE: src has had no ptam_make_keyframe_rest since its last ptam_make_keyframe_lite.  PTAM_E_ARG also for keyframes
 * of another device, repeated or out-of-range levels, n_levels outside 1..4 and busy levels outside 0..3. */
int ptam_add_map_points_epipolar(ptam_ctx* ctx, const ptam_kf* src, const double src_pose[12],
                                 ptam_kf* target, const double target_pose[12], const ptam_epipolar_opts* opts,
                                 int n_busy, const int32_t* busy_level, const double* busy_root_xy,
                                 ptam_new_map_point* out, int cap, int32_t* n_out,
                                 ptam_epipolar_level_stats* stats);

/* ---- Tracker::TrackForInitialMap: TrailTracking_Start / TrailTracking_Advance (src/Tracker.cc:352-432) with
 *      MiniPatch::SampleFromImage / FindPatch / SSDAtPoint (src/ImageProcess.cc:57-80, 196-252), on device-resident keyframes.
 *      A trail is a 9x9 byte patch (MiniPatch::mirPatchSize) sampled in the first frame, its position there and its position
 *      in the newest frame.  Every value is an integer: the device list is the reference's list, to the bit.
 *      The object belongs to the context it was created with (its queue, its staging) and to that context's image size
 *      (ptam_cam_params.width / height); all its memory is allocated by ptam_trails_create.  Every call is synchronous: one
 *      host wait, at the end. */
typedef struct ptam_trails ptam_trails;
typedef struct { int32_t initial_x, initial_y, current_x, current_y; } ptam_trail;   /* Trail::irInitialPos, irCurrentPos (include/Tracker.h) */
/* HomographyMatch (include/HomographyInit.h): v2CamPlaneFirst, v2CamPlaneSecond, m2PixelProjectionJac row-major */
typedef struct { double first[2], second[2], jac[4]; } ptam_homography_match;

/* max_trails >= 1: room for that many trails (Tracker.MaxInitialTrails is 1000) */
int ptam_trails_create(ptam_ctx* ctx, int max_trails, ptam_trails** out);
int ptam_trails_destroy(ptam_trails* t);
/* TrailTracking_Start (src/Tracker.cc:352-370) after the caller's ptam_make_keyframe_rest(first) (:354; PTAM_E_STATE without
 * it): the level-0 candidates — maximal corners >= 10 pixels inside the image with Shi-Tomasi score > min_shi_tomasi
 * (src/KeyFrame.cc:66-76) — in std::sort's order of pair<-score, ImageRef> (:356-359: descending score, ties by ascending
 * y, then x: libCVD's ImageRef::operator<); the first min(max_initial, max_trails) become trails (:360-368), each with its
 * patch around its position and irCurrentPos = irInitialPos.  The object keeps ITS OWN copy of first's level-0 image,
 * corners and row LUT as the previous frame (mPreviousFrameKF = mFirstKF, :369): the caller may reuse `first` for the next
 * frame.  A start on a started object begins again.  *n_trails: the trails made. */
int ptam_trails_start(ptam_trails* t, const ptam_kf* first, double min_shi_tomasi, int max_initial, int* n_trails);
/* TrailTracking_Advance (src/Tracker.cc:376-432).  Per trail, in list order: FindPatch(irEnd = irCurrentPos, current level-0
 * image, nRange 10, current vCorners) — the corners of the closed box +-10 in raster order (started from the row LUT entry
 * of the clamped top row: the same corners as the reference's linear start, :216-220), SSDAtPoint of each (nMaxSSD + 1 =
 * 100001 for a corner nearer than 4 pixels to a border), the first strictly smaller SSD wins, found iff the best is below
 * 100000.  Not found: the trail is erased.  Found: it counts in *n_good and irCurrentPos = irEnd; then a 9x9 patch sampled at
 * irEnd in the current frame is searched the same way in the previous frame from irEnd, and the trail stays iff that search
 * found something and (irBackWardsFound - irStart).mag_squared() <= 2 (:402-407).  A trail that fails this married-matches
 * check is erased although it was counted (:409-410): *n_good is the reference's return value — the caller's
 * `nGoodTrails < 10 -> Reset()` (:329) — and *n_alive the length of the list afterwards.  Survivors keep their order.  The
 * current frame's level-0 data is then copied into the object as the previous frame (:430).  Two kernel launches. */
int ptam_trails_advance(ptam_trails* t, const ptam_kf* current, int* n_good, int* n_alive);
/* TrailTracking_Advance (src/Tracker.cc:376-432) behind MakeKeyFrame_Lite (src/KeyFrame.cc:17-59, as TrackFrame calls it, :87) for
 * nb cameras — trails[i] with its keyframe current[i] — as ONE chain of launches on the queue of trails[0]'s context: the pyramid
 * and the corners of d_frames[i] (a device-resident frame) into current[i], one launch of the search for all cameras' trails, one
 * launch of the compaction and the kept frames.  d_frames == NULL or d_frames[i] == NULL: current[i] has been made already.  The
 * counts come back through a host-mapped block of each object (allocated by ptam_trails_create), written behind the camera's last
 * workgroup: one wait per camera on those words, no copy.  Camera i's list, patches, kept frame, n_good[i], n_alive[i] and
 * current[i] are, to the bit, what ptam_make_keyframe_lite_dev + ptam_trails_advance leave, for every nb; an object without live
 * trails is legal (0 / 0, its frame is kept).
 * Conditions, those of ptam_track_map_frames_batch: nb in 1..4096; one device, one image size and one halfSample variant; every
 * object in a DIFFERENT context; no object and no keyframe twice; each keyframe of its object's device and image size (a keyframe
 * carries no context of its own).  The call first waits for the queues of the other objects' contexts.  PTAM_E_ARG for a broken
 * condition or a null entry, PTAM_E_STATE for an object before its ptam_trails_start — both decided before anything is enqueued,
 * with every object and keyframe as it was.  PTAM_E_HIP (the queue failed): no object is committed — each still names its list of
 * before the call, though keyframes and kept frames may have been written; the next batch clears what the dead chain left in the
 * objects' headers.  Start the trails again after such a failure. */
int ptam_trails_advance_batch(int nb, ptam_trails* const* trails, ptam_kf* const* current, const uint8_t* const* d_frames,
                              int32_t* n_good, int32_t* n_alive);
/* mlTrails in list order.  cap < the live count: PTAM_E_ARG and nothing is written. */
int ptam_trails_read(ptam_trails* t, ptam_trail* out, int cap, int* n);
/* Trail::mPatch.mimOrigPatch of the live trails in list order: 81 bytes each (9 rows of 9); cap in trails */
int ptam_trails_read_patches(ptam_trails* t, uint8_t* out, int cap, int* n);
/* The first loop of MapMaker::InitFromStereo (src/MapMaker.cc:272-279) for the live trails: first = UnProject(irInitialPos),
 * second = UnProject(irCurrentPos) (src/ATANCamera.cc:125-140), jac = GetProjectionDerivs() (:179-209) as the camera's cache
 * stands after the SECOND UnProject — mvLastCam = second, mdLastR = the undistorted radius, mdLastFactor = 1 / dFactor: the
 * derivative at the second point.  fp64 in the reference's operation order, no FMA contraction.  This is the input of
 * HomographyInit::Compute (src/HomographyInit.cc): ptam_trails_homography below runs it on this table without the download;
 * a caller that keeps the reference's own Compute reads the table here. */
int ptam_trails_matches(ptam_trails* t, ptam_homography_match* out, int cap, int* n);
/* PTAM_E_ARG: a null pointer, max_trails < 1, a keyframe of another device or of another image size than the object's,
 * cap smaller than the live count.  PTAM_E_STATE: advance / read / read_patches / matches before start. */

/* ---- HomographyInit::Compute (src/HomographyInit.cc:35-63), stage (1) of MapMaker::InitFromStereo (src/MapMaker.cc:281-293),
 *      fp64 throughout, two kernel launches, one host wait at the end:
 *      BestHomographyFromMatches_MLESAC (:179-230): fewer than ten matches -> one DLT over all of them (HomographyFromMatches
 *      :65-115, with the zeroed ninth row when 2n < 9); otherwise `trials` hypotheses, each the DLT of four matches scored by the
 *      sum of MLESACScore (:23-33) over all matches; the strictly smaller score wins, among equal scores the lowest trial.  The
 *      DLT's null vector is the right singular vector of the smallest singular value by one-sided Jacobi (the reference:
 *      TooN SVD over LAPACK; a singular vector's sign is free and nothing below depends on it).
 *      Inliers: IsHomographyInlier (:14-21, squared pixel error strictly below max_pixel_error^2), then five
 *      RefineHomographyWithInliers (:120-177): WLS<9> with the prior 1.0, Tukey::FindSigmaSquared (the median is sorted[n / 2],
 *      2n - 6 in size_t arithmetic) and Tukey::Weight (include/Tools.h), the 9x9 system solved by Cholesky (L D L^T).
 *      One place where the reference divides zero by zero is given a defined meaning: a match whose error is exactly zero
 *      has weight 1 (with a zero median, which four exactly fitted matches can produce, Tukey::Weight is 1 - 0 / 0 and the
 *      reference's pose is NaN).
 *      DecomposeHomography (:232-339): the eight solutions in the reference's push order; bit-equal singular values
 *      (nCase != 1) end the call with PTAM_HOMOG_DEGENERATE.  ChooseBestDecomposition (:363-435): the two visibility counts,
 *      each followed by a stable sort (std::sort on eight elements is an insertion sort), the ratio test
 *      (double)s1 / (double)s0 < 0.9, else the Sampson sums over ALL matches, capped at 4 max_pixel_error^2, `<=` choosing the
 *      first.  An empty inlier set (the reference asserts in FindSigmaSquared) ends the call with PTAM_HOMOG_NO_INLIERS.
 *      The draw: the reference calls rand() (:198-211); here the quadruples are an input.  opts->samples: trials x 4 match
 *      indices; NULL: the table ptam_homography_samples(opts->seed, n, trials) — splitmix64 (state += 0x9E3779B97F4A7C15;
 *      z = state; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; next = z ^ z >> 31) started from
 *      state = seed, every index next() % n_matches, an index already in its quadruple drawn again (the while(!isUnique) loop).
 *      Sums over matches are reduced in a fixed order: two calls on the same input give the same bits. */
enum { PTAM_HOMOG_OK = 0, PTAM_HOMOG_DEGENERATE = 1, PTAM_HOMOG_NO_INLIERS = 2 };
typedef struct {
    double   max_pixel_error;   /* 5.0: src/MapMaker.cc, the Compute(vMatches, 5.0, se3) call */
    int32_t  trials;            /* 300: src/HomographyInit.cc:195 */
    uint64_t seed;              /* used when samples == NULL */
    const int32_t* samples;     /* trials x 4 match indices, or NULL */
} ptam_homography_opts;
typedef struct {
    int32_t status, n_matches, n_inliers, best_trial /* -1 on the < 10 path */, ambiguous /* dRatio >= 0.9 */;
    double  best_score;         /* dBestError; 0 on the < 10 path */
    double  homography[9];      /* mm3BestHomography after the five refinements, row-major (NO_INLIERS: before them) */
    double  sampson[2];         /* adSampsonusScores when ambiguous, else 0; in the order of the two surviving decompositions,
                                   which between equal counts is their push order and follows the SVD's signs */
} ptam_homography_info;
void ptam_homography_opts_default(ptam_homography_opts*);
/* out: trials x 4.  PTAM_E_ARG: out == NULL, n_matches < 4, trials < 1.  Host only. */
int  ptam_homography_samples(uint64_t seed, int n_matches, int trials, int32_t* out);
/* se3_second_from_first = mvDecompositions[0].se3SecondFromFirst (R row-major, then t), written only when info->status ==
 * PTAM_HOMOG_OK (the reference's `return true`); info always; inlier_out (nullable): n bytes, 1 = mvHomographyInliers holds
 * the match.  The workspace is the context's scratch, which grows on demand and stays. */
int  ptam_homography_init(ptam_ctx*, int n, const ptam_homography_match* matches /* host */,
                          const ptam_homography_opts*, double se3_second_from_first[12],
                          ptam_homography_info* info, uint8_t* inlier_out);
/* The same on the live trails: ptam_trails_matches' kernel (the same bits) into the object's memory, then the kernels of
 * ptam_homography_init on that table; nothing comes down but the result.  ptam_trails_create reserves the workspace of a
 * call with max_trails matches and 300 trials.  inlier_out: one byte per live trail, in list order. */
int  ptam_trails_homography(ptam_trails*, const ptam_homography_opts*, double se3_second_from_first[12],
                            ptam_homography_info* info, uint8_t* inlier_out);
/* PTAM_E_ARG, with nothing written: a null pointer (inlier_out excepted), n < 4 (fewer than four live trails), trials < 1,
 * max_pixel_error <= 0, a sample index outside [0, n) or repeated inside its quadruple.  PTAM_E_STATE:
 * ptam_trails_homography before ptam_trails_start. */

/* ---- MapMaker::InitFromStereo, the point loop (src/MapMaker.cc:310-367): per match, in order, a level-0 map point in the
 *      first keyframe (whose pose is the identity, :305) centred on `initial`: the _NC vectors (:321-326),
 *      MakeTemplateCoarseNoWarp(first, 0, initial) (src/PatchFinder.cc:137-148), MakeSubPixTemplate, SetSubPixPos(vec(current)),
 *      IterateSubPixToConvergence(second, subpix_max_its) (:330-333, the code of ptam_subpix_batch),
 *      Triangulate(se3, UnProject(sub-pixel position), UnProject(initial)) (:342 -> :171-189: the 4x4 system, the same routine
 *      as ptam_add_map_points_epipolar; the reference's 6x4 TriangulateNew, :216-258, is not called by InitFromStereo), and
 *      MapPoint::RefreshPixelVectors (src/Map.cc:40-65).  The point is dropped when the alignment fails (:334-337) or its
 *      world z is negative (:343-346).
 *      Two places where the reference reads memory it has not written are given a defined meaning here.  (1) A centre nearer
 *      than 5 pixels to a border makes MakeTemplateCoarseNoWarp return with mbTemplateBad set, which InitFromStereo does not
 *      look at: it aligns the previous point's template.  Here the match is dropped as template_bad (a trail's initial
 *      position is >= 10 pixels inside, so the reference's own flow never gets there).  (2) :327 calls RefreshPixelVectors before
 *      v3WorldPos is assigned (:342); the vectors are computed again after the first accepted bundle step.  Here they are
 *      computed from the triangulated position.
 *      se3_second_from_first: HomographyInit's pose with its translation already scaled to WiggleScale (:296-297).
 *      out: room for n records; the made points come out in match order with level = 0, center = initial,
 *      src_root_pos = vec(initial) (the SRC_ROOT measurement, :352-357), target_pos = the sub-pixel position (the SRC_TRAIL
 *      measurement, :360-365), candidate = the match index, target_corner = -1, best_zmssd = 0.  status: n entries. */
enum { PTAM_INIT_MADE = 0, PTAM_INIT_SUBPIX_FAILED = 1, PTAM_INIT_BEHIND_CAMERA = 2, PTAM_INIT_TEMPLATE_BAD = 3 };
int ptam_init_points_from_trails(ptam_ctx* ctx, const ptam_kf* first, ptam_kf* second, const double se3_second_from_first[12],
                                 int n, const ptam_trail* matches, int subpix_max_its /* 10 (:333) */,
                                 ptam_new_map_point* out, int32_t* status, int32_t* n_out);

/* ---- Tracker pose Gauss-Newton (src/Tracker.cc:613-643 driver, :928-1005 CalcPoseUpdate,
 *      include/Tracker.h:125-142 CalcJacobian/LinearUpdate) ---------------------------------------- */
typedef struct {
    double world[3];         /* MapPoint::v3WorldPos */
    double found[2];         /* v2Found (level-0 pixels) */
    double sqrt_inv_noise;   /* dSqrtInvNoise = 1 / 2^level (src/Tracker.cc:889) */
} ptam_pose_meas;

typedef struct {
    int32_t iterations;          /* 10 */
    uint32_t nonlinear_mask;     /* bit i set = full re-projection + Jacobian on iteration i;
                                    fine stage 0x211 (iter 0,4,9), coarse stage 0x3ff */
    int32_t override_after;      /* override sigma^2 used for iter > override_after (5) */
    double override_sigma_sq;    /* 16.0 fine, 1.0 coarse */
    int32_t mark_outliers_iter;  /* iteration whose weight==0 set is reported (9; -1 = none) */
    int32_t estimator;           /* PTAM_EST_* ("Tracker.MEstimator") */
    double prior;                /* wls.add_prior(100.0) */
} ptam_gn_opts;
void ptam_gn_opts_default(ptam_gn_opts* o);   /* fine-stage schedule of src/Tracker.cc:613-643 */

/* Runs the whole 10-iteration loop on the device in one launch.
 * pose_inout: mse3CamFromWorld.  entry (nullable): per-measurement state at loop entry as left by
 * the caller's last Project (used on iteration 0, which does not re-project, src/Tracker.cc:617);
 * NULL = project every point with the entry pose.  outlier_flags (nullable, n ints): 1 where
 * Weight()==0 on mark_outliers_iter.  updates_out (nullable): iterations*6 doubles, the v6Update
 * of every iteration. */
int ptam_pose_gn(ptam_ctx* ctx, int n, const ptam_pose_meas* meas, const ptam_projection* entry,
                 double pose_inout[12], const ptam_gn_opts* opts,
                 int32_t* outlier_flags, double* updates_out);

/* The same, also returning the measurements' TrackerData state when the loop ends (cam = v3Cam, image = v2Image, derivs =
 * m2CamDerivs as the last ProjectAndDerivs / LinearUpdate left them; in_image unspecified): what a FOLLOWING loop starts
 * from, because its iteration 0 does not re-project (src/Tracker.cc:617) — the coarse loop's points in the fine loop. */
int ptam_pose_gn_state(ptam_ctx* ctx, int n, const ptam_pose_meas* meas, const ptam_projection* entry,
                       double pose_inout[12], const ptam_gn_opts* opts, int32_t* outlier_flags, double* updates_out,
                       ptam_projection* state_out);

/* device-resident variant: every pointer is a device pointer (d_entry, d_outlier_flags, d_updates nullable; d_updates
 * holds 32*6 doubles), asynchronous on the context's stream — the measurements of a tracked frame are produced on
 * the device (patch search / sub-pixel results), so the frame needs no upload and only the 96-byte pose comes back.
 * n must be >= 1. */
int ptam_pose_gn_dev(ptam_ctx* ctx, int n, const ptam_pose_meas* d_meas, const ptam_projection* d_entry,
                     double* d_pose_inout, const ptam_gn_opts* opts, int32_t* d_outlier_flags, double* d_updates);

/* The same with the measurement count in device memory (d_n, clamped to [0, n_cap]; 0 = pose unchanged, zero updates,
 * src/Tracker.cc:955-956): the list ptam_gather_pose_meas_dev compacted is consumed without a host round trip.
 * Outlier flags are written for the first *d_n entries only.  pose_host_in (nullable, HOST pointer, 12 doubles): the entry
 * pose (the motion model's prediction) handed over as a kernel argument instead of being read from d_pose_inout — no
 * copy of its own.  pose_host_out (nullable, HOST pointer, 12 doubles): when
 * given, the call returns once the refined pose has arrived there — the kernel writes it into host-mapped memory, so a
 * tracked frame ends with one PCIe write instead of a D2H copy + stream synchronise; d_pose_inout is updated either way. */
int ptam_pose_gn_dev_counted(ptam_ctx* ctx, int n_cap, const int32_t* d_n, const ptam_pose_meas* d_meas,
                             const ptam_projection* d_entry, double* d_pose_inout, const ptam_gn_opts* opts,
                             int32_t* d_outlier_flags, double* d_updates, const double* pose_host_in, double* pose_host_out);

/* ---- Tracker::SearchForPoints' bookkeeping for a batch (src/Tracker.cc:883-909), device resident, asynchronous:
 *      query i with level >= 0 whose patch was found (d_results[i].found) — and, when d_subpix is given, whose
 *      sub-pixel refinement converged (:898-904) — becomes the next pose measurement, in query order:
 *      {v3WorldPos_i, v2Found = coarse position (:908) or sub-pixel position (:905), dSqrtInvNoise = 1 / LevelScale(level) (:889)}.
 *      d_world: the points' world positions, 3 doubles every world_stride_bytes (24 for packed xyz, sizeof(ptam_pvs_point) to
 *      read them out of the PVS input).  d_src_index (nullable): query index of every measurement (routes the outlier flags of
 *      the pose solve back to the map points).  d_count: number of measurements written.  d_level_found (nullable, 4 ints):
 *      manMeasFound per level (:892, :901). */
int ptam_gather_pose_meas_dev(ptam_ctx* ctx, int n, const ptam_patch_query* d_queries, const ptam_patch_result* d_results,
                              const ptam_subpix_result* d_subpix, const void* d_world, int world_stride_bytes,
                              ptam_pose_meas* d_meas_out, int32_t* d_src_index, int32_t* d_count, int32_t* d_level_found);

/* ---- Tracker::TrackMap (src/Tracker.cc:442-696) as ONE device-resident chain ------------------------------------------
 *      PVS loop -> choice of the coarse / top-level / fine search sets -> coarse SearchForPoints (range 30, sub-pixel) ->
 *      ten coarse pose iterations -> re-projection + SearchForPoints of the other sets -> ten fine pose iterations ->
 *      measurement and scene-depth bookkeeping.  List lengths, the mbDidCoarse decision and the fine search range are taken
 *      on the device; the call enqueues everything at once and returns when the result block has arrived (host-mapped
 *      memory, no copy).  The map (world positions, pixel vectors, patch sources) stays resident between frames, and so
 *      does every point's PatchFinder (TrackerData::Finder): MakeTemplateCoarseCont keeps a point's search template — and
 *      its mbTemplateBad — from frame to frame while neither column of the warp moves by more than 0.07
 *      (src/PatchFinder.cc:98-127), a warp rejected by CalcSearchLevelAndWarpMatrix leaves mbTemplateBad up until the next
 *      re-make (:78-81).  ptam_tracker_set_map starts every finder afresh. */
typedef struct ptam_tracker ptam_tracker;
typedef struct {
    int32_t try_coarse;         /* bTryCoarse after the caller's heuristics (src/Tracker.cc:505-516: DisableCoarse, velocity,
                                   just-recovered — then the caller also doubles coarse_max / coarse_range) */
    uint32_t coarse_min;        /* Tracker.CoarseMin 20        :492 */
    uint32_t coarse_max;        /* Tracker.CoarseMax 60        :493 */
    uint32_t coarse_range;      /* Tracker.CoarseRange 30      :494 */
    int32_t coarse_subpix_its;  /* Tracker.CoarseSubPixIts 8   :495 */
    int32_t max_patches;        /* Tracker.MaxPatchesPerFrame 1000  :593 */
    int32_t estimator;          /* Tracker.MEstimator */
    int32_t pad_;
} ptam_trackmap_opts;
void ptam_trackmap_opts_default(ptam_trackmap_opts* o);
typedef struct {
    double pose[12];            /* mse3CamFromWorld after the fine stage */
    int32_t did_coarse;         /* mbDidCoarse */
    int32_t n_pvs[4];           /* avPVS[l].size() after the PVS loop */
    int32_t attempted[4];       /* manMeasAttempted */
    int32_t found[4];           /* manMeasFound */
    int32_t n_coarse, n_top, n_fine;   /* sizes of the coarse set, of the remaining top-level set and of the fine set */
    int32_t n_meas;             /* found entries of vIterationSet = measurements of the fine pose loop */
    int32_t depth_n;            /* number of found points in the two sums below */
    int32_t templates_reused;   /* searched patches whose PatchFinder kept last frame's template (src/PatchFinder.cc:103-111) */
    int32_t pad_;
    double depth_sum, depth_sum_sq;   /* sums of v3Cam[2] and its square over the found points (:680-690) */
} ptam_trackmap_result;
/* one entry of vIterationSet, in its order (coarse set, top-level set, fine set) */
typedef struct {
    int32_t point;              /* map point index */
    int32_t level;              /* nSearchLevel (-1: bad template, not searched) */
    int32_t found;              /* bFound */
    int32_t did_subpix;         /* bDidSubPix */
    int32_t outlier;            /* Weight() == 0 on the fine loop's last iteration (:640, CalcPoseUpdate bMarkOutliers) */
    int32_t pad_;
    double v2_found[2];         /* v2Found, level-0 pixels (valid iff found) */
} ptam_trackmap_meas;
int ptam_tracker_create(ptam_ctx* ctx, int max_points, ptam_tracker** out);
int ptam_tracker_destroy(ptam_tracker* t);
/* the map: world position + pixel vectors per point, and its patch source (src_kf, src_level, center_x / center_y of
 * ptam_template_query; the other fields are ignored).  The source keyframes must stay alive while the tracker uses them. */
int ptam_tracker_set_map(ptam_tracker* t, int n, const ptam_pvs_point* points, const ptam_template_query* sources);
/* The map after the mapmaker changed it (points added at a new keyframe, bad points removed, positions refined by a bundle
 * adjustment): like ptam_tracker_set_map, but a point that was in the previous map keeps its TrackerData — prev_index[i] is the
 * index new point i had in the map of the last set_map / update_map call, -1 for a new point.  Its PatchFinder's template, warp
 * matrix and mbTemplateBad carry over as they do in the reference, where TrackerData lives as long as its MapPoint
 * (include/Tracker.h:42-67, src/Tracker.cc:453-464); new points start with a fresh finder.  No old index may appear twice.
 * Both calls clear the tracker's serial list (ptam_tracker_take_map, below): the points handed over here have no identity the
 * resident map knows, and the next take treats every point as new.  With the map in a ptam_rmap on the same device,
 * ptam_rmap_publish / ptam_tracker_take_map do this hand-over without the host tables and without a composed prev_index. */
int ptam_tracker_update_map(ptam_tracker* t, int n, const ptam_pvs_point* points, const ptam_template_query* sources,
                            const int32_t* prev_index);
/* The frame's random orders, each a permutation of 0..n-1 (asynchronous upload): level l's PVS list is taken in the order
 * its members appear in shuffle_levels (replaces std::random_shuffle of avPVS[l], :483-484), the chop of the fine set to
 * MaxPatchesPerFrame in the order of shuffle_fine (:597-600).  Identity until set. */
int ptam_tracker_set_shuffle(ptam_tracker* t, const int32_t* shuffle_levels, const int32_t* shuffle_fine);
/* The same two orders drawn ON THE DEVICE, on the tracker's queue: nothing proportional to the map is made, checked or uploaded
 * by the host, and the call waits for nothing.  For order w (0: shuffle_levels, 1: shuffle_fine) and point i the key is
 *     (hi32(splitmix64(seed, ((2 * frame + w) << 32) | i)) << 32) | i
 * with splitmix64(seed, k) the k-th output of the generator whose state starts at seed (as ptam_mapmaker_opts' failure draw;
 * 2 * frame + w is taken modulo 2^32); the order is the low words of the n keys sorted ascending.  The keys are distinct, so the
 * order is total and a permutation by construction.  Maps of at most 8192 points: one launch, a workgroup per order, keys made
 * and sorted in LDS; larger maps: one launch for the keys, the device's 64-bit key sort per order, one launch for the low words.
 * n == 0: nothing happens.  ptam_tracker_set_shuffle afterwards replaces the orders and the other way round; a new map of
 * another size resets them to the identity, as before. */
int ptam_tracker_draw_shuffles(ptam_tracker* t, uint64_t seed, uint64_t frame);
/* The two orders the tracker's next frame will use, n entries each, however they were set: a copy on the tracker's queue, which is
 * waited for — from the device arrays after a draw, a take or a set_shuffle of a map of more than 8192 points; after a set_shuffle
 * of a smaller map from the host-mapped copy that call keeps (read through the queue as well, so behind whatever is enqueued). */
int ptam_tracker_read_shuffle(ptam_tracker* t, int32_t* shuffle_levels, int32_t* shuffle_fine);
/* The definition the device is held to, in plain host code (no device, no tracker): order `which` (0 / 1) of n points into
 * out[0..n-1].  PTAM_E_ARG: which outside 0..1, n < 0, out NULL with n > 0. */
int ptam_shuffle_order_host(uint64_t seed, uint64_t frame, int which, int n, int32_t* out);
int ptam_track_map(ptam_tracker* t, const ptam_kf* current, const double pose_in[12], const ptam_trackmap_opts* opts,
                   ptam_trackmap_result* out);
/* A whole tracked frame in one call: KeyFrame::MakeKeyFrame_Lite (src/KeyFrame.cc:18-54) of the device-resident image
 * d_frame (stride == width) into `current`, then TrackMap against it: one entry, one queue, one wait. */
int ptam_track_map_frame(ptam_tracker* t, ptam_kf* current, const uint8_t* d_frame, const double pose_in[12],
                         const ptam_trackmap_opts* opts, ptam_trackmap_result* out);
/* ---- the tracker's motion model and Tracker::TrackFrame's tracking branch (src/Tracker.cc:134-137) ----------------------
 *      Host scalar code (no device work of its own): the decaying constant-velocity model of :1008-1056 and the bTryCoarse
 *      heuristics of :505-516, kept in a plain struct the caller owns.  ptam_motion_predict / ptam_track_frame are the model with
 *      the SmallBlurryImage rotation estimator (Tracker.UseRotationEstimator, :1017-1028) switched off — the velocity comes from
 *      the last two tracked poses alone; ptam_motion_predict_sbi / ptam_track_frame_sbi below are the model with it on. */
typedef struct {
    double pose[12];               /* mse3CamFromWorld */
    double start_pose[12];         /* mse3StartPos: the pose before the prediction, :1015 */
    double velocity[6];            /* mv6CameraVelocity (translation, rotation) */
    double msd_scaled_velocity;    /* mdMSDScaledVelocityMagnitude, :1052-1055 */
    double scene_depth_mean;       /* mCurrentKF.dSceneDepthMean (1.0 after a reset, :56), updated when more than 20 points were found, :692-696 */
    double scene_depth_sigma;      /* mCurrentKF.dSceneDepthSigma */
    double coarse_min_velocity;    /* Tracker.CoarseMinVelocity 0.006, :496 */
    int32_t use_constant_velocity; /* Tracker.UseConstantVelocity 1, :1041 */
    int32_t disable_coarse;        /* Tracker.DisableCoarse 0, :495 */
    int32_t just_recovered;        /* mbJustRecoveredSoUseCoarse: the next frame tries the coarse stage with doubled CoarseMax / CoarseRange, :508-513 */
    int32_t pad_;
} ptam_motion_model;
/* Tracker::Reset's part of the model (:52-56): pose = the given one, zero velocity, depth mean 1, default tunables */
void ptam_motion_reset(ptam_motion_model* m, const double pose[12]);
/* Tracker::PredictPoseWithMotionModel :1013-1030: start_pose = pose; pose = exp(velocity) * start_pose */
void ptam_motion_predict(ptam_motion_model* m);
/* the end of TrackMap (:692-696: scene depth from the frame's sums when depth_n > 20) + Tracker::UpdateMotionModel :1036-1056 with
 * pose = r->pose: velocity = ln(pose * start_pose^-1) (or its decaying mix), msd_scaled_velocity = |(v_t / depth mean, v_w)| */
void ptam_motion_update(ptam_motion_model* m, const ptam_trackmap_result* r);
/* TooN SE3<>::exp / SE3<>::ln on (R row-major | t) poses; mu = (translation part, rotation vector) */
void ptam_se3_exp(const double mu[6], double pose_out[12]);
void ptam_se3_ln(const double pose[12], double mu_out[6]);
/* One tracked frame of a camera that moves (src/Tracker.cc:134-137 with :94 before them): MakeKeyFrame_Lite of the
 * device-resident frame into `current`, PredictPoseWithMotionModel, the bTryCoarse heuristics (*opts is the caller's tunables;
 * its try_coarse is ignored and decided here, coarse_max / coarse_range doubled after a recovery), TrackMap from the predicted
 * pose, UpdateMotionModel.  m->pose is the tracked pose afterwards.  A call that returns an error leaves *m untouched (the
 * model is advanced on a copy and committed on success): the frame can be retried. */
int ptam_track_frame(ptam_tracker* t, ptam_kf* current, const uint8_t* d_frame, ptam_motion_model* m,
                     const ptam_trackmap_opts* opts, ptam_trackmap_result* out);

/* ---- SmallBlurryImage (src/ImageProcess.cc:255-495), Relocaliser (src/Relocaliser.cc:12-38) and the tracker's rotation
 *      estimator (src/Tracker.cc:94-108, :1016-1028) ----------------------------------------------------------------------
 *      An SBI is halfSample(aLevels[3].im) — (level-3 size) / 2 by integer division, 40x30 for a 640x480 frame —, its mean
 *      (exact unsigned sum, float division), the float template `small - mean` blurred by convolveGaussian, and the central
 *      differences (r - l, d - u) of the template without the 0.5, zero on the one-pixel border.  The Jacobians are always made:
 *      there is no mbMadeJacs to forget.  Limits: at most 4096 pixels and 256 a side (PTAM_E_LIMIT), at least 3x3.
 *      Three libCVD rules are restated here as the project's own and are UNPINNED (libCVD is not vendored by the reference and
 *      no build of it has confirmed them):
 *        halfSample        the context's variant (ptam_ctx_set_halfsample), the pyramid's routine;
 *        transform/sample  as in ptam_make_templates_batch: p0 = inOrig - M * outOrig, then `across` added per pixel and the carriage
 *                          return per row by repeated fp64 addition; a sample is inside iff 0 <= p.x, 0 <= p.y, p.x < w - 1,
 *                          p.y < h - 1 (or the whole image's bounding box is); the bilinear blend in fp64, rounded once to float32
 *                          (not truncated to a byte); outside: the default value -9e20f;
 *        convolveGaussian  k = ceil(3 sigma) taps each side, weights exp(-i^2 / 2 sigma^2) normalised to sum 1 in fp64 on the host;
 *                          a row pass then a column pass, fp64 between them, taps in ascending order; pixels outside the image
 *                          count as 0, nothing is renormalised at the border; rounded once to float32.  0 < sigma <= 5, else
 *                          PTAM_E_ARG.
 *      Sums over pixels are reduced in a fixed order: two calls on the same input give the same bits. */
typedef struct ptam_sbi ptam_sbi;   /* one SmallBlurryImage, device-resident */
int ptam_sbi_create(ptam_ctx* ctx, int frame_w, int frame_h, ptam_sbi** out);
int ptam_sbi_destroy(ptam_sbi* s);
/* SmallBlurryImage::MakeFromKF (:279-304) + MakeJacs (:170-191) from kf's level 3; one launch, asynchronous.  blur: 2.5 for
 * keyframes and the relocaliser (include/ImageProcess.h:57-58), Tracker.RotationEstimatorBlur = 0.75 for the per-frame pair.
 * PTAM_E_ARG: a keyframe of another device or frame size.  The kernel reads the keyframe's level 3 on THIS object's context's queue: a
 * keyframe made on another context's queue must be synchronised by the caller first (ptam_ctx_sync of that context); the same holds
 * for ptam_sbi_bank_add, ptam_sbi_bank_add_batch and ptam_relocalise. */
int ptam_sbi_make(ptam_sbi* s, const ptam_kf* kf, double blur);
int ptam_sbi_size(const ptam_sbi* s, int* w, int* h);   /* mirSize */
/* mimSmall (w*h bytes), mimTemplate (w*h floats), mimImageJacs (w*h x 2 floats: x, y per pixel); NULL pointers are skipped.
 * PTAM_E_STATE before the first make. */
int ptam_sbi_read(ptam_sbi* s, uint8_t* small, float* tmpl, float* jacs);

typedef struct {
    double se2_rot[4], se2_trans[2];   /* se2CtoC: rotation matrix row-major, translation */
    double score, mean_offset;         /* dFinalScore: the LAST formed sums' sum of dDiff^2 (taken before that iteration's update); dMeanOffset */
    double rotation[9];                /* SE3fromSE2(se2CtoC): the rotation, row-major (its translation is zero) */
    int32_t iterations_done;           /* iterations whose update was applied */
    int32_t n_used;                    /* pixels that entered the last formed sums */
    int32_t degenerate, pad_;
} ptam_sbi_alignment;
/* SmallBlurryImage::CalcSBIRotation (:485-495) = IteratePosRelToTarget (:313-417; the reference passes 6 iterations) + SE3fromSE2
 * (:427-476) with the context's camera at the SBI's size; one launch (all iterations, fp64 sums, the 4x4 Cholesky, the SE2 update),
 * one wait for the result block in host-mapped memory.  1 <= iterations <= 64.
 * Degenerate systems, which the reference divides by: when a pivot of the Cholesky is not strictly positive (a blank frame: all
 * gradients zero; a warp that leaves no pixel inside) the iteration stops, the SE2 of the previous iteration stands and
 * degenerate = 1; score and rotation are finite.  An SE2 that is exactly the identity gives exactly the identity rotation (the
 * reference's three Gauss-Newton steps would leave the ~1e-17 of Project(UnProject(p)) - p in it).  A step that is not finite (the
 * update, or the SE2 and mean offset it would give: a tiny positive pivot) ends the iteration in the same way, degenerate = 1. */
int ptam_sbi_calc_rotation(ptam_sbi* current, const ptam_sbi* target, int iterations, ptam_sbi_alignment* out);

/* The map's keyframe SBIs (KeyFrame::MakeKeyFrame_Rest, src/KeyFrame.cc:80-81: pSBI = new SmallBlurryImage(*this); pSBI->MakeJacs)
 * side by side in device memory, in the order they were added = the order of Map::vpKeyFrames. */
typedef struct ptam_sbi_bank ptam_sbi_bank;
int ptam_sbi_bank_create(ptam_ctx* ctx, int frame_w, int frame_h, int capacity, ptam_sbi_bank** out);
int ptam_sbi_bank_destroy(ptam_sbi_bank* b);
/* one make launch into the next entry, asynchronous; *index (nullable): the entry.  PTAM_E_LIMIT: the bank is full.  PTAM_E_STATE
 * (this call and the next): the entries came from ptam_sbi_bank_take_keyframes and the bank has not been cleared since. */
int ptam_sbi_bank_add(ptam_sbi_bank* b, const ptam_kf* kf, double blur, int* index);
/* n keyframes into the next n entries with ONE make launch (grid x = n), asynchronous; *first_index (nullable): the first entry.
 * PTAM_E_LIMIT: fewer than n entries are free; nothing is added. */
int ptam_sbi_bank_add_batch(ptam_sbi_bank* b, int n, const ptam_kf* const* kfs, double blur, int* first_index);
int ptam_sbi_bank_count(const ptam_sbi_bank* b, int* n);
typedef struct {
    int32_t best, good;     /* mnBest; AttemptRecovery's return value: align.score < max_score */
    double best_ssd;        /* mdBestScore */
    double pose[12];        /* mse3Best = rotation * se3CfromW(best) */
    ptam_sbi_alignment align;
} ptam_reloc_result;
/* Relocaliser::AttemptRecovery (src/Relocaliser.cc:12-38, called at src/Tracker.cc:171): the current keyframe's SBI into `scratch`
 * (blur 2.5), SSDofImgs (src/ImageProcess.cc:88-105: difference in float, sum in double) against every entry — one workgroup each —,
 * the first entry with the strictly lowest SSD, CalcSBIRotation against it, pose = rotation * kf_poses12[best].  The arg-min is taken
 * at the start of the align launch: make, SSD and align launches, one wait.  kf_poses12: host, count x 12.  max_score:
 * Reloc2.MaxScore, 9e6.  ssd_out (nullable): count doubles.  PTAM_E_STATE: an empty bank. */
int ptam_relocalise(ptam_sbi_bank* b, ptam_sbi* scratch, const ptam_kf* current, const double* kf_poses12, double blur, double max_score,
                    ptam_reloc_result* out, double* ssd_out);

/* mpSBILastFrame / mpSBIThisFrame (src/Tracker.cc:94-108): two SBIs and which of them is last frame's */
typedef struct ptam_rotation_estimator ptam_rotation_estimator;
int ptam_rotation_estimator_create(ptam_ctx* ctx, int frame_w, int frame_h, double blur /* Tracker.RotationEstimatorBlur 0.75 */,
                                   ptam_rotation_estimator** out);
int ptam_rotation_estimator_destroy(ptam_rotation_estimator* e);
/* the next frame is both "this" and "last" (:98-102): its rotation is the identity */
int ptam_rotation_estimator_reset(ptam_rotation_estimator* e);
/* Tracker::PredictPoseWithMotionModel (:1013-1029) with mbUseSBIInit: start_pose = pose; v = velocity with v[3..5] = ln(rotation),
 * v[0] = v[1] = 0 (v[2] stays); pose = exp(v) * start_pose */
void ptam_motion_predict_sbi(ptam_motion_model* m, const double rotation[9]);
/* Tracker::AttemptRecovery (:196-207) after a good ptam_relocalise: pose = start_pose = the given pose, zero velocity, just_recovered */
void ptam_motion_recover(ptam_motion_model* m, const double pose[12]);
/* ptam_track_frame with the rotation estimator switched on, the reference's default (Tracker.UseRotationEstimator = 1, :96):
 * ptam_make_keyframe_lite_dev of d_frame into `current`; this frame's SBI and its alignment against last frame's (two launches), one
 * mapped wait for the rotation; ptam_motion_predict_sbi and the bTryCoarse heuristics on the host, as ptam_track_frame has them;
 * ptam_track_map on the made keyframe; ptam_motion_update.  Two waits per frame instead of ptam_track_frame's one.  The model and the
 * estimator's last / this pair are advanced on copies and committed only when the frame was tracked: a call that fails leaves both
 * untouched.  align_out (nullable): the frame's alignment.  The estimator must belong to the tracker's context. */
int ptam_track_frame_sbi(ptam_tracker* t, ptam_kf* current, const uint8_t* d_frame, ptam_motion_model* m, ptam_rotation_estimator* e,
                         const ptam_trackmap_opts* opts, ptam_trackmap_result* out, ptam_sbi_alignment* align_out);

/* nb frames of nb independent trackers (own context, map, keyframe, prediction each) as ONE chain of launches on the first
 * tracker's queue: every kernel of the chain gets a second grid dimension, row i works on frame i.  Not part of the
 * reference's surface (it tracks one camera); it exists because a process gets four hardware queues and a tracked frame
 * occupies one for its whole dependent chain, so separate calls keep at most four frames in flight whatever the device has
 * idle.  Frame i's result is what ptam_track_map_frame(trackers[i], current[i], d_frames[i], poses_in + 12 i, opts) gives
 * (bit for bit when the batch's list capacities select the same pose-kernel instantiation as the single call: maps of equal
 * size do).  The trackers must sit on one device in DIFFERENT contexts with the same camera model, image size and halfSample
 * variant; set the frames' permutations beforehand (ptam_tracker_set_shuffle). */
int ptam_track_map_frames_batch(int nb, ptam_tracker* const* trackers, ptam_kf* const* current, const uint8_t* const* d_frames,
                                const double* poses_in, const ptam_trackmap_opts* opts, ptam_trackmap_result* out);
/* Tracker::TrackFrame's tracking branch for nb cameras as ONE chain of launches with one wait per camera: ptam_track_map_frames_batch
 * with the motion model, the bTryCoarse heuristics (:503-514) PER CAMERA, and the rotation estimator.  Frame i is
 *   with estimators[i]:     what ptam_track_frame_sbi(trackers[i], current[i], d_frames[i], &models[i], estimators[i], opts, ..) does —
 *                           this frame's SmallBlurryImage, its alignment and the prediction from the rotation are made on the device
 *                           (the device's asin / acos / sin / cos are not the host's: pose_in agrees with ptam_motion_predict_sbi to a
 *                           few ulps, and everything behind it is ptam_track_map_frame from info[i].pose_in, bit for bit);
 *   without (estimators == NULL or a NULL entry): what ptam_track_frame(trackers[i], ..) does, bit for bit.
 * opts: the tunables, shared by all frames; its try_coarse is ignored (every frame's is decided from its model).  The conditions of
 * ptam_track_map_frames_batch hold (one device, different contexts, the same camera model, image size and halfSample variant, nb in
 * 1..4096); estimators[i] must belong to trackers[i]'s context, no estimator may appear twice, and all share image size and blur.
 * All or nothing: the models and the estimators' last / this pairs are advanced on copies and committed when every frame of the batch
 * has arrived; a call that returns an error leaves every models[i] byte for byte as it was and every estimator where it was.  (As in
 * ptam_track_map_frames_batch the trackers' per-point PatchFinder state may already have moved.)  info (nullable): per frame the pose
 * TrackMap started from, the alignment and the heuristics as applied. */
typedef struct {
    double pose_in[12];          /* the predicted pose TrackMap started from (device-computed when an estimator is given) */
    ptam_sbi_alignment align;    /* this frame's alignment; all zero without an estimator */
    int32_t try_coarse;          /* the frame's heuristics as applied (:503-514) */
    uint32_t coarse_max, coarse_range;
    int32_t pad_;
} ptam_track_frame_info;
int ptam_track_frames_batch(int nb, ptam_tracker* const* trackers, ptam_kf* const* current, const uint8_t* const* d_frames,
                            ptam_motion_model* models /* nb, in/out */, ptam_rotation_estimator* const* estimators /* nullable; entries nullable */,
                            const ptam_trackmap_opts* opts, ptam_trackmap_result* out, ptam_track_frame_info* info /* nullable, nb */);
/* Test hook: the device's form of ptam_motion_predict_sbi (the one ptam_track_frames_batch runs in the align workgroup) on a table —
 * one launch, one thread per row: poses_out12 + 12 i = the pose ptam_motion_predict_sbi(models + i, rotations9 + 9 i) leaves in the
 * model.  The models are not changed.  The ranges of SO3::ln near pi, which no tracked sequence reaches, are run through this. */
int ptam_motion_predict_sbi_dev(ptam_ctx* ctx, int n, const ptam_motion_model* models, const double* rotations9, double* poses_out12);

/* ---- Tracker::TrackFrame for a good map (src/Tracker.cc:91-111, :127-176): tracking, loss and recovery per camera ----------------
 *      The tracker's state next to the motion model, and AssessTrackingQuality (:1062-1107); plain host code like ptam_motion_*. */
#define PTAM_TRACK_BAD 0
#define PTAM_TRACK_GOOD 1
typedef struct {
    ptam_motion_model model;
    int32_t lost_frames;            /* mnLostFrames */
    int32_t quality;                /* mTrackingQuality: PTAM_TRACK_BAD 0, PTAM_TRACK_GOOD 1 */
    int32_t frame;                  /* mnFrame */
    int32_t last_keyframe_dropped;  /* mnLastKeyFrameDropped; -20 after a reset (:62) */
} ptam_track_state;
/* Tracker::Reset :52-62: ptam_motion_reset, quality GOOD, no lost frames, frame 0, last_keyframe_dropped -20 */
void ptam_track_state_reset(ptam_track_state* s, const double pose[12]);
typedef struct {
    double quality_good;                   /* Tracker.TrackingQualityGood 0.3 */
    double quality_lost;                   /* Tracker.TrackingQualityLost 0.13 */
    double wiggle_scale;                   /* MapMaker::GetWiggleScale(), 0.1 */
    double wiggle_scale_depth_normalized;  /* mdWiggleScaleDepthNormalized (the map maker's; 0.1 here: the wiggle scale at unit depth) */
    double max_kf_dist_wiggle_mult;        /* MapMaker.MaxKFDistWiggleMult 0.05 (IsNeedNewKeyFrame, src/MapMaker.cc:754-763) */
    double reloc_blur;                     /* the relocaliser's SmallBlurryImage blur, 2.5 */
    double reloc_max_score;                /* Reloc2.MaxScore 9e6 */
} ptam_track_state_opts;
void ptam_track_state_opts_default(ptam_track_state_opts* o);
/* AssessTrackingQuality :1062-1107 on a frame's counts (ptam_trackmap_result.attempted / .found): quality and lost_frames move, nothing
 * else does, and lost_frames moves nowhere else.  closest_kf_dist (KeyFrameLinearDist to the closest keyframe) is read in the third
 * branch only (:1095-1100), where a camera within 10 wiggle scales of a keyframe KEEPS its previous quality.  opts nullable. */
void ptam_assess_tracking_quality(ptam_track_state* s, const int32_t attempted[4], const int32_t found[4], double closest_kf_dist,
                                  const ptam_track_state_opts* opts);

/* se3CfromW of the bank's entries first .. first + n - 1 (which must exist), kept in device memory (mse3Best is formed there by
 * ptam_track_frames_recover_batch) and in a host mirror (the closest-keyframe distance); the upload is asynchronous on the bank's
 * context's queue.  ptam_relocalise keeps taking its own host table.  ptam_sbi_bank_poses reads the mirror; PTAM_E_STATE where an
 * entry's pose was never set. */
int ptam_sbi_bank_set_poses(ptam_sbi_bank* b, int first, int n, const double* poses12);
int ptam_sbi_bank_poses(const ptam_sbi_bank* b, int first, int n, double* poses_out12);

#define PTAM_FRAME_TRACKED 0
#define PTAM_FRAME_RECOVERED 1
#define PTAM_FRAME_RECOVERY_FAILED 2
typedef struct {
    int32_t branch;                /* PTAM_FRAME_* */
    int32_t closest_kf;            /* ClosestKeyFrame (src/MapMaker.cc:736-752) of the tracked pose among banks[i]'s poses; -1 without them */
    double closest_kf_dist;        /* KeyFrameLinearDist (:696-703) to it; 0 without */
    int32_t need_new_keyframe;     /* IsNeedNewKeyFrame :754-763 — information only, as the reference has it commented out */
    int32_t want_keyframe;         /* quality == GOOD && frame - last_keyframe_dropped > 20 (:146-161 without the queue size) */
    ptam_track_frame_info frame;   /* PTAM_FRAME_RECOVERED: pose_in is the relocaliser's pose, align is zero (no alignment is run) */
    ptam_reloc_result reloc;       /* the recovery branches; zero for PTAM_FRAME_TRACKED */
} ptam_track_frame_state_info;
/* Tracker::TrackFrame for a good map, for nb cameras as ONE chain of launches with one wait per camera; each camera takes the branch its
 * own state selects, decided on the host before the launch.
 *   states[i].lost_frames < 3   the frame is what ptam_track_frames_batch does for it (out, info.frame and the model bit for bit), then
 *                               ptam_assess_tracking_quality on its counts and the keyframe decision (:146-166): the caller ANDs
 *                               want_keyframe with its queue size and sets last_keyframe_dropped = frame when it adds the keyframe.
 *   otherwise                   recovery (:168-176, :196-207, src/Relocaliser.cc:12-38) inside the same chain: MakeKeyFrame_Lite; the
 *                               estimator's pair advances (this frame's image is made, nothing is aligned); this frame's relocaliser
 *                               image goes into scratch[i] (opts' reloc_blur; a second make launch, enqueued only when a camera
 *                               recovers); its SSD against every entry of banks[i] (one launch for all recovering cameras); an align
 *                               workgroup in the estimators' align launch takes the first strictly lowest SSD, aligns against that
 *                               entry, forms pose = rotation * bank pose[best] exactly as ptam_relocalise does and decides
 *                               good = score < reloc_max_score.
 *       good    PTAM_FRAME_RECOVERED: TrackMap from that pose with try_coarse = 1 and doubled coarse_max / coarse_range (:508-513);
 *               the model is pose = the tracked pose, start_pose = the relocaliser's, zero velocity, just_recovered = 0, the scene
 *               depth of :692-696 (msd_scaled_velocity stays: no UpdateMotionModel, :171-175); AssessTrackingQuality follows.  The
 *               reference takes no keyframe decision on this branch: need_new_keyframe and want_keyframe are 0.
 *       else    PTAM_FRAME_RECOVERY_FAILED: the device skips the frame's TrackMap kernels (they read the workgroup's verdict from device
 *               memory; nothing is waited for or spun on): the tracker's per-point PatchFinder state, its iteration set and states[i]
 *               stay byte for byte but for states[i].frame, the estimator's pair still advances, out[i] is zero.
 * states[i].frame moves by one in every branch.  A batch without a recovering camera enqueues exactly ptam_track_frames_batch's launches.
 * banks[i]: needed (with every entry's pose set, ptam_sbi_bank_set_poses) for a recovering camera; for a tracking camera it is
 * optional and feeds closest_kf (walked on the host after the wait).  One bank may serve several cameras.  A recovering camera's bank
 * is read on the LEAD tracker's queue: the call waits for the bank's own context's queue first, so whatever was enqueued there (adds,
 * pose uploads) is seen; nothing else may use that queue during the call.  scratch[i]: the recovering camera's current image, none
 * twice.  Banks, scratches and estimators must sit on the trackers' device and have the frames' size.
 * PTAM_E_ARG / PTAM_E_STATE, decided before the first enqueue with everything where it was: a recovering camera without bank or
 * scratch, an empty bank (STATE), entries whose pose was never set (STATE), another device or image size, a scratch named twice, a
 * recovering camera in a batch whose coarse_max exceeds the fused pose kernels' 1024 entries.  As in ptam_track_frames_batch states and
 * estimators advance on copies and commit when every frame has arrived; an error leaves every states[i] byte for byte.
 * estimators, banks, scratch and info are nullable, as are their entries (banks / scratch: of cameras that are not lost). */
int ptam_track_frames_recover_batch(int nb, ptam_tracker* const* trackers, ptam_kf* const* current, const uint8_t* const* d_frames,
                                    ptam_track_state* states /* nb, in/out */, ptam_rotation_estimator* const* estimators,
                                    ptam_sbi_bank* const* banks, ptam_sbi* const* scratch, const ptam_trackmap_opts* opts,
                                    const ptam_track_state_opts* state_opts, ptam_trackmap_result* out, ptam_track_frame_state_info* info);
/* Test hook: the SSD table (mdBestScore's candidates, src/Relocaliser.cc:21-31) of the row-th recovering camera, in camera order, of the
 * last ptam_track_frames_recover_batch that `lead` (its trackers[0]) led: the first count entries of its bank.  PTAM_E_ARG: no such row,
 * or more entries than the row's bank held. */
int ptam_tracker_read_reloc_ssd(ptam_tracker* lead, int row, int count, double* ssd_out);
/* vIterationSet of the last frame (what :667-676 turns into mCurrentKF.mMeasurements): *n = its length; out (nullable)
 * receives up to cap entries. */
int ptam_tracker_read_iteration_set(ptam_tracker* t, ptam_trackmap_meas* out, int cap, int* n);

/* One Tracker::CalcPoseUpdate (src/Tracker.cc:928-1005) on caller-provided Jacobians. */
typedef struct {
    double found[2];
    double image[2];
    double sqrt_inv_noise;
    double jac[12];          /* m26Jacobian row-major 2x6 */
} ptam_pose_update_meas;
int ptam_calc_pose_update(ptam_ctx* ctx, int n, const ptam_pose_update_meas* meas,
                          double override_sigma_sq, int estimator, double prior,
                          double mu_out[6], int32_t* weight_zero_flags);

/* ---- Bundle (include/Bundle.h:106-152, src/Bundle.cc) -------------------------------------------- */
typedef struct {
    int32_t max_iterations;          /* Bundle.MaxIterations = 20          src/Bundle.cc:40 */
    double update_sq_conv_limit;     /* UpdateSquaredConvergenceLimit 1e-6  src/Bundle.cc:41 */
    double min_sigma;                /* Bundle.MinTukeySigma = 0.4          src/Bundle.cc:234 */
    int32_t estimator;               /* Bundle.MEstimator = Tukey           src/Bundle.cc:132 */
    int32_t verbose;                 /* Bundle.Cout                         src/Bundle.cc:42 */
    int32_t deterministic;           /* not in the reference: 1 = camera sums of pass 2 (src/Bundle.cc:315-321) in a fixed order —
                                        the accumulation kernel stores each measurement's weighted A (2x6) and epsilon, a
                                        camera-major pass adds them up; two runs of the same problem are then bit-identical.
                                        0 (default): LDS atomics, whose order differs from run to run in the last bits */
    int32_t pad_;
} ptam_ba_opts;
void ptam_ba_opts_default(ptam_ba_opts* o);

/* one lambda trial (the unit mnCounter counts, src/Bundle.cc:518); mirrors the cout line :508 */
typedef struct {
    double lambda;          /* mdLambda used by this trial */
    double sigma_sq;        /* mdSigmaSquared of the enclosing LM step */
    double err_old;         /* dCurrentError */
    double err_new;         /* dNewError */
    double sum_sq_update;   /* |da|^2 + |db|^2 */
    int32_t n_bad;          /* measurements flagged bBad in the enclosing step (so far) */
    int32_t accepted;       /* 1 if this trial's step was committed */
} ptam_ba_trial;

int ptam_ba_create(ptam_ctx* ctx, const ptam_ba_opts* opts, ptam_ba** out);
int ptam_ba_destroy(ptam_ba* ba);
/* Bundle::AddCamera src/Bundle.cc:46-63: returns the camera id (>= 0) */
int ptam_ba_add_camera(ptam_ba* ba, const double pose[12], int fixed);
/* Bundle::AddPoint src/Bundle.cc:66-79 (NaN point -> zeros): returns the point id (>= 0) */
int ptam_ba_add_point(ptam_ba* ba, const double pos[3]);
/* Bundle::AddMeas src/Bundle.cc:82-93; sigma_sq = 4^level (src/MapMaker.cc:879-880) */
int ptam_ba_add_meas(ptam_ba* ba, int cam, int point, const double found[2], double sigma_sq);
/* bulk marshalling of the same three calls (ids are assigned in array order) */
int ptam_ba_add_cameras(ptam_ba* ba, int n, const double* poses12, const uint8_t* fixed);
int ptam_ba_add_points(ptam_ba* ba, int n, const double* pos3);
int ptam_ba_add_measurements(ptam_ba* ba, int n, const int32_t* cam, const int32_t* point,
                             const double* found2, const double* sigma_sq);
/* Bundle::Compute src/Bundle.cc:116-158.  *abort_flag (nullable) is polled on the host between
 * device trials (src/Bundle.cc:134,338); a sharded bundle sums the flags of all ranks with every trial's
 * scalars and acts on the sum, so that all ranks stop at the same trial (one trial later than a local
 * test would).  *accepted_out = mnAccepted, always >= 0: the reference's `return -1` (src/Bundle.cc:149-150)
 * is dead code there — Do_LM_Step returns true unconditionally (:550), TooN's LDL^T signals nothing — and
 * a singular or non-finite system shows up as it does in the reference: NaN errors, rejected trials, and
 * (where the reference would loop for ever, :118-123) an early stop.  Errors of the call itself (< 0
 * status: PTAM_E_ARG for a duplicate measurement, HIP / communicator failures) are the return value, not
 * *accepted_out.  Like src/Bundle.cc:46-93 the device path bounds neither the cameras of a bundle nor the measurements of a
 * point (a point seen by more than 256 keyframes and more than ~600 free cameras take slower kernel forms). */
int ptam_ba_compute(ptam_ba* ba, const volatile unsigned char* abort_flag, int* accepted_out);
int ptam_ba_converged(const ptam_ba* ba);                    /* include/Bundle.h:115 */
int ptam_ba_get_point(const ptam_ba* ba, int n, double pos[3]);      /* src/Bundle.cc:613 */
int ptam_ba_get_camera(const ptam_ba* ba, int n, double pose[12]);   /* src/Bundle.cc:618 */
int ptam_ba_get_all(const ptam_ba* ba, double* poses12, double* points3);
/* GetOutlierMeasurements src/Bundle.cc:623: (point, camera) pairs in the reference's order
 * (LM step, then measurement insertion order).  Returns the count; writes up to cap pairs. */
int ptam_ba_get_outliers(const ptam_ba* ba, int32_t* point_cam_pairs, int cap);
int ptam_ba_get_trials(const ptam_ba* ba, ptam_ba_trial* out, int cap);   /* returns count */
int ptam_ba_counts(const ptam_ba* ba, int* n_cams, int* n_free_cams, int* n_points, int* n_meas);
/* Trials of this bundle that were run again with the launch-per-block-column form of the camera solve because the persistent
 * form (one launch whose workgroups hand tiles to each other through flags) gave up a wait — it needs all of its workgroups
 * resident, which a device shared with another process' solve may not grant.  The repeated trial's result is what the reference
 * computes; the rest of the adjustment keeps the slower form.  0 in normal operation (returned as the function's value). */
int ptam_ba_solve_fallbacks(const ptam_ba* ba);
/* The other deliberate deviation made observable.  The reference accepts a second measurement of a point by the same camera
 * (both stay in mMeasList, src/Bundle.cc:76-93, while the look-up table of :558-567 keeps the last one: the two are summed into
 * U, V and the gradients but only one reaches the Schur complement); here ptam_ba_prepare / ptam_ba_compute refuse such a bundle
 * with PTAM_E_ARG.  Returns how many measurements of the last prepare had a twin (0 for a bundle that was accepted). */
int ptam_ba_duplicates_refused(const ptam_ba* ba);
/* Operating switches of the camera solve, read from the environment once per process: PTAM_LDLT_NO_CHAIN=1 uses the
 * launch-per-block-column form everywhere (a device shared between processes that all adjust bundles); PTAM_CH_SPIN_LIMIT=<n> is
 * the number of looks (~1 us each, default 2^18) a workgroup of the persistent form takes before it gives up a wait.
 * A comparison switch of the bundle's trial, read once per process as well (the GPU tests compare the two forms on this library):
 * PTAM_UPDATE_LOADS_W=1 — the point update reads W back from the Jacobian pass' planes instead of rebuilding it in registers
 * (the form before docs/LOG_point_update.md; the same adjustment to the last few bits). */

/* profiling hooks used by bench.py: HIP-event timing of individual kernels on the ctx stream. */
enum {
    PTAM_K_PROJECT = 0,     /* K5 pass-1 project + e^2 */
    PTAM_K_SELECT = 1,      /* K6 order statistic */
    PTAM_K_JACOBIAN = 2,    /* K7 fused Jacobian + normal-equation accumulate (roofline kernel) */
    PTAM_K_VINV = 3,
    PTAM_K_SCHUR = 4,       /* K8 */
    PTAM_K_SOLVE = 5,       /* K9 */
    PTAM_K_UPDATE = 6,      /* K10 back-substitution + apply + new error */
    PTAM_K_EXCHANGE = 7,    /* sharded bundles only: the all-reduce of S|E (the path's one exchange step) */
    PTAM_K_COUNT = 8
};
int ptam_ba_set_profiling(ptam_ba* ba, int on);
int ptam_ba_kernel_time(const ptam_ba* ba, int kernel, double* total_ms, int* launches);
/* upload + build the device structures without running (Compute does this implicitly) */
int ptam_ba_prepare(ptam_ba* ba);
/* (measurement-only entry points — the K7 launch bracket, the native frame drivers — are declared in ptam_hip_bench.h) */

/* ---- MapMaker::BundleAdjustRecent / BundleAdjustAll / BundleAdjust (src/MapMaker.cc:768-933) as ONE call on flat map tables ----
 *      The caller keeps its map and hands over: every keyframe's se3CfromW and bFixed (vpKeyFrames order, the newest last =
 *      vpKeyFrames.back()), every point's v3WorldPos (vpPoints order) and the table of all keyframes' mMeasurements, sorted by
 *      (kf, point) with no repeated pair — the vpKeyFrames x std::map<MapPoint*> walk of :871-882 with index order in place of
 *      pointer order.  On the device:
 *        RECENT (:788-828): KeyFrameLinearDist (:696-703: camera centres of se3CfromW.inverse(), fp64, the reference's operation
 *          order without FMA contraction) from the newest keyframe to every other one, the 4 nearest by (distance, index)
 *          (partial_sort, :711-730; ties by index where the reference breaks them by KeyFrame*); adjust set = the newest
 *          keyframe + the non-fixed ones of the 4; points = every point an adjust keyframe measures; fixed set = every other
 *          keyframe that measures one of them.  A map of fewer than 8 keyframes: ran = 0 and nothing else happens (:790-793).
 *        ALL (:768-783): adjust = the non-fixed keyframes, fixed = the fixed ones, points = all points.
 *        Bundle order (:851-882): adjust cameras ascending by kf with their own bFixed, then the fixed cameras ascending
 *          (fixed = 1), the points ascending, the measurements in table order with sigma^2 = LevelScale(level)^2.
 *      Compute(abort_flag) runs with *opts as ptam_ba_compute does.  accepted > 0: the adjusted points and the poses of every
 *      bundle camera are written into points3 / kf_poses12 (:895-904); otherwise the tables are not touched.
 *      Outliers in GetOutlierMeasurements order (src/Bundle.cc:540, :623) with the routing of :916-932: GoodMeasCount starts as
 *      the point's number of table rows; <= 2 or SRC_ROOT -> POINT_BAD (count unchanged), else FAILURE_QUEUE for TRACKER /
 *      EPIPOLAR and NEVER_RETRY for the other sources, and the point's count drops by one.  The caller applies the actions
 *      (bBad, mvFailureQueue, sNeverRetryKFs, the erase from mMeasurements / sMeasurementKFs); the call erases nothing.
 *      PTAM_E_ARG, with nothing written: a table row out of order or repeated, an index out of range, a level outside 0..3,
 *      a source outside 0..4, outliers != NULL with outlier_cap < n_meas.  Single device only (no communicator).
 *      Synchronous: one host wait after the selection (sizes), those of Compute(), one at the end. */
typedef struct {
    int32_t kf, point;        /* index into the keyframe / point tables */
    int32_t level;            /* Measurement::nLevel 0..3 */
    int32_t source;           /* Measurement::Source (include/KeyFrame.h:50): TRACKER, REFIND, ROOT, TRAIL, EPIPOLAR = 0..4 */
    double root_pos[2];       /* Measurement::v2RootPos */
} ptam_map_meas;
enum { PTAM_MAP_BA_ALL = 0, PTAM_MAP_BA_RECENT = 1 };
enum { PTAM_MAP_SRC_TRACKER = 0, PTAM_MAP_SRC_REFIND = 1, PTAM_MAP_SRC_ROOT = 2, PTAM_MAP_SRC_TRAIL = 3, PTAM_MAP_SRC_EPIPOLAR = 4 };
enum { PTAM_MAP_OUT_POINT_BAD = 1, PTAM_MAP_OUT_FAILURE_QUEUE = 2, PTAM_MAP_OUT_NEVER_RETRY = 3 };
typedef struct { int32_t point, kf, action, meas; } ptam_map_outlier;   /* meas = row of the table */
typedef struct {
    int32_t ran;              /* 0: RECENT on a map of < 8 keyframes, nothing else happened */
    int32_t accepted;         /* Compute()'s mnAccepted */
    int32_t converged;        /* Bundle::Converged() */
    int32_t n_adjust, n_fixed, n_points, n_meas, n_outliers;   /* the bundle's cameras (adjust set, fixed set), points, measurements */
} ptam_map_ba_result;
/* cam_kf (nullable, room for n_kf): bundle camera id -> keyframe; point_ids (nullable, room for n_points): bundle point id -> point */
int ptam_map_bundle_adjust(ptam_ctx* ctx, const ptam_ba_opts* opts, int mode, int n_kf, double* kf_poses12, const uint8_t* kf_fixed,
                           int n_points, double* points3, int n_meas, const ptam_map_meas* meas,
                           const volatile unsigned char* abort_flag, ptam_map_ba_result* res, ptam_map_outlier* outliers,
                           int outlier_cap, int32_t* cam_kf, int32_t* point_ids);

/* ---- MapMaker::CalcPlaneAligner (src/MapMaker.cc:1100-1195), the first half of stage (8) of InitFromStereo (:397), on the point
 *      table (v3WorldPos, vpPoints order), fp64 throughout, two kernel launches, one host wait at the end:
 *      `trials` hypotheses (:1112-1149), each the plane through three points: v3Mean = 0.33333333 * (A + B + C) (that literal),
 *      v3Normal = (C - A) ^ (B - A); a normal whose squared length is exactly 0 skips the trial (:1128-1129), else it is
 *      normalised and the score is the sum over all points whose squared distance from v3Mean is not 0.0 (:1136-1137) of
 *      min(|v3Diff * v3Normal|, max_dist); the strictly smaller score wins, among equal scores the lowest trial.
 *      Inliers (:1152-1161): not at v3BestMean itself, and nearer the plane than max_dist (strictly).  Their mean, then their
 *      covariance about that mean (:1164-1173, two passes).  The normal is the eigenvector of the covariance's smallest
 *      eigenvalue by cyclic Jacobi (the reference: TooN SymEigen<3> over LAPACK, get_evectors()[0]), negated when its z is > 0
 *      (:1180-1181); rotation rows as in :1183-1187 (row 2 the normal, row 0 = e_x - n (e_x . n) normalised, row 1 = row 2 ^ row 0),
 *      translation -R * mean (:1189-1192).  max_dist stands for both literals 0.05 (:1140, :1159).
 *      The reference's operation order without FMA contraction; every sum over points is reduced in a fixed order: two calls
 *      on the same input give the same bits.
 *      The draw: the reference calls rand() (:1113-1119); here the triples are an input.  opts->samples: trials x 3 point
 *      indices; NULL: the table ptam_plane_samples(opts->seed, n, trials) — the splitmix64 of ptam_homography_samples started
 *      from state = seed, nA = next() % n, nB drawn again while it equals nA, nC drawn again while it equals nA or nB.
 *      Four places where the reference's behaviour is undefined are given a meaning here:
 *        n_points < 10 (:1103-1106 returns SE3<>()): PTAM_PLANE_TOO_FEW, nothing is drawn or scored;
 *        every trial skipped (:1146-1147 never run, :1154 reads an unassigned v3BestMean): PTAM_PLANE_DEGENERATE;
 *        an empty inlier set (:1167 divides by zero): PTAM_PLANE_DEGENERATE;
 *        a row 0 of zero length before normalize (:1186, the normal along x): PTAM_PLANE_DEGENERATE.
 *      With a status other than PTAM_PLANE_OK the aligner is the identity. */
enum { PTAM_PLANE_OK = 0, PTAM_PLANE_TOO_FEW = 1, PTAM_PLANE_DEGENERATE = 2 };
typedef struct {
    double   max_dist;          /* 0.05: src/MapMaker.cc:1140 and :1159 */
    int32_t  trials;            /* 100: MapMaker.PlaneAlignerRansacs (:1111) */
    uint64_t seed;              /* used when samples == NULL */
    const int32_t* samples;     /* trials x 3 point indices, or NULL */
} ptam_plane_opts;
typedef struct {
    int32_t status, n_points, n_inliers, best_trial /* -1: none */, trials_skipped, pad_;
    double  best_score;         /* dBestDistSquared of the winning trial; 0 without one */
    double  mean[3];            /* v3MeanOfInliers */
    double  normal[3];          /* v3Normal after the sign rule = row 2 of the rotation */
    double  eigenvalues[3];     /* of m3Cov, ascending */
} ptam_plane_info;
void ptam_plane_opts_default(ptam_plane_opts*);
/* out: trials x 3.  PTAM_E_ARG: out == NULL, n_points < 3, trials < 1.  Host only. */
int  ptam_plane_samples(uint64_t seed, int n_points, int trials, int32_t* out);
/* se3_aligner: R row-major, then t; info always; inlier_out (nullable): n_points bytes, 1 = vv3Inliers holds the point (all 0
 * where no inlier pass ran).  The workspace is the context's scratch, which grows on demand and stays.
 * PTAM_E_ARG, with nothing written: a null pointer (inlier_out excepted; points3 may be null with n_points == 0), n_points < 0,
 * trials < 1, max_dist <= 0, and with n_points >= 10 a sample index outside [0, n_points) or repeated inside its triple. */
int  ptam_calc_plane_aligner(ptam_ctx*, int n_points, const double* points3 /* host */, const ptam_plane_opts*,
                             double se3_aligner[12], ptam_plane_info* info, uint8_t* inlier_out);

/* ---- MapMaker::ApplyGlobalTransformationToMap (src/MapMaker.cc:463-472) on the map tables, one launch (one thread per keyframe
 *      and per point), one host wait: every se3CfromW becomes se3CfromW * se3NewFromOld.inverse() (TooN: the inverse is
 *      (R^T, -(R^T t)), the product (Rl Rr, tl + Rl tr)), every v3WorldPos becomes se3NewFromOld * v3WorldPos, both in place.
 *      With a source table MapPoint::RefreshPixelVectors (src/Map.cc:40-65) is then run per point against the NEW pose of its
 *      source keyframe, with v3Normal_NC = (0,0,-1) as everywhere here, and the rows come out as ptam_pvs_point — what
 *      ptam_tracker_set_map / ptam_tracker_update_map and the re-finder take as is.  `sources` and `out` are nullable together.
 *      PTAM_E_ARG, with nothing written: a null aligner, a negative count, a null table with a non-zero count, one of
 *      sources / out without the other, a src_kf outside [0, n_kf). */
typedef struct {
    int32_t src_kf, pad_;       /* pPatchSourceKF as an index into the keyframe table */
    double center_nc[3], one_right_nc[3], one_down_nc[3];   /* as ptam_new_map_point returns them */
} ptam_map_point_source;
int  ptam_map_apply_global_transform(ptam_ctx*, const double se3_new_from_old[12], int n_kf, double* kf_poses12, int n_points,
                                     double* points3, const ptam_map_point_source* sources, ptam_pvs_point* out);

/* ---- stage (8) of MapMaker::InitFromStereo (src/MapMaker.cc:397), ApplyGlobalTransformationToMap(CalcPlaneAligner()), as ONE
 *      call: the points go up once, the two kernels of ptam_calc_plane_aligner run, the kernel of
 *      ptam_map_apply_global_transform reads the aligner from device memory, everything comes down together: three launches,
 *      one host wait, the same bits as the two calls one after the other.  The tables are written only when info->status ==
 *      PTAM_PLANE_OK.  PTAM_PLANE_TOO_FEW: the reference applies the identity, so the tables stay as they are and `out`, if
 *      given, is filled from them.  PTAM_PLANE_DEGENERATE: nothing but se3_aligner (the identity), info and inlier_out is
 *      written.  PTAM_E_ARG: the refusals of both calls. */
int  ptam_map_align_to_plane(ptam_ctx*, const ptam_plane_opts*, int n_kf, double* kf_poses12, int n_points, double* points3,
                             const ptam_map_point_source* sources, ptam_pvs_point* out, double se3_aligner[12],
                             ptam_plane_info* info, uint8_t* inlier_out);

/* ---- MapMaker::RefreshSceneDepth (src/MapMaker.cc:1202-1219), stage (5) of InitFromStereo (:378-380), for EVERY keyframe of the
 *      table in one call: one launch (one workgroup per keyframe, its rows found in the sorted table, the sums in a fixed
 *      order), one host wait.  meas: the table of ptam_map_bundle_adjust, sorted by (kf, point) with no repeated pair (only kf
 *      and point are read).  Per keyframe, with z the third component of se3CfromW * v3WorldPos over its rows:
 *      depth_mean = sum z / n, depth_sigma = sqrt(sum z^2 / n - depth_mean^2).  The reference asserts nMeas > 2 (:1216); here
 *      n_meas tells the caller: a keyframe without a row gets 0 / 0 / 0, and a radicand that rounding made negative gives 0.
 *      PTAM_E_ARG, with nothing written: a null table with a non-zero count, a negative count, an index out of range, a row
 *      out of order or repeated. */
typedef struct {
    double  depth_mean, depth_sigma;   /* KeyFrame::dSceneDepthMean, dSceneDepthSigma */
    int32_t n_meas, pad_;
} ptam_scene_depth;
int  ptam_map_scene_depth(ptam_ctx*, int n_kf, const double* kf_poses12, int n_points, const double* points3, int n_meas,
                          const ptam_map_meas* meas, ptam_scene_depth* out /* n_kf */);

/* ---- MapMaker::ReFindInSingleKeyFrame / ReFindNewlyMade / ReFindFromFailureQueue (src/MapMaker.cc:1028-1081) as ONE call on the
 *      map tables.  The caller keeps its map and hands over: the keyframe handles and their se3CfromW (vpKeyFrames order), the
 *      point table (vpPoints order: pixel vectors, patch source as a keyframe INDEX, bBad), the table of all mMeasurements as
 *      ptam_map_bundle_adjust takes it, and the table of all sNeverRetryKFs entries, both sorted by (kf, point) with no repeated
 *      pair.  Index order stands in for pointer order.  The pairs, in visiting order:
 *        KEYFRAME (:1028-1040): work = one int32 keyframe index k (n_work == 1); the pairs (k, p), p = 0 .. n_points-1.  bBad is
 *          not looked at (:1031-1037).
 *        NEW_POINTS (:1046-1065): work = n_work point indices in mqNewQueue order, none repeated; a point with `bad` set adds one
 *          to n_bad_points and makes no pair (:1056-1059), every other one is paired with keyframes 0 .. n_kf-1 in turn.
 *        FAILURE_QUEUE (:1070-1081): work = n_work ptam_map_pair in any order; the call sorts them by (kf, point) (:1074, on the
 *          host: the list comes from there) and skips a pair equal to its predecessor (the reference's first visit has put it into
 *          one of the two sets).
 *      On the device, per pair: skip = (kf, point) is in meas or in never (:947-948, a binary search in each table); the pair
 *      record ptam_refind_pairs would have been given (pose, point, template source, point_id = point index); then the finder
 *      chain of ptam_refind_pairs itself, with `finder`'s state, which carries over to the next call of either entry.  No per-pair
 *      data is built on or copied from the host: the tables go up once per call.
 *      Passes: at most opts->max_pairs_per_pass pairs are in flight (0 or opts == NULL: 4096), in NEW_POINTS whole points (at
 *      least one): the per-pair work memory is bounded by the pass, the finder state carries from pass to pass.  *stop_flag
 *      (nullable) is read on the host before each pass is enqueued — mvpKeyFrameQueue.empty() per point (:1053); once it is set
 *      the call finishes what is enqueued and reports stopped = 1, the pairs visited (n_pairs) and, in NEW_POINTS, the work
 *      entries consumed (points_consumed, bad ones included).  No host wait between passes; two waits per call.
 *      Outputs, in visiting order: found_out = {kf, point, level, PTAM_MAP_SRC_REFIND, root_pos} with found_subpix (Measurement::
 *      bSubPix) beside it (:996-1011), never_out = every visited, non-skipped pair that failed (each failure path of :951-993).
 *      meas_merged / never_merged (nullable, each on its own; room for n_meas / n_never + the call's pair count): meas + the found
 *      rows, never + the new never pairs, each sorted by (kf, point) on the device — what the next ptam_map_bundle_adjust /
 *      ptam_map_scene_depth / ptam_map_refind takes as it is.  The same input gives the same bits.
 *      out_cap: at least the call's pair count (n_points | n_kf * n_work | n_work).  n_work == 0: PTAM_OK, zero counts, the
 *      merged tables are copies.
 *      PTAM_E_ARG, with nothing written and the finder state untouched: a table out of order or repeated, an index, level or
 *      source out of range, a null or foreign-device keyframe, a keyframe of another frame size than the context's, a repeated
 *      point in NEW_POINTS, n_work > 1 in KEYFRAME, a capacity that is too small, a null output with a non-zero pair count. */
enum { PTAM_MAP_REFIND_KEYFRAME = 0, PTAM_MAP_REFIND_NEW_POINTS = 1, PTAM_MAP_REFIND_FAILURE_QUEUE = 2 };
typedef struct {
    ptam_pvs_point pv;                                  /* v3WorldPos, v3PixelRight_W, v3PixelDown_W */
    int32_t src_kf, src_level, center_x, center_y;      /* pPatchSourceKF (index), nSourceLevel, irCenter */
    int32_t bad, pad_;                                  /* bBad */
} ptam_map_refind_point;
typedef struct { int32_t kf, point; } ptam_map_pair;
typedef struct { int32_t max_pairs_per_pass; /* 0: the library's default */ int32_t pad_; } ptam_map_refind_opts;
typedef struct {
    int32_t n_pairs, n_skipped, n_found, n_never;       /* visited = skipped + found + never */
    int32_t n_bad_points, n_template_kept, points_consumed, stopped;
} ptam_map_refind_result;
int ptam_map_refind(ptam_ctx*, ptam_refinder*, const ptam_map_refind_opts*, int mode, int n_kf, const ptam_kf* const* kfs,
                    const double* kf_poses12, int n_points, const ptam_map_refind_point* points, int n_meas, const ptam_map_meas* meas,
                    int n_never, const ptam_map_pair* never, int n_work, const void* work, const volatile unsigned char* stop_flag,
                    ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix, ptam_map_pair* never_out, int out_cap,
                    ptam_map_meas* meas_merged, ptam_map_pair* never_merged);

/* ---- The edits of the map tables between the ptam_map_* calls, each as ONE device call: the bundle's outliers
 *      (src/MapMaker.cc:916-932), MapMaker::HandleBadPoints with Map::MoveBadPointsToTrash (:131-153, src/Map.cc:20-30) and a
 *      call's new points (:679-688, :352-362).  With them one MapMaker::run() iteration (:57-114) is a sequence of table calls:
 *      every table one call returns is valid input for the next.
 *      Common to the three: the tables are host arrays that go up once; flags are set per row, the rows are compacted or merged
 *      in order on the device (an ordered multi-workgroup compaction: per-tile counts, a scan of the tile counts, a scatter) and
 *      the point column is remapped; one host wait at the end, and one before it where a count decides how much comes down.
 *      Every order is fixed: the same input gives the same bits.  All outputs are integer and bit-copy work.  Output buffers must
 *      not overlap input buffers.  The inputs are not modified (`bad` of ptam_map_apply_outliers and the columns of
 *      ptam_map_handle_bad_points excepted, which are in and out).  Rows behind the counts a call reports are not written. */

/* ---- the outlier loop of MapMaker::BundleAdjust (src/MapMaker.cc:916-932) applied to the tables.  meas / never: sorted by
 *      (kf, point), no repeated pair; failure: mvFailureQueue as it stands (any order, duplicates allowed); outliers: exactly
 *      what ptam_map_bundle_adjust returned for this meas; bad: n_points bytes, bBad, in and out.  Per outlier, in list order:
 *        PTAM_MAP_OUT_POINT_BAD      bad[point] = 1, the row stays (:921-922)
 *        PTAM_MAP_OUT_FAILURE_QUEUE  (kf, point) is appended to the failure queue, the row is erased (:925-926, :929-930)
 *        PTAM_MAP_OUT_NEVER_RETRY    (kf, point) enters the never table, the row is erased (:928-930)
 *      meas_out (room for n_meas): the surviving rows, in order.  never_out (room for n_never + n_outliers): the old and the new
 *      pairs, merged and sorted.  failure_out (room for n_failure + n_outliers): the old queue, then the new pairs in outlier order.
 *      On the device: one thread per outlier writes its row's flag and sets bad; the rows without a flag are compacted into
 *      meas_out; the rows flagged NEVER_RETRY are compacted into the new never pairs, which are sorted because the table is;
 *      the two sorted never lists are merged by the rule of ptam_map_refind's merge; the outliers with FAILURE_QUEUE are
 *      compacted in list order.
 *      PTAM_E_ARG, with nothing written: a table out of order or with a repeated pair, an index out of range, a level outside
 *      0..3, a source outside 0..4, an action outside 1..3, an outlier whose meas is outside the table or whose (kf, point) is not
 *      that row's, the same row named twice, a NEVER_RETRY pair that is already in never (a consistent map holds no pair in both
 *      sets, :947-948), a null pointer with a non-zero count (bad: with n_points > 0), a negative count. */
typedef struct {
    int32_t n_point_bad, n_failure_added, n_never_added;   /* outliers per action */
    int32_t n_meas_out, n_never_out, n_failure_out;        /* rows written */
} ptam_map_outliers_result;
int ptam_map_apply_outliers(ptam_ctx*, int n_kf, int n_points, int n_meas, const ptam_map_meas* meas, int n_never,
                            const ptam_map_pair* never, int n_failure, const ptam_map_pair* failure, int n_outliers,
                            const ptam_map_outlier* outliers, uint8_t* bad, ptam_map_outliers_result* res, ptam_map_meas* meas_out,
                            ptam_map_pair* never_out, ptam_map_pair* failure_out);

/* ---- MapMaker::HandleBadPoints (src/MapMaker.cc:131-153) with Map::MoveBadPointsToTrash (src/Map.cc:20-30) on the tables.
 *      bad (n_points bytes, nullable = all zero): bBad.  outlier_count / inlier_count (int32 per point, nullable together):
 *      nMEstimatorOutlierCount / nMEstimatorInlierCount, which the caller keeps from the tracker's iteration-set flags.
 *      A point is removed iff bad[i], or outlier_count[i] > 20 && outlier_count[i] > inlier_count[i] (:136).  The survivors keep
 *      their order (src/Map.cc:23-29 erases from the back).  Removing a point renumbers every later one:
 *        new_index (n_points int32)  the point's new index, -1 for a removed point
 *        kept (room for n_points)    survivor j's old index: the prevIndex of ptam_tracker_update_map for a tracker that last
 *                                    saw the whole old table
 *        meas_out (room for n_meas)  the rows of surviving points with `point` rewritten (:142-151); still sorted by (kf, point)
 *                                    because the remap is monotone
 *        never_out (room for n_never)  the same: a removed point's sNeverRetryKFs go with its pMMData
 *        new_queue (n_new point indices in mqNewQueue order, none repeated, nullable) -> new_queue_out (room for n_new): the
 *                                    surviving entries, rewritten, in order.  The reference leaves a removed point in the queue
 *                                    and skips it when it is popped (:1056-1059): n_new_dropped is what ptam_map_refind would
 *                                    have reported as n_bad_points
 *        failure (any order, duplicates allowed, nullable) -> failure_out (room for n_failure): the surviving pairs, rewritten, in
 *                                    order.  A DEFINED DEVIATION: the reference keeps the MapPoint pointer in mvFailureQueue and
 *                                    would re-find a trashed point; no later stage reads such a measurement (:876-877)
 *        columns (at most 8)         point-side tables with one row of row_bytes (a positive multiple of 4) per point — points3,
 *                                    the ptam_map_refind_point table, the ptam_map_point_source table, the two counts, whatever
 *                                    the caller keeps — each compacted IN PLACE: rows 0 .. n_kept-1 of data become the
 *                                    survivors' rows, the bytes behind them are not touched
 *      On the device: one thread per point marks; an ordered exclusive scan over the points gives new_index and kept; one ordered
 *      compaction with the remap per table and per queue; one gather per column, threads over (surviving row, dword).
 *      PTAM_E_ARG, with nothing written: the table refusals of ptam_map_apply_outliers, a repeated or out-of-range new_queue entry,
 *      one of the two count arrays without the other, more than 8 columns, a row_bytes that is not a positive multiple of 4, a
 *      null column.  (The compaction takes any table of fewer than 2^31 rows: there is no size refusal.) */
enum { PTAM_MAP_MAX_COLUMNS = 8 };
typedef struct { void* data; int32_t row_bytes; int32_t pad_; } ptam_map_column;
typedef struct {
    int32_t n_marked;                  /* points the counts marked that bad had not (:136-137) */
    int32_t n_removed, n_kept;
    int32_t n_meas_out, n_never_out, n_new_out, n_new_dropped, n_failure_out;
} ptam_map_bad_points_result;
int ptam_map_handle_bad_points(ptam_ctx*, int n_kf, int n_points, const uint8_t* bad, const int32_t* outlier_count,
                               const int32_t* inlier_count, int n_meas, const ptam_map_meas* meas, int n_never,
                               const ptam_map_pair* never, int n_new, const int32_t* new_queue, int n_failure,
                               const ptam_map_pair* failure, int n_columns, const ptam_map_column* columns,
                               ptam_map_bad_points_result* res, int32_t* new_index, int32_t* kept, ptam_map_meas* meas_out,
                               ptam_map_pair* never_out, int32_t* new_queue_out, ptam_map_pair* failure_out);

/* ---- the new points of ptam_add_map_points_epipolar (MapMaker::AddPointEpipolar, src/MapMaker.cc:670-685; target_source =
 *      PTAM_MAP_SRC_EPIPOLAR) or ptam_init_points_from_trails (InitFromStereo, :352-362; PTAM_MAP_SRC_TRAIL) into the tables.
 *      New point i gets index n_points + i; the new queue (mqNewQueue.push, :671) is that index range itself, in order.
 *      meas_out (room for n_meas + 2 n_made): meas with {src_kf, n_points + i, level, PTAM_MAP_SRC_ROOT, src_root_pos} and
 *      {target_kf, n_points + i, level, target_source, target_pos} inserted, each at the end of its keyframe's run because the new
 *      indices exceed all old ones: two upper-bound searches and one shifted copy, one thread per output row.
 *      points_out (nullable, n_made ptam_map_refind_point): pv = the record's point, src_kf, src_level = level, center_x / y,
 *      bad = 0.  sources_out (nullable, n_made ptam_map_point_source): src_kf and the record's three _nc vectors.
 *      PTAM_E_ARG, with nothing written: a table out of order or repeated, src_kf == target_kf, an index, level or source out of
 *      range, n_points + n_made >= 2^31 or n_meas + 2 n_made >= 2^31, a null pointer with a non-zero count, a negative count. */
int ptam_map_add_points(ptam_ctx*, int n_kf, int n_points, int n_meas, const ptam_map_meas* meas, int src_kf, int target_kf,
                        int target_source, int n_made, const ptam_new_map_point* made, ptam_map_meas* meas_out,
                        ptam_map_refind_point* points_out, ptam_map_point_source* sources_out);

/* ---- The resident map: the tables of the ptam_map_* calls kept in device memory from call to call ------------------------------
 *      A ptam_rmap owns, on its context's device, the keyframe side (se3CfromW, bFixed; the ptam_kf handles and a mirror of the
 *      poses and flags stay on the host), the point side (points3, the ptam_map_refind_point rows, the ptam_map_point_source
 *      rows, the bBad bytes, the two M-estimator counts), the measurement table and the never table, both sorted by (kf, point),
 *      mqNewQueue as point indices and mvFailureQueue as pairs.  A resident form ptam_rmap_X does what ptam_map_X does, through the
 *      same device kernels, on these tables: nothing proportional to a table crosses the host link, and the order and range rules
 *      the host-table forms walk on every call are checked once, on the device, by ptam_rmap_upload.  Every resident call keeps
 *      them, so every call finds valid tables.
 *      Redundant columns: points3 and refind_point.pv.world, bad and refind_point.bad, source.src_kf and refind_point.src_kf
 *      hold the same values.  ptam_rmap_upload refuses tables in which they differ; every call that writes one writes the other.
 *      Transactions: a call that can be refused by what the device finds writes each new table into the table's second buffer
 *      and, after its one wait has shown that no refusal was published, swaps the buffers on the host; rows appended behind a
 *      table's count are no part of the table until the count moves, after the same wait; the bytes of bad are set in place by a
 *      kernel that first reads the refusal word of the kernels launched before it; the accepted bundle's scatter and the count
 *      increments are in place, in calls nothing can refuse once they run.  A refused call (PTAM_E_ARG) leaves every table and
 *      count as it was; ptam_rmap_last_refusal names the row.
 *      Memory: ptam_rmap_reserve sets capacities in rows; a call that needs more doubles the table (device-to-device copy) —
 *      the only place a resident call allocates.  Work memory is the context's scratch.
 *      All calls are synchronous and belong to the context's thread.  The same input gives the same bits.
 *      One exception to the memory rule: ptam_rmap_bundle_adjust builds its bundle per call, as ptam_map_bundle_adjust does, from
 *      the context's cache of released bundle blocks (no allocation once a bundle of that size has run).
 *      The context must outlive the handle: ptam_rmap_destroy before ptam_ctx_destroy. */
typedef struct ptam_rmap ptam_rmap;
enum {   /* the tables, as ptam_rmap_download and ptam_rmap_last_refusal name them; one row is ... */
    PTAM_RMAP_KF_POSES = 0,      /* 12 doubles */
    PTAM_RMAP_KF_FIXED = 1,      /* 1 byte */
    PTAM_RMAP_POINTS3 = 2,       /* 3 doubles */
    PTAM_RMAP_REFIND_POINTS = 3, /* ptam_map_refind_point */
    PTAM_RMAP_SOURCES = 4,       /* ptam_map_point_source */
    PTAM_RMAP_BAD = 5,           /* 1 byte */
    PTAM_RMAP_OUTLIER_COUNT = 6, /* int32 */
    PTAM_RMAP_INLIER_COUNT = 7,  /* int32 */
    PTAM_RMAP_MEAS = 8,          /* ptam_map_meas */
    PTAM_RMAP_NEVER = 9,         /* ptam_map_pair */
    PTAM_RMAP_NEW_QUEUE = 10,    /* int32 */
    PTAM_RMAP_FAILURE = 11,      /* ptam_map_pair */
    PTAM_RMAP_TABLES = 12,
    PTAM_RMAP_OUTLIERS = 12      /* ptam_rmap_last_refusal only: the outlier list of ptam_rmap_apply_outliers */
};
typedef struct { int32_t n_kf, n_points, n_meas, n_never, n_new, n_failure; } ptam_rmap_counts_t;
typedef struct { int32_t point, level; double root_pos[2]; } ptam_map_kf_row;   /* one measurement of a new keyframe */
/* the bytes every resident call moves besides its arguments: the refusal and count words, down */
enum { PTAM_RMAP_WORD_BYTES = 64 };
/* an upper bound on the level record (image and corner-table addresses of the four levels) that ptam_rmap_refind sends per keyframe */
enum { PTAM_RMAP_KF_RECORD_BYTES = 512 };

int ptam_rmap_create(ptam_ctx*, ptam_rmap** out);   /* an empty map */
int ptam_rmap_destroy(ptam_rmap*);
/* capacities in rows, each at least the table's count; never shrinks.  PTAM_E_ARG: a negative capacity. */
int ptam_rmap_reserve(ptam_rmap*, int n_kf, int n_points, int n_meas, int n_never, int n_new, int n_failure);
int ptam_rmap_counts(const ptam_rmap*, ptam_rmap_counts_t* out);
/* Replaces the whole map.  kfs (nullable: no handles are kept), outlier_count / inlier_count (nullable together: zeros).  The
 * tables go up into the second buffers and are checked there by kernels, one thread per row against its predecessor and the
 * ranges: meas and never sorted by (kf, point) with no repeated pair, kf in [0, n_kf), point in [0, n_points), level 0..3,
 * source 0..4; failure in range; new_queue in range and without a repeated entry (a per-point owner word: atomicMin of the
 * entry's index, then a compare — the later entry of a repeated point offends); the redundant columns equal and src_kf in
 * range.  The lowest offending row of each table is published with atomicMin and read in the call's one wait: PTAM_E_ARG,
 * ptam_rmap_last_refusal = the first offending table in the order meas, never, new_queue, failure, refind_points and that
 * row, and the previous map stays as it was.  PTAM_E_ARG also for a negative count or a null table with a non-zero count. */
int ptam_rmap_upload(ptam_rmap*, int n_kf, const ptam_kf* const* kfs, const double* kf_poses12, const uint8_t* kf_fixed, int n_points,
                     const double* points3, const ptam_map_refind_point* points, const ptam_map_point_source* sources,
                     const uint8_t* bad, const int32_t* outlier_count, const int32_t* inlier_count, int n_meas,
                     const ptam_map_meas* meas, int n_never, const ptam_map_pair* never, int n_new, const int32_t* new_queue,
                     int n_failure, const ptam_map_pair* failure);
/* rows [first, first + count) of one table into dst.  PTAM_E_ARG: a range outside the table. */
int ptam_rmap_download(ptam_rmap*, int which, int first, int count, void* dst);
/* the device-decided refusal of the handle's last refused call: the table (or PTAM_RMAP_OUTLIERS) and the offending row */
int ptam_rmap_last_refusal(const ptam_rmap*, int* table, int* row);
/* running sums of every byte the handle's calls have copied over the host link, in either direction */
int ptam_rmap_traffic(const ptam_rmap*, unsigned long long* h2d_bytes, unsigned long long* d2h_bytes);

/* ptam_map_bundle_adjust on the resident tables: the selection, the id maps and the bundle's measurement chunks are built from
 * the handle's buffers; the O(K) camera list is marshalled from the host mirror.  accepted > 0: the scatter kernels write the
 * poses and points in place (nothing can refuse the call once they run), a kernel copies points3 into refind_point.pv.world,
 * and the K poses come down into the mirror; the caller fetches them with ptam_rmap_download.  Otherwise no table is touched.
 * The reference does not refresh the pixel vectors after a bundle (src/MapMaker.cc:895-904), and neither does this call.
 * outliers (nullable; outlier_cap >= n_meas), cam_kf, point_ids: as ptam_map_bundle_adjust.  ptam_rmap_traffic counts what this
 * layer copies: 32 + 4 n_kf bytes, the accepted poses, 16 bytes per outlier and point_ids down.  Up it adds a NOMINAL 97 bytes per
 * bundle camera (pose and flag, marshalled from the mirror): the bundle object's own transfers — its camera upload, Compute()'s
 * result words — happen inside ptam_ba_* and are not measured by the handle. */
int ptam_rmap_bundle_adjust(ptam_rmap*, const ptam_ba_opts* opts, int mode, const volatile unsigned char* abort_flag,
                            ptam_map_ba_result* res, ptam_map_outlier* outliers, int outlier_cap, int32_t* cam_kf, int32_t* point_ids);
/* ptam_map_refind on the resident tables, through `finder` (its state carries from call to call as with ptam_map_refind); the
 * keyframe handles are those given to ptam_rmap_upload / ptam_rmap_add_keyframe (PTAM_E_ARG if one is missing).  work: as
 * ptam_map_refind, or NULL for NEW_POINTS / FAILURE_QUEUE: the resident queue is the work, and afterwards points_consumed entries
 * are popped from the front of new_queue, or failure is cleared (src/MapMaker.cc:1080; not when the call was stopped).  The merged
 * tables are written into the second buffers and become the map's after the call's wait.  found_out / found_subpix / never_out
 * (nullable together; out_cap as ptam_map_refind when given) come down only when asked for.  The visiting order is the host's:
 * the resident queue comes down (4 bytes per new_queue entry plus its point's bBad byte, 8 bytes per failure pair; for a caller's
 * NEW_POINTS list its indices go up and a byte each comes down) and the pairs' work lists go up (8 bytes per good new point, 8
 * per failure pair), with one level record per keyframe (at most PTAM_RMAP_KF_RECORD_BYTES); 16 bytes of counts and the lists asked for come down.  Nothing
 * proportional to the measurement table moves. */
int ptam_rmap_refind(ptam_rmap*, ptam_refinder*, const ptam_map_refind_opts*, int mode, int n_work, const void* work,
                     const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out,
                     int32_t* found_subpix, ptam_map_pair* never_out, int out_cap);
/* ptam_rmap_refind(work = NULL) — MapMaker::ReFindNewlyMade / ReFindFromFailureQueue on the resident queue — with the visiting
 * order decided on the device: neither queue comes down and no work list goes up.  mode: PTAM_MAP_REFIND_NEW_POINTS or
 * PTAM_MAP_REFIND_FAILURE_QUEUE.  The result, the merged tables and the queue afterwards are those of ptam_rmap_refind(work = NULL);
 * no list comes down (ptam_rmap_refind is the call that returns them).
 *   NEW_POINTS      each entry's bBad byte is read where it lies; the good entries are compacted in queue order (the ordered
 *                   compaction of the table edits: tile counts, scan, scatter) into the points and their entry numbers; each
 *                   point's place among the good points in index order comes from a sort of the keys (point << 32 | place).
 *                   The host reads the count of good points — one word, in one wait — for the pair count and the passes
 *   FAILURE_QUEUE   the keys (kf << 32 | point) are sorted (:1074); duplicates stay, the pair kernel skips them as it does
 * The sort: tiles of 1024 keys, each sorted by one workgroup of 1024 threads (a bitonic network: lane exchanges inside a wave, LDS
 * across waves), then merge passes that place every key by a binary search in the sibling run.  Equal keys are equal records, so
 * the output is a function of the input alone.
 * A NEW_POINTS call that *stop_flag ended after it had visited a point reads one more word: that point's entry number, which says
 * how many entries are popped.
 * Moves up one level record per keyframe (at most PTAM_RMAP_KF_RECORD_BYTES each) when there is a pair to visit, and nothing else.
 * Moves down 4 bytes in NEW_POINTS with a non-empty queue, 16 bytes of counts when there is a pair to visit, and 4 bytes more in
 * the stopped case above.  No term grows with a queue's length. */
int ptam_rmap_refind_queue(ptam_rmap*, ptam_refinder*, const ptam_map_refind_opts*, int mode, const volatile unsigned char* stop_flag,
                           ptam_map_refind_result* res);
/* ptam_map_apply_global_transform on the resident tables (the re-anchoring call): the poses are written into the second buffer
 * and come down into the mirror, the points move in place, and every point's RefreshPixelVectors runs against its source
 * keyframe's new pose straight into the point rows' pv (pv.world included).  out_rows (nullable, n_points ptam_pvs_point): the
 * rows for ptam_tracker_set_map.  Moves 256 bytes up; 96 n_kf bytes and out_rows down. */
int ptam_rmap_apply_global_transform(ptam_rmap*, const double se3_new_from_old[12], ptam_pvs_point* out_rows);
/* ptam_map_apply_outliers on the resident tables; outliers: host.  The action and the row index of every outlier are checked on
 * the host (the list is there).  What needs the table is checked by a kernel launched before the flag kernel, one thread per
 * outlier: the row's (kf, point) is the outlier's; no row is named twice (owner word per row); a NEVER_RETRY pair is not in
 * never (binary search).  PTAM_E_ARG with ptam_rmap_last_refusal = (PTAM_RMAP_OUTLIERS, the lowest offending list index).
 * Moves n_outliers * 16 bytes up and PTAM_RMAP_WORD_BYTES down. */
int ptam_rmap_apply_outliers(ptam_rmap*, int n_outliers, const ptam_map_outlier* outliers, ptam_map_outliers_result* res);
/* ptam_rmap_bundle_adjust followed by ptam_rmap_apply_outliers on the list it routed, as ONE call (MapMaker::BundleAdjust with its
 * outlier loop, src/MapMaker.cc:768-933): the routed list stays where the routing kernel wrote it, in the call's work memory, and
 * the outlier stage's kernels read it there.  What ptam_rmap_apply_outliers reads off the list on the host — the outliers per action
 * — a kernel adds up (a ballot per wave and action, integer atomic adds: exact in any order; no atomic decides a position) into the
 * call's count words, which come down with the stage's one wait.  Every entry of the routed list names a row of the bundle's
 * selection and one of the three actions by construction; the checks that need the tables (the row's pair, no row twice, no
 * NEVER_RETRY pair already in never) run as in ptam_rmap_apply_outliers.  The bundle's outlier count is on the host when Compute()
 * returns: never and failure get room for that many more rows before the stage's first launch.
 * res: as ptam_rmap_bundle_adjust.  outliers_res: as ptam_rmap_apply_outliers on that list; of an empty list (zero outliers per
 * action, the three row counts as they stand) when the bundle did not run or reported none.
 * The tables and the mirror end exactly as after the two calls.  A refusal by the outlier stage (PTAM_E_ARG, ptam_rmap_last_refusal =
 * (PTAM_RMAP_OUTLIERS, the lowest offending list index)) leaves measurements, never, failure and bad as they were, while the accepted
 * bundle's scatter has happened and the mirror has followed it: what the two calls leave.
 * Moves a NOMINAL 97 bytes per bundle camera up, as ptam_rmap_bundle_adjust; down 32 + 4 n_kf bytes, 96 n_kf more when the bundle
 * was accepted, and PTAM_RMAP_WORD_BYTES more when the bundle reported an outlier.  No term grows with the outlier count. */
int ptam_rmap_bundle_adjust_routed(ptam_rmap*, const ptam_ba_opts* opts, int mode, const volatile unsigned char* abort_flag,
                                   ptam_map_ba_result* res, ptam_map_outliers_result* outliers_res);
/* ptam_map_handle_bad_points on the resident tables: the columns are the handle's six point-side tables (the surviving points'
 * bad bytes are zero by construction) and the serial column.  kept_out (nullable, room for n_points; the tracker's prevIndex) and new_index_out
 * (nullable, n_points) come down only when asked for.  Moves PTAM_RMAP_WORD_BYTES down, and what was asked for. */
int ptam_rmap_handle_bad_points(ptam_rmap*, ptam_map_bad_points_result* res, int32_t* kept_out, int32_t* new_index_out);
/* ptam_map_add_points on the resident tables; made: host.  The two run ends are found by a binary search in the resident table
 * in each thread of the row kernel.  The new points' rows go to the ends of the six point-side tables (points3 from the record's
 * point, zeros to bad and the counts), their indices to the end of new_queue.  Moves n_made * sizeof(ptam_new_map_point) up. */
int ptam_rmap_add_points(ptam_rmap*, int src_kf, int target_kf, int target_source, int n_made, const ptam_new_map_point* made);
/* The table side of MapMaker::AddKeyFrameFromTopOfQueue (src/MapMaker.cc:501-506): the keyframe gets index n_kf, and its
 * measurements (rows: host, sorted by point, none repeated; checked on the host) are appended at the table's end as
 * {n_kf, point, level, PTAM_MAP_SRC_TRACKER, root_pos}.  kf (nullable): the handle kept for it.  Moves 97 + n_rows * 24 bytes up. */
int ptam_rmap_add_keyframe(ptam_rmap*, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows, const ptam_map_kf_row* rows);
/* The tracker's per-frame iteration set (src/Tracker.cc:987-998) into the counts: per entry outlier_count[point]++ where the
 * flag is set, else inlier_count[point]++ (integer atomic adds: exact in any order; a point may be named more than once).
 * points, outlier_flags: host, checked there.  Moves n * 5 bytes up. */
int ptam_rmap_note_tracked(ptam_rmap*, int n, const int32_t* points, const uint8_t* outlier_flags);
/* ptam_map_scene_depth on the resident tables.  out: n_kf rows, host.  Moves n_kf * sizeof(ptam_scene_depth) down. */
int ptam_rmap_scene_depth(ptam_rmap*, ptam_scene_depth* out);
/* MapMaker::ClosestKeyFrame / NClosestKeyFrames (src/MapMaker.cc:711-752) on the resident pose table: the n_out = min(n, n_kf - 1)
 * keyframes other than `kf` that come first by (KeyFrameLinearDist(kf, k), k), ascending — a strictly lower distance wins, equal
 * distances go to the lower index.  One one-workgroup kernel, in the arithmetic ptam_rmap_bundle_adjust(RECENT) chooses its four
 * nearest with (camera centres of se3CfromW^-1 in uncontracted fp64, sqrt).  out_kf, out_dist: room for min(n, n_kf - 1) entries.
 * PTAM_E_ARG: kf outside [0, n_kf), n < 1.  Moves 8 + 12 n_out bytes down and nothing else. */
int ptam_rmap_closest_keyframes(ptam_rmap*, int kf, int n, int32_t* out_kf, double* out_dist, int32_t* n_out);

/* MapMaker::AddKeyFrameFromTopOfQueue (src/MapMaker.cc:493-518) after MakeKeyFrame_Rest, as ONE call on the resident map. */
typedef struct {
    ptam_epipolar_opts epipolar;        /* levels {3,0,1,2}, the new keyframe's depth_mean/sigma, wiggle, threshold */
    ptam_map_refind_opts refind;        /* as ptam_rmap_refind */
    int32_t target_kf;                  /* -1: ClosestKeyFrame of the new keyframe */
    int32_t skip_refind, skip_points;   /* 0 / 0 is the reference */
} ptam_rmap_insert_opts;
typedef struct {
    int32_t kf;                         /* the new keyframe's index */
    int32_t target_kf;                  /* -1 with skip_points */
    double target_dist;                 /* KeyFrameLinearDist(kf, target_kf) */
    ptam_map_refind_result refind;
    int32_t first_point, n_made;        /* the new points are [first_point, first_point + n_made) */
    ptam_epipolar_level_stats levels[4];
} ptam_rmap_insert_result;
/* The steps, each enqueued behind the one it depends on:
 *   (a) ptam_rmap_add_keyframe's table step (:501-506);
 *   (b) ptam_rmap_refind(KEYFRAME) of the new keyframe through `finder` (:508): the merged tables become the map's;
 *   (c) target_kf < 0: the closest keyframe (AddSomeMapPoints' ClosestKeyFrame, :451), by ptam_rmap_closest_keyframes' kernel
 *       (it reads the poses alone and is enqueued with (a)); target_kf >= 0: the same kernel measures that keyframe's distance;
 *   (d) a kernel writes the busy list of ThinCandidates (:415-441) from the new keyframe's run in the resident measurement
 *       table as (b) left it — the run of the highest keyframe index is the table's tail;
 *   (e) the launch chain of ptam_add_map_points_epipolar (:511-514), the target's pose taken from the handle's mirror and its
 *       implane tables built on its handle (as ptam_add_map_points_epipolar does on the target it is given);
 *   (f) the made count and the level stats come down in one wait;
 *   (g) ptam_rmap_add_points' kernels on the chain's device output, target_source = PTAM_MAP_SRC_EPIPOLAR, the new points'
 *       indices to the end of new_queue.
 * The ptam_new_map_point records never leave the device: the tracker's rows are
 * ptam_rmap_download(PTAM_RMAP_REFIND_POINTS, first_point, n_made).  skip_refind / skip_points leave out (b) / (c)-(g).
 * Everything that can refuse the call is decided on the host before anything is enqueued, and a refused call leaves every table
 * and count as it was.  PTAM_E_ARG: rows unsorted, repeated or out of range; kf null, or (unless both steps are skipped) a
 * keyframe of the map without a handle; target_kf outside [-1, n_kf) (the new keyframe's own index n_kf included); the level list
 * as ptam_add_map_points_epipolar.  PTAM_E_STATE, unless skip_points: kf has no MakeKeyFrame_Rest; the map has no keyframe
 * (where the reference's assert(nClosest != -1) stands).
 * Moves 97 + 24 n_rows bytes, the re-find's level records (at most PTAM_RMAP_KF_RECORD_BYTES per keyframe) up; 20 bytes for (c),
 * the re-find's 16 bytes of counts and 16 + 4 sizeof(ptam_epipolar_level_stats) bytes for (f) down.  Nothing proportional to the
 * candidates, the made points or the measurement table moves. */
int ptam_rmap_insert_keyframe(ptam_rmap*, ptam_refinder*, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows,
                              const ptam_map_kf_row* rows, const ptam_rmap_insert_opts*, ptam_rmap_insert_result*);

/* ---- The first map, made in the resident map: MapMaker::InitFromStereo (src/MapMaker.cc:268-405) as ONE call ----------------------
 *      first / second: the caller's clones of the two keyframes (*pkFirst = kF, :299-302); the map keeps them as the handles of
 *      keyframes 0 and 1, and the call runs ptam_make_keyframe_rest on whichever lacks it (:371-372).  trails != NULL: the live
 *      list is read where it lies on the device, n_matches / matches are ignored.  trails == NULL: matches (host, n_matches rows of
 *      16 bytes) is the reference's vTrailMatches.
 *      The stages, each enqueued on the handle's context behind the one before it:
 *        (1) :272-287  the match table and HomographyInit::Compute: the kernels of ptam_trails_homography.  Not OK: NO_HOMOGRAPHY.
 *        (2) :290-297  on the host: the baseline test (ZERO_BASELINE), t *= wiggle_scale / |t|.
 *        (3) :299-367  the point loop (the kernel of ptam_init_points_from_trails) on the device list; the made records compacted in
 *                      match order on the device (tile counts, scan, scatter: no atomic decides a place) and added with
 *                      src_kf = 0, target_kf = 1, PTAM_MAP_SRC_TRAIL as ptam_rmap_add_points adds them.  Fewer than 3: TOO_FEW_POINTS.
 *        (4) :374-375  first_bundles x (ptam_rmap_bundle_adjust(ALL), ptam_rmap_apply_outliers).
 *        (5) :378-380  ptam_rmap_scene_depth; keyframe 1's mean and sigma become the epipolar options' depth.
 *        (6) :382-385  steps (d)-(g) of ptam_rmap_insert_keyframe for kSrc = keyframe 1 (its run is the table's tail), kTarget = 0.
 *        (7) :387-394  stage (4)'s step until the bundle reports convergence; *stop_flag (nullable) is the bundle's abort flag and is
 *                      read after each bundle: STOPPED.  max_bundles > 0: STOPPED when that many bundles of this loop have not converged.
 *        (8) :397      ptam_rmap_align_to_plane.
 *      TRANSACTION.  The call replaces the whole map as ptam_rmap_upload does (new serials, a new keyframe epoch, first / second the
 *      only handles).  NO_HOMOGRAPHY, ZERO_BASELINE, TOO_FEW_POINTS and every PTAM_E_ARG / PTAM_E_STATE refusal leave the previous
 *      map exactly as it was: stages (1)-(3) work in the context's scratch until stage (3)'s count is known.  STOPPED leaves the
 *      handle empty (the reference's Reset() after `return false`).  The outcomes are result->status; the return value is PTAM_OK.
 *      REFUSALS, decided before anything is enqueued, the result struct untouched.  PTAM_E_ARG: a null handle, keyframe, options or
 *      result; trails of another context or image size than the map's; keyframes of another device or size; fewer than 4 matches
 *      (or trails == NULL with matches == NULL); the option refusals of ptam_trails_homography, ptam_add_map_points_epipolar's level
 *      list and ptam_calc_plane_aligner; wiggle_scale <= 0, subpix_max_its < 1, first_bundles < 0, max_bundles < 0; plane.samples
 *      (the point count is not known to the caller: a seed is).  PTAM_E_STATE: trails not started.
 *      HOST WAITS and the decision each serves: (1) stage 1's result — NO_HOMOGRAPHY, the baseline, the scaling; (2) stage 3's
 *      counts — TOO_FEW_POINTS, the rows to make room for; (3) the add's wait, after which the counts move; (4) per bundle, the
 *      selection's and Compute()'s waits of ptam_rmap_bundle_adjust and, with outliers, the wait of ptam_rmap_apply_outliers —
 *      converged, the outlier list, the stop flag; (5) the two depth rows — the epipolar depth range; (6) the epipolar header — the
 *      made count, then the add's wait; (7) the plane record and the poses — the status, the tracker's pose.
 *      ptam_rmap_traffic counts, for the call: up, 16 n_matches with trails == NULL, 16 x trials for stage 1's samples (n_matches >= 10),
 *      192 + 2 for the two poses and flags, per bundle 2 x 97 and 16 per outlier, the plane call's bytes (below); down, 256 for stage 1's
 *      result, PTAM_RMAP_WORD_BYTES for stage 3's counts, per bundle 32 + 4 x 2, 192 when accepted, 16 per outlier and, with outliers,
 *      PTAM_RMAP_WORD_BYTES, 2 sizeof(ptam_scene_depth), 16 + 4 sizeof(ptam_epipolar_level_stats), the plane call's bytes.  With
 *      trails != NULL nothing proportional to the matches, the points or the measurement table crosses in either direction. */
enum { PTAM_INIT_MAP_OK = 0, PTAM_INIT_MAP_NO_HOMOGRAPHY = 1, PTAM_INIT_MAP_ZERO_BASELINE = 2, PTAM_INIT_MAP_TOO_FEW_POINTS = 3,
       PTAM_INIT_MAP_STOPPED = 4 };
typedef struct {
    ptam_homography_opts homography;    /* 5.0 / 300 / seed or samples */
    double wiggle_scale;                /* MapMaker.WiggleScale, 0.1 (:34) */
    int32_t subpix_max_its;             /* 10 (:333) */
    int32_t first_bundles;              /* 5 (:374) */
    int32_t max_bundles;                /* 0: the reference's unbounded while (:390-394) */
    int32_t pad_;
    ptam_ba_opts ba;
    ptam_epipolar_opts epipolar;        /* levels {0,3,1,2} (:382-385); depth_mean / depth_sigma are ignored (stage 5 gives them) */
    ptam_plane_opts plane;
} ptam_rmap_init_opts;
typedef struct {
    int32_t status;                     /* PTAM_INIT_MAP_* */
    int32_t n_matches;
    ptam_homography_info homography;
    double baseline;                    /* dTransMagn (:290) */
    int32_t n_made, n_subpix_failed, n_behind_camera, n_template_bad;   /* stage 3, by PTAM_INIT_* status */
    int32_t n_bundles, n_accepted, n_outliers, n_outlier_bundles;       /* over stages 4 and 7; the bundles that had outliers */
    int32_t converged, pad_;                                            /* the last bundle's flag */
    ptam_scene_depth depth[2];
    double wiggle_scale_depth_normalized;   /* mdWiggleScaleDepthNormalized (:380) */
    int32_t first_epipolar_point, n_epipolar;
    ptam_epipolar_level_stats levels[4];
    ptam_plane_info plane;
    double se3_aligner[12];
    double tracker_pose[12];            /* se3TrackerPose = pkSecond->se3CfromW (:400) */
    ptam_rmap_counts_t counts;          /* the map as the call leaves it */
} ptam_rmap_init_result;
/* PTAM_E_ARG: a null pointer */
int ptam_rmap_init_opts_default(ptam_rmap_init_opts*);
int ptam_rmap_init_from_stereo(ptam_rmap*, const ptam_kf* first, ptam_kf* second, ptam_trails* trails, int n_matches,
                               const ptam_trail* matches, const ptam_rmap_init_opts*, const volatile unsigned char* stop_flag,
                               ptam_rmap_init_result*);
/* ptam_map_align_to_plane on the resident tables (the re-anchoring of a running session, and stage 8 above): plane_score_kernel /
 * plane_finish_kernel on the resident points, the apply kernel reading the aligner from device memory.  The same kernels and bits
 * as ptam_map_align_to_plane, and every info->status with that call's meaning: OK, the poses go into the second buffer (and the
 * mirror) and the points move in place; TOO_FEW and DEGENERATE, poses and points stay.  In every case the point rows' pixel vectors
 * end as RefreshPixelVectors against the final poses leaves them (DEGENERATE: by a second launch that moves nothing).
 * out_rows (nullable, n_points ptam_pvs_point): the rows for ptam_tracker_set_map.  opts->samples as ptam_calc_plane_aligner.
 * An empty map: PTAM_PLANE_TOO_FEW, the identity, nothing enqueued.
 * Moves 12 x trials bytes up (n_points >= 10) and 256 more when DEGENERATE; 256 (the info and the aligner), 96 n_kf and out_rows down. */
int ptam_rmap_align_to_plane(ptam_rmap*, const ptam_plane_opts*, double se3_aligner[12], ptam_plane_info*, ptam_pvs_point* out_rows);
/* MapMaker::Reset (src/MapMaker.cc:37-43) for the tables: all counts 0, no keyframe handles, a new keyframe epoch.  The capacities,
 * the serial counter and the traffic sums stay.  Moves nothing. */
int ptam_rmap_clear(ptam_rmap*);

/* ---- The resident map published to the tracker on the device --------------------------------------------------------------------
 *      Replaces the one table-sized trip left between the two threads: ptam_rmap_download of the point rows and `kept`, the host
 *      loop that composes prev_index, ptam_tracker_update_map's upload.
 *      POINT SERIALS.  A ptam_rmap keeps a seventh point-side column: one 64-bit serial per point, given by the library from the
 *      handle's running counter (starting at 1) and never reused within the handle.  ptam_rmap_upload gives every point a fresh
 *      one (a re-uploaded map is a new map to every tracker), ptam_rmap_add_points and ptam_rmap_insert_keyframe append the next
 *      ones behind the count, ptam_rmap_handle_bad_points compacts the column with the others, growth copies it.  Points are only
 *      appended at the end and removed by an order-preserving compaction, so the column is strictly increasing with the point index
 *      without any sort.  It follows the two-buffer rules of its neighbours: a refused call leaves it as it was.  It is no table
 *      of ptam_rmap_download and costs no existing call a byte over the host link.  Every handle also has a process-wide map_id,
 *      given at ptam_rmap_create: (map_id, serial) names a point for as long as the handle lives.
 *      SNAPSHOT.  A ptam_map_snapshot holds, in device memory, what the tracker needs of one state of the map: n, the map_id, a
 *      generation number, the ptam_pvs_point rows, the patch sources resolved to level images, and the serials.  It has three
 *      slots: the current generation, the one a publish is writing, one a take may still be copying.  The hand-over is host-side:
 *      a publish completes on the mapmaker's queue (its one wait) before the generation becomes current under the snapshot's
 *      mutex; a take picks the current slot under the same mutex and enqueues on the tracker's queue afterwards.  No kernel waits
 *      for another queue and no flag is spun on in device memory; a take never sees a half-written generation, a publish never
 *      overwrites one a take is copying, and neither thread waits for the other's device work (with more than one tracker taking
 *      from one snapshot, a publish may wait for one take's copy).  One thread publishes into a snapshot; any number take.
 *      The keyframes of the map must outlive every snapshot generation and tracker that names their images. */
typedef struct ptam_map_snapshot ptam_map_snapshot;
typedef struct {
    int64_t generation;                 /* of this publish: 1, 2, ... per snapshot */
    int64_t map_id;
    int32_t n_points, n_kf;
    int32_t grew, pad_;                 /* the slot was too small and was reallocated (the call's only allocation) */
} ptam_map_publish_result;
typedef struct {
    int32_t changed;                    /* 0: the tracker holds this generation already; nothing else was done */
    int32_t n_points;
    int32_t n_carried, n_new, n_dropped;   /* points that kept their PatchFinder | new to the tracker | old points without successor */
    int32_t link_bytes;                 /* what crossed the host link in this call */
    int64_t generation, map_id;
} ptam_map_take_result;
typedef struct { int64_t generation, map_id; int32_t n_points, pad_; } ptam_map_snapshot_info_t;
/* max_points: the capacity of all three slots.  The snapshot remembers the context's device and frame size, not the context. */
int ptam_map_snapshot_create(ptam_ctx*, int max_points, ptam_map_snapshot** out);
int ptam_map_snapshot_destroy(ptam_map_snapshot*);
/* at least max_points in every slot that is neither current nor being copied (those grow when they are next written); the
 * publisher's thread.  Never shrinks. */
int ptam_map_snapshot_reserve(ptam_map_snapshot*, int max_points);
/* the current generation (0: never published into), its map and point count; any thread */
int ptam_map_snapshot_info(ptam_map_snapshot*, ptam_map_snapshot_info_t* out);

/* The map as it stands into the snapshot's free slot; the mapmaker's thread, synchronous.  One gather kernel, one thread per point,
 * reads refind_points[i].pv, src_kf, src_level, center_x / y and the serial, and resolves src_kf through a per-keyframe record of
 * the four level image addresses and sizes, which goes up with the call (64 bytes a keyframe, well under
 * PTAM_RMAP_KF_RECORD_BYTES, counted in ptam_rmap_traffic).  Every point of the table is published, bad ones included (the
 * reference's tracker walks vpPoints until HandleBadPoints has trashed a point).  After the call's one wait the slot becomes the
 * current generation.  A slot that is too small is reallocated at double its size: the call's only allocation, which
 * ptam_map_snapshot_reserve avoids.
 * PTAM_E_ARG, decided before anything is enqueued, the snapshot keeping its generation: a keyframe of the map without a handle (or
 * with one of another device), a snapshot on another device than the map's.  PTAM_E_STATE: a publish into this snapshot is under way.
 * Moves 64 n_kf bytes up and nothing down: nothing proportional to the points.
 * Into a snapshot with a keyframe section (ptam_snapshot_keyframes_enable, below) the same call also publishes the keyframes'
 * poses and SmallBlurryImages, with the further refusals and the 8 bytes per made image listed there. */
int ptam_rmap_publish(ptam_rmap*, ptam_map_snapshot*, ptam_map_publish_result* res);
/* rows [first, first + count) of the serial column.  PTAM_E_ARG: a range outside the points.  Moves 8 count bytes down. */
int ptam_rmap_point_serials(ptam_rmap*, int first, int count, int64_t* out);
/* The current point index of each serial, by a binary-search kernel in the resident serial column, one thread per entry: -1 for
 * a point that has been removed (or a value never given out); *n_gone (nullable) counts those.  No order rule on the input.
 * Serial order is index order: a host that sorts a keyframe's found entries by serial has the rows of ptam_rmap_insert_keyframe
 * sorted by point.  This is how the tracker's iteration set (ptam_tracker_read_iteration_serials) reaches ptam_rmap_note_tracked
 * and ptam_rmap_insert_keyframe after ptam_rmap_handle_bad_points has renumbered the map.
 * Moves 8 n bytes up, 4 n + PTAM_RMAP_WORD_BYTES down. */
int ptam_rmap_resolve_serials(ptam_rmap*, int n, const int64_t* serials, int32_t* index_out, int32_t* n_gone);

/* ptam_tracker_update_map from the snapshot's current generation, everything table-sized staying on the device; the tracker's
 * thread, synchronous.  If the snapshot's generation is the one this tracker took last: changed = 0, no launch, no copy, one mutex
 * hold — the per-frame poll.  Otherwise the point rows and the sources are copied device to device; a kernel computes prev[i],
 * one thread per new point, by a binary search of the new serial in the tracker's serial list of its current map (-1 when it is
 * not there, or when the map_id differs: both lists are strictly increasing, so no old index is hit twice); the finder-carry
 * kernel of ptam_tracker_update_map runs on that prev; a kernel writes the identity shuffles when n changed; the tracker's
 * serial list becomes the snapshot's.  The same input gives the same bits, and the tracker's next frame is the one
 * ptam_tracker_update_map with the composed prev_index gives.
 * PTAM_E_ARG, with the tracker's map untouched: n above the tracker's max_points, a snapshot on another device, a snapshot of
 * another frame size than the tracker's context's, a snapshot never published into.
 * Moves 8 bytes down (the carried count) and nothing up: at most 64 bytes cross the host link. */
int ptam_tracker_take_map(ptam_tracker*, ptam_map_snapshot*, ptam_map_take_result* res);
/* rows [first, first + count) of the tracker's serial list: the serials of its map's points after a take, empty after
 * ptam_tracker_set_map / ptam_tracker_update_map (which clear it: the next take treats every point as new).
 * PTAM_E_ARG: a range outside the list. */
int ptam_tracker_point_serials(ptam_tracker*, int first, int count, int64_t* out);
/* the serial of every entry of the iteration set, in the order of ptam_tracker_read_iteration_set (a gather kernel): what
 * ptam_rmap_resolve_serials turns into the map's numbering of the moment.  out (nullable: *n alone), cap as there.
 * PTAM_E_STATE: the tracker's map did not come from a snapshot. */
int ptam_tracker_read_iteration_serials(ptam_tracker*, int64_t* out, int cap, int* n);

/* ---- The map's keyframes published to the relocaliser on the device ---------------------------------------------------------------
 *      The reference's relocaliser and IsNeedNewKeyFrame read Map::vpKeyFrames directly (src/Relocaliser.cc:12-38,
 *      src/MapMaker.cc:736-763): every keyframe's pSBI (src/KeyFrame.cc:80-81) and se3CfromW.  Here the tracker's thread keeps them
 *      in a ptam_sbi_bank; with a keyframe section in the snapshot the bank follows the resident map without the host carrying a
 *      keyframe handle or a pose table between the threads.
 *      KEYFRAME IDENTITY.  A ptam_rmap only appends keyframes (add_keyframe, insert_keyframe, insert_keyframe_report) or replaces
 *      them all (ptam_rmap_upload).  The handle counts its successful uploads (the keyframe epoch): (map_id, epoch) and an index
 *      name a keyframe, and a keyframe's SmallBlurryImage never changes.
 *      TWO TAKES.  ptam_tracker_take_map and ptam_sbi_bank_take_keyframes are separate calls (batched trackers keep one bank per
 *      camera), each against its own (snapshot, generation).  A publish can land between the two: each side is then whole in
 *      itself, of one generation, and the next frame's poll brings the other one up. */
typedef struct {
    int64_t generation;                 /* the snapshot's current generation (0: never published into) */
    int64_t map_id, epoch;              /* of the keyframes it holds (0: none, or published before the section was enabled) */
    int32_t enabled, max_keyframes;
    int32_t n_kf, n_made;               /* keyframes in the current generation | SmallBlurryImages its publish had to make */
    int32_t sbi_w, sbi_h;               /* mirSize for the snapshot's frame size */
    double blur;
} ptam_snapshot_keyframes_info_t;
typedef struct {
    int32_t changed;                    /* 0: the bank holds this generation already; nothing else was done */
    int32_t n_kf;                       /* the bank's count after the call */
    int32_t n_new;                      /* SmallBlurryImages copied into the bank */
    int32_t link_bytes;                 /* what crossed the host link in this call: 96 n_kf, or 0 */
    int64_t generation, map_id;
} ptam_keyframes_take_result;
/* Room for max_keyframes keyframes in every slot: se3CfromW (12 doubles) and a SmallBlurryImage in the ptam_sbi_bank's layout,
 * 13 bytes a pixel (about 15.6 kB per keyframe and slot at 640x480); blur: 2.5, the keyframes' (include/ImageProcess.h:57-58).
 * The publisher's thread, before the threads start or between two publishes; generations published before it hold no keyframes.
 * PTAM_E_ARG: max_keyframes < 1 (or above 65535), a blur outside (0, 5].  PTAM_E_LIMIT: a frame size whose SmallBlurryImage is
 * above the library's limit.  PTAM_E_STATE: enabled already, or a publish is under way.
 * ptam_rmap_publish into an enabled snapshot then also, in the same slot, on the same queue, before its one wait and its commit:
 *   (a) copies the resident pose table [0, n_kf) into the slot, device to device;
 *   (b) makes the SmallBlurryImage (src/KeyFrame.cc:80-81) of every keyframe the slot does not hold yet — [slot's count, n_kf) when
 *       the slot last held keyframes of the same (map_id, epoch), else [0, n_kf) — with ONE make launch, grid x = their number, the
 *       kernel of ptam_sbi_bank_add_batch: with three slots a keyframe's image is made at most three times in its life;
 * so the points and the keyframes of a generation belong together.  Further refusals, decided before a slot is taken, the snapshot
 * keeping its generation: PTAM_E_LIMIT, n_kf > max_keyframes; PTAM_E_ARG, a keyframe of another frame size than the snapshot's.
 * Moves 8 bytes up per image made (its level-3 address; counted in ptam_rmap_traffic) and nothing down. */
int ptam_snapshot_keyframes_enable(ptam_map_snapshot*, int max_keyframes, double blur /* 2.5 */);
/* any thread */
int ptam_snapshot_keyframes_info(ptam_map_snapshot*, ptam_snapshot_keyframes_info_t* out);
/* Map::vpKeyFrames as Relocaliser::AttemptRecovery (src/Relocaliser.cc:12-38) and MapMaker::ClosestKeyFrame (src/MapMaker.cc:
 * 736-763) read it, from the snapshot's current generation into the bank; the tracker's thread, synchronous, one wait.  If the
 * generation is the one this bank took last: changed = 0, no launch, no copy — the per-frame poll.  Otherwise ONE copy launch moves
 * the poses [0, n_kf) into the bank's device table and the SmallBlurryImages the bank lacks into its entries — [count, n_kf) when
 * the bank's entries are keyframes of the same snapshot, map_id and epoch and count <= n_kf, else [0, n_kf) — and the poses come down
 * once into the bank's host mirror (what ptam_sbi_bank_poses and the closest-keyframe walk of ptam_track_frames_recover_batch
 * read), behind any pending copy from that mirror; then count = n_kf.
 * PTAM_E_STATE: the keyframe section is not enabled.  PTAM_E_ARG: a snapshot on another device, of another frame size, or never
 * published into (since the section was enabled); a bank that holds entries added by hand with another blur than the snapshot's —
 * the bank is the only record of a blur on the tracker's side (ptam_relocalise and ptam_track_frames_recover_batch take theirs per
 * call), so entries of blur x mean the bank is used with x.  PTAM_E_LIMIT: n_kf above the bank's capacity.  In every refusal the
 * bank, its mirror and what it remembers of its last take are as they were.
 * After a take ptam_sbi_bank_add / _add_batch are refused (PTAM_E_STATE) until ptam_sbi_bank_clear; ptam_sbi_bank_set_poses stays
 * allowed, and the next changed take overwrites what it set.
 * Moves 96 n_kf bytes down and nothing up. */
int ptam_sbi_bank_take_keyframes(ptam_sbi_bank*, ptam_map_snapshot*, ptam_keyframes_take_result* res);
/* Tracker::Reset / a new map (src/Tracker.cc:49-76; MapMaker::Reset, src/MapMaker.cc:37-43, clears Map::vpKeyFrames): count = 0, and where the entries came from is forgotten: both
 * ptam_sbi_bank_add and a take work again, a take copying every entry. */
int ptam_sbi_bank_clear(ptam_sbi_bank*);
/* entry `index` as ptam_sbi_read gives a single image (mimSmall, mimTemplate, mimImageJacs of Map::vpKeyFrames[index]->pSBI);
 * NULL pointers are skipped.  PTAM_E_ARG: an index outside [0, count). */
int ptam_sbi_bank_read(ptam_sbi_bank*, int index, uint8_t* small, float* tmpl, float* jacs);

/* ---- A tracked frame handed to the resident map on the device ----------------------------------------------------------------------
 *      The opposite direction of the snapshot.  The reference's tracker writes into the map on every frame: CalcPoseUpdate bumps
 *      nMEstimatorOutlierCount / nMEstimatorInlierCount of every found point (src/Tracker.cc:989-997), TrackMap turns vIterationSet
 *      into mCurrentKF.mMeasurements (:667-676), AddKeyFrameFromTopOfQueue stamps those into the map (src/MapMaker.cc:501-506).
 *      A ptam_frame_report holds, in device memory, the FOUND entries of one iteration set as 32-byte records sorted by point serial
 *      (strictly increasing: a point makes at most one record; if the set named a point twice, the later entry would stand, as
 *      mMeasurements[&p] = m does).  Serial order is the tracker's point-index order and the map's, because both serial columns
 *      increase strictly with the index: nothing is sorted, and no atomic decides where a record lands — the same frame gives the
 *      same bytes.  The host keeps the report's info: the map_id the serials belong to, the caller's tag, the counts.
 *      THREADING.  A report is complete on the device when the call that fills it returns; whoever holds it then may read it, on any
 *      queue of its device.  The library keeps no lock on a report and no kernel waits for another queue: handing a report from the
 *      tracker's thread to the mapmaker's (a queue, a pool) is the caller's, as mvpKeyFrameQueue is the reference's.  Refilling or
 *      destroying a report that another thread is consuming is the caller's error. */
typedef struct ptam_frame_report ptam_frame_report;
typedef struct {
    int64_t serial;             /* of the point, in the map `map_id` */
    int32_t level;              /* nSearchLevel */
    uint8_t outlier, did_subpix, pad_[2];   /* 0 / 1, as ptam_trackmap_meas::outlier and ::did_subpix */
    double root_pos[2];         /* v2_found */
} ptam_frame_record;
typedef struct {
    int64_t map_id;             /* 0: an empty report (never filled, or too small for its frame) */
    int64_t tag;                /* the caller's, e.g. the frame number */
    int32_t n_records;          /* found points */
    int32_t n_entries;          /* the iteration set's length */
    int32_t n_outliers;         /* records with outlier != 0 */
    int32_t pad_;
} ptam_frame_report_info_t;
/* max_records >= 1: the report's capacity, device memory of 32 max_records bytes; a fill also keeps one word per point of the
 * frame's map on the report (grown on demand: the one allocation a fill may make). */
int ptam_frame_report_create(ptam_ctx*, int max_records, ptam_frame_report** out);
int ptam_frame_report_destroy(ptam_frame_report*);
/* host only: moves nothing */
int ptam_frame_report_info(const ptam_frame_report*, ptam_frame_report_info_t* out);
/* records [first, first + count) down, for tests, drawing and hosts that keep MapPoint objects.  PTAM_E_ARG: a range outside
 * [0, n_records).  Moves 32 count bytes down. */
int ptam_frame_report_read(ptam_frame_report*, int first, int count, ptam_frame_record* out);
/* The frames the trackers tracked last into the reports, nb >= 1 cameras in ONE launch (a workgroup per camera) and one wait, on
 * the queue that last ran trackers[0] (a tracker that last ran on another queue is waited for on the host first: its frame has
 * been delivered, so that wait finds the queue idle).  The kernel reads the tracker's own buffers — search slots, found flags,
 * levels, positions, the outlier flags in whichever of the two layouts the frame's pose loop left them (at the slots, or at the
 * compacted measurements) — and the tracker's serial list; the set's length is read on the device.  tags (nullable): nb values.
 * PTAM_E_STATE: a tracker whose map did not come from a snapshot (ptam_tracker_take_map).  PTAM_E_ARG: a null handle, a report on
 * another device than its tracker, a report or a tracker named twice.  All of these are decided before anything is enqueued and
 * leave every report as it was.  A report too small for its frame's found points is known only after the wait: that report comes
 * back empty (n_records = 0, map_id = 0), the others are filled, and the call returns PTAM_E_ARG.
 * Moves 144 bytes per camera up (where its buffers lie) and 16 bytes per camera down; no record crosses the host link. */
int ptam_tracker_report_frames(int nb, ptam_tracker* const* trackers, ptam_frame_report* const* reports, const int64_t* tags);
/* The same device core on arrays the host supplies, for a host whose tracker is not a ptam_tracker: point_serials (n_points,
 * strictly increasing) is the serial list of the tracker's map, entries (n_entries) an iteration set in that tracker's point
 * numbering.  tag becomes 0.  PTAM_E_ARG, the report as it was: map_id == 0, serials not strictly increasing, a found entry whose
 * point is outside [0, n_points) or whose level is outside 0..3; after the wait, the report empty: more found points than
 * max_records.  Moves 8 n_points + 40 n_entries + 144 bytes up, 16 down. */
int ptam_frame_report_from_host(ptam_frame_report*, int64_t map_id, int n_points, const int64_t* point_serials, int n_entries,
                                const ptam_trackmap_meas* entries);

/* ptam_track_frames_recover_batch with the frames' reports filled INSIDE the chain and, optionally, the frames' two random orders
 * drawn there: one call and one host wait per camera where the sequence set_shuffle / recover_batch / report_frames has two calls
 * with a launch and a queue wait behind the frame's.  The first twelve arguments are ptam_track_frames_recover_batch's and mean the
 * same; results, states, infos and iteration sets are that call's bit for bit (the same kernels on the same data), the reports'
 * records and infos those of ptam_tracker_report_frames called behind it.
 *   reports        nullable, as is every entry: camera i's frame goes into reports[i].  The fill (one workgroup per report, the
 *                  kernel body of ptam_tracker_report_frames) is one more launch behind the fine pose loops on the chain's queue; its
 *                  jobs ride in the batch's one argument upload (184 bytes a report), and its head words land in the frame's
 *                  host-mapped result block under the frame's sequence number: the host waits for them as it waits for the frame.
 *   tags           nullable: reports[i]'s tag (0 without).
 *   shuffle_seeds  nullable: the caller has set the shuffles (on a map of more than 8192 points ptam_tracker_set_shuffle uploads them
 *                  asynchronously from the context's pinned staging block, which a batch call fills next: wait for the tracker's
 *                  queue between the two).  Otherwise EVERY camera's two orders are drawn in front of the set
 *                  choice exactly as ptam_tracker_draw_shuffles(trackers[i], shuffle_seeds[i], states[i].frame) would, states[i].frame
 *                  as it is at entry — one launch for all maps of at most 8192 points, the larger ones one by one.
 *   report_info    nullable: per camera the report's info as ptam_frame_report_info gives it (zero without a report) and
 *                  report_in_chain.
 * What happens to a report:
 *   PTAM_FRAME_RECOVERY_FAILED   the frame tracked nothing: the report comes back EMPTY (map_id 0, n_records 0, tag 0).  The fill
 *                                workgroup reads the relocaliser's verdict as the TrackMap kernels do and does not look at the
 *                                tracker's control block, which still holds the frame before.
 *   a frame on the long path     its fine pose loop outgrew the fused kernel and is finished by launches the host enqueues on the
 *                                frame's own queue behind the wait: the report cannot be in the chain.  It is filled behind those
 *                                passes by ptam_tracker_report_frames itself, with a second wait; report_in_chain is 0.
 *   a report too small           for its frame's found points: every frame is delivered and every state moves, THAT report comes
 *                                back empty with report_too_small set, the call returns PTAM_E_ARG (as ptam_tracker_report_frames).
 *                                A refused call writes no report_info: a caller that zeroes it first tells the two PTAM_E_ARG apart
 *                                by that flag.
 * Refused before the first enqueue with everything where it was, beyond ptam_track_frames_recover_batch's own refusals:
 * PTAM_E_STATE a camera with a report whose tracker's map did not come from ptam_tracker_take_map; PTAM_E_ARG a report on another
 * device, a report named twice.  As there, states and estimators advance on copies and commit when every frame has arrived.
 * A failure BEHIND the first enqueue (PTAM_E_HIP, a wait that times out) leaves states and estimators where they were too, but not
 * everything: every report of the call comes back empty (its records may be half rewritten), and with seeds the trackers' orders
 * are the drawn ones. */
typedef struct {
    ptam_frame_report_info_t report;
    int32_t report_in_chain;    /* 1: filled at the chain's end; 0: no report, or filled behind the long path's passes */
    int32_t report_too_small;   /* 1: the report could not hold the frame's found points and is empty (the call returns PTAM_E_ARG) */
} ptam_track_report_info;
int ptam_track_frames_report_batch(int nb, ptam_tracker* const* trackers, ptam_kf* const* current, const uint8_t* const* d_frames,
                                   ptam_track_state* states, ptam_rotation_estimator* const* estimators, ptam_sbi_bank* const* banks,
                                   ptam_sbi* const* scratch, const ptam_trackmap_opts* opts, const ptam_track_state_opts* state_opts,
                                   ptam_trackmap_result* out, ptam_track_frame_state_info* info, ptam_frame_report* const* reports,
                                   const int64_t* tags, const uint64_t* shuffle_seeds, ptam_track_report_info* report_info);

/* The consumers, on the mapmaker's thread.  Both refuse, on the host with every table as it was (PTAM_E_ARG): a null or empty
 * report (n_records == 0), a report whose map_id is not this handle's, a report on another device. */
typedef struct { int32_t n_records, n_gone; } ptam_rmap_note_result;
/* ptam_rmap_note_tracked for n >= 1 reports in one launch (a row of workgroups per report): every record's serial is looked up in
 * the resident serial column (the binary search of ptam_rmap_resolve_serials); a live point gets outlier_count++ or inlier_count++
 * (integer atomic adds: exact in any order), a point that ptam_rmap_handle_bad_points has removed since the frame is counted in
 * n_gone.  The same report may be named more than once (it then counts more than once).  res->n_records: the records of all reports.
 * Moves 16 bytes per report up (where its records lie, how many) and PTAM_RMAP_WORD_BYTES down. */
int ptam_rmap_note_reports(ptam_rmap*, int n, ptam_frame_report* const* reports, ptam_rmap_note_result* res);
/* ptam_rmap_insert_keyframe with step (a) fed from the report: one one-workgroup kernel resolves every record's serial and
 * appends the live ones, in order, behind the measurement table's count as {n_kf, point, level, PTAM_MAP_SRC_TRACKER, root_pos}
 * — sorted by point and unique by construction, so there is nothing to check.  Room is made for report.n_records rows, the
 * host-known upper bound; the live count comes down in a wait of its own (PTAM_RMAP_WORD_BYTES) before the counts move and steps
 * (b)-(g) run, which are ptam_rmap_insert_keyframe's own code.  *n_rows (nullable): the rows appended; *n_gone (nullable):
 * n_records - *n_rows.  Refusals as ptam_rmap_insert_keyframe (the row checks apart) and as above.  A record's level is inside
 * 0..3: a found slot has been searched at a level, and ptam_frame_report_from_host refuses any other.
 * Moves 97 bytes and the re-find's level records up, PTAM_RMAP_WORD_BYTES more than ptam_rmap_insert_keyframe down: nothing
 * proportional to the rows. */
int ptam_rmap_insert_keyframe_report(ptam_rmap*, ptam_refinder*, const ptam_kf* kf, const double pose12[12], int fixed,
                                     ptam_frame_report* report, const ptam_rmap_insert_opts*, ptam_rmap_insert_result*, int32_t* n_rows,
                                     int32_t* n_gone);

/* ---- The mapmaker: one iteration of MapMaker::run() (src/MapMaker.cc:57-114) as ONE call on a resident map --------------------------
 *      A ptam_mapmaker wraps a ptam_rmap, the ptam_refinder its re-finds go through and, optionally, the ptam_map_snapshot it
 *      publishes into; it owns none of them (destroy it first).  It keeps what the reference's MapMaker keeps beside the map: the
 *      keyframe queue (mvpKeyFrameQueue), the flags mbBundleConverged_Recent / _Full, mbBundleRunning and mbBundleAbortRequested,
 *      the reset request, and the tracked frames' reports that wait to be counted.
 *      THREADS.  ptam_mapmaker_step, _flags, _set_flags and _destroy belong to the mapmaker's thread, the thread of the map's
 *      context.  ptam_mapmaker_add_keyframe, _note_frame, _queue_size, _request_reset, _reset_done, _released, _request_init and
 *      _init_poll may be called from the tracker's thread: they take the handle's mutex and touch no device.
 *      LIFETIMES.  A keyframe clone and a report handed over stay the caller's objects and must stay alive and unchanged until
 *      their tag comes back from ptam_mapmaker_released (a keyframe that has entered the map: as ptam_rmap_insert_keyframe_report
 *      says, for as long as the map names it).  Every tag handed over comes back exactly once: after the step that used it, or
 *      after the reset that dropped it.
 *      ptam_mapmaker_step runs the body of the loop once, in the reference's order, each condition asked when its stage is
 *      reached, with the queue as it stands then:
 *        CHECK_RESET (before every stage): a requested reset runs ptam_rmap_clear, empties the keyframe queue and the pending
 *          reports and releases their tags, sets the flags as Reset() does (:37-51: both converged, nothing running) and ends
 *          the step with status PTAM_MM_RESET.
 *        a map without a keyframe (:79) ends the step with status PTAM_MM_IDLE.
 *        :88   !converged_recent && queue == 0: BundleAdjustRecent = ptam_rmap_bundle_adjust_routed(RECENT) under the handle's
 *              abort byte.  With fewer than 8 keyframes it does not run and sets converged_recent (:790-793).  After Compute()
 *              (:895-913): accepted clears converged_recent and converged_full, converged sets converged_recent.
 *        :93   converged_recent && queue == 0: ReFindNewlyMade = ptam_rmap_refind_queue(NEW_POINTS), stopped by the byte that says
 *              the keyframe queue is not empty (:1053).
 *        :98   converged_recent && !converged_full && queue == 0: BundleAdjustAll = ptam_rmap_bundle_adjust_routed(ALL): accepted
 *              clears converged_full, converged sets both.
 *        :103  converged_recent && converged_full && draw && queue == 0: ReFindFromFailureQueue = ptam_rmap_refind_queue(
 *              FAILURE_QUEUE).  The draw is splitmix64(failure_seed, n) % failure_period == 0 for the n-th draw, in place of
 *              rand() % 20; as the reference's && does, a draw is made (and counted in `draws`) only when both flags are set.
 *        :107  the pending reports of ptam_mapmaker_note_frame, all in one ptam_rmap_note_reports launch; then HandleBadPoints =
 *              ptam_rmap_handle_bad_points.
 *        :111  queue > 0: AddKeyFrameFromTopOfQueue: the front leaves the queue, ptam_make_keyframe_rest runs on a keyframe that
 *              lacks it, ptam_rmap_insert_keyframe_report with the handle's insert options and the keyframe's depth; both
 *              converged flags are cleared (:516-517).
 *        with a snapshot: one ptam_rmap_publish at the end if a bundle was accepted, points were removed or a keyframe was inserted.
 *      AddKeyFrame (:480-488) raises the abort byte only while a bundle runs, decided under the mutex that the step holds when it
 *      sets and clears `bundle_running`.
 *      The result: status; `stages`, a mask of the PTAM_MM_STAGE_* that ran (a RECENT bundle that did not run for want of
 *      keyframes is not in it); each stage's own result struct, zero where it did not run; the flags, the queue size and the
 *      draw count afterwards.  A stage's error is the step's return value; the tags of what that stage consumed are released, and
 *      the result still says which stages had run and holds the flags, the queue size and the draw count as they stand.
 *      Moves what its stages move, and nothing else. */
typedef struct ptam_mapmaker ptam_mapmaker;
typedef struct {
    ptam_ba_opts ba;
    ptam_map_refind_opts refind;
    ptam_rmap_insert_opts insert;       /* epipolar.depth_mean / depth_sigma are the keyframe's own: ptam_mapmaker_add_keyframe */
    int32_t failure_period;             /* 20: rand() % 20 (:103) */
    uint64_t failure_seed;
} ptam_mapmaker_opts;
/* PTAM_MM_INIT, PTAM_MM_STAGE_INIT: the status and the stage bit of a step that made the first map (ptam_mapmaker_request_init) */
enum { PTAM_MM_RAN = 0, PTAM_MM_IDLE = 1, PTAM_MM_RESET = 2, PTAM_MM_INIT = 3 };
enum {
    PTAM_MM_STAGE_BUNDLE_RECENT = 1, PTAM_MM_STAGE_REFIND_NEW = 2, PTAM_MM_STAGE_BUNDLE_ALL = 4, PTAM_MM_STAGE_REFIND_FAILURE = 8,
    PTAM_MM_STAGE_NOTES = 16, PTAM_MM_STAGE_BAD_POINTS = 32, PTAM_MM_STAGE_ADD_KEYFRAME = 64, PTAM_MM_STAGE_PUBLISH = 128,
    PTAM_MM_STAGE_INIT = 256
};
/* what ptam_mapmaker_init_poll says of a request (0, 1, 2) */
enum { PTAM_MM_INIT_NONE, PTAM_MM_INIT_PENDING, PTAM_MM_INIT_DONE };
typedef struct {
    int32_t status, stages;
    ptam_map_ba_result recent;
    ptam_map_outliers_result recent_outliers;
    ptam_map_refind_result refind_new;
    ptam_map_ba_result all;
    ptam_map_outliers_result all_outliers;
    ptam_map_refind_result refind_failure;
    ptam_rmap_note_result notes;
    ptam_map_bad_points_result bad_points;
    ptam_rmap_insert_result insert;
    int32_t insert_rows, insert_gone;
    ptam_map_publish_result publish;
    int32_t converged_recent, converged_full, queue_size, pad_;
    uint64_t draws;
} ptam_mapmaker_step_result;
/* the reference's: ptam_ba_opts_default, max_pairs_per_pass 0, ptam_epipolar_opts_default with the levels {3,0,1,2} of :511-514,
 * target_kf -1, nothing skipped, failure_period 20, failure_seed 0.  PTAM_E_ARG: a null pointer. */
int ptam_mapmaker_opts_default(ptam_mapmaker_opts*);
/* snapshot, opts: nullable (no publish; the defaults).  The flags start as Reset() leaves them.  PTAM_E_ARG: a null map, finder
 * or out; failure_period < 1. */
int ptam_mapmaker_create(ptam_rmap*, ptam_refinder*, ptam_map_snapshot* snapshot, const ptam_mapmaker_opts* opts, ptam_mapmaker** out);
int ptam_mapmaker_destroy(ptam_mapmaker*);
/* MapMaker::AddKeyFrame (:480-488): the clone, its pose and flag, the tracker's report of the frame, the scene depth the
 * epipolar search of this keyframe uses, and the tag that names clone and report in ptam_mapmaker_released.  PTAM_E_ARG: a null
 * handle, clone, pose or report. */
int ptam_mapmaker_add_keyframe(ptam_mapmaker*, const ptam_kf* clone, const double pose12[12], int fixed, ptam_frame_report* report,
                               double depth_mean, double depth_sigma, int64_t tag);
/* a tracked frame's report, to be counted by the next step's ptam_rmap_note_reports */
int ptam_mapmaker_note_frame(ptam_mapmaker*, ptam_frame_report* report, int64_t tag);
int ptam_mapmaker_queue_size(ptam_mapmaker*, int32_t* out);
int ptam_mapmaker_request_reset(ptam_mapmaker*);   /* MapMaker::RequestReset (:116-120) */
int ptam_mapmaker_reset_done(ptam_mapmaker*, int32_t* out);   /* MapMaker::ResetDone */
/* MapMaker::InitFromStereo (src/MapMaker.cc:268-405) asked for by the tracker's thread (src/Tracker.cc:338-341).  The reference runs
 * it on the tracker's thread while run() idles (:79); here the resident map belongs to the mapmaker's context, so the tracker hands
 * over a REQUEST, as it hands over a keyframe: first / second (the caller's clones, under the lifetime rule of
 * ptam_rmap_init_from_stereo: the map names them until the next reset), a copy of the matches (the reference's vMatches, built on the
 * host at src/Tracker.cc:338-340; at most 16 bytes per trail), the options (nullable: ptam_rmap_init_opts_default) and a tag.
 * Callable from the tracker's thread: it takes the handle's mutex and touches no device.
 * The next ptam_mapmaker_step runs it in front of the :79 idle test, behind its first CHECK_RESET:
 *   ptam_rmap_init_from_stereo(map, first, second, NULL, n_matches, matches, opts, stop, &result), stop a byte that
 *   ptam_mapmaker_request_reset raises (mbResetRequested at :392).
 *   PTAM_INIT_MAP_OK: the flags are what the loop of :387-394 leaves (both converged, nothing running); with a snapshot the step
 *   publishes; the step ends with status PTAM_MM_INIT and PTAM_MM_STAGE_INIT (| PTAM_MM_STAGE_PUBLISH) in `stages`.
 *   Any other outcome: the map is as ptam_rmap_init_from_stereo leaves it (empty), the flags as Reset() leaves them (:45-50);
 *   PTAM_MM_STAGE_INIT is set and the step goes on to its idle test (PTAM_MM_IDLE), or to the reset that stopped it (PTAM_MM_RESET).
 *   The tag comes back through ptam_mapmaker_released after the step that ran the request.
 * A reset requested while a request is pending drops it: the tag is released by the step's reset, the outcome is
 * PTAM_INIT_MAP_STOPPED.  A step without a request enqueues and returns what it did before this entry existed.
 * PTAM_E_ARG: a null handle, keyframe or matches, n_matches < 4.  PTAM_E_STATE: a request is pending; the map has a keyframe (its
 * count is a host word that only the mapmaker's thread writes, while it makes, grows or clears a map: a tracker asks while no map
 * exists, when that thread idles at :79). */
int ptam_mapmaker_request_init(ptam_mapmaker*, const ptam_kf* first, ptam_kf* second, int n_matches, const ptam_trail* matches,
                               const ptam_rmap_init_opts* opts, int64_t tag);
/* *state: PTAM_MM_INIT_NONE (no request yet), _PENDING, _DONE.  DONE is set after the step's publish, so a tracker that reads it
 * finds the map in the snapshot; *out (nullable) is then the request's full result, readable until the next request.  Callable from
 * the tracker's thread.  PTAM_E_ARG: a null handle or state. */
int ptam_mapmaker_init_poll(ptam_mapmaker*, int32_t* state, ptam_rmap_init_result* out);
int ptam_mapmaker_flags(ptam_mapmaker*, int32_t* converged_recent, int32_t* converged_full, int32_t* bundle_running);
/* for tests, and for a host that resumes a map */
int ptam_mapmaker_set_flags(ptam_mapmaker*, int converged_recent, int converged_full);
/* up to cap tags the mapmaker has finished with, oldest first, removed from its list; *n: how many */
int ptam_mapmaker_released(ptam_mapmaker*, int cap, int64_t* tags, int32_t* n);
int ptam_mapmaker_step(ptam_mapmaker*, ptam_mapmaker_step_result*);

/* ---- The tracker: one frame of Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) as ONE call, hand-over included --------------
 *      A ptam_camera_tracker OWNS what the reference's Tracker owns for that branch — the ptam_tracker, the current keyframe
 *      (mCurrentKF), the rotation estimator (optional), the relocaliser's bank with its scratch image, the ptam_track_state, a pool
 *      of frame reports and a pool of keyframe clones — all created by _create, so a frame allocates nothing.  It BORROWS the
 *      ptam_map_snapshot the map is published into (keyframe section enabled) and the ptam_mapmaker (destroy the handle first).
 *      It lives on the tracker's thread, in `ctx`; of the mapmaker it uses only the entries that thread may call
 *      (ptam_mapmaker_released, _queue_size, _add_keyframe, _note_frame), so it touches neither the map's context nor its queue.
 *      TrackForInitialMap (:181) is the session entry below (ptam_camera_tracker_enable_session, _session_frames); without it a
 *      session starts with ptam_rmap_init_from_stereo, a publish and _reset(tracker pose).
 *      ptam_camera_tracker_track_frames, for nb handles in different contexts on one device (as ptam_track_frames_recover_batch asks)
 *      whose trackmap and state options are the same (PTAM_E_ARG otherwise: a chain takes them once):
 *        per camera   (a) ptam_mapmaker_released: a report whose tag came back is free again; a CLONE whose tag came back has been
 *                         inserted by the mapmaker's step and stays with the map until _reset / _destroy.  Handles that share a
 *                         mapmaker must be tracked in the same call (the tags are read once per mapmaker and dealt out).
 *                         PTAM_E_STATE, before anything is enqueued: no free report; no free clone while the frame could end in
 *                         AddKeyFrame (the camera is not lost and frame + 1 - last_keyframe_dropped > keyframe_gap).
 *                     (b) ptam_tracker_take_map and ptam_sbi_bank_take_keyframes from the snapshot.  PTAM_E_STATE "no map": nothing
 *                         was ever published, or the map has no point: this handle tracks a map that exists.
 *        together     (c) ptam_track_frames_report_batch with every camera's report, tag and seed (opts.shuffle_seed): the orders
 *                         are drawn on the device, the report is filled inside the chain.
 *        per camera   (d) :146-166.  ADD when the branch is PTAM_FRAME_TRACKED, the quality GOOD, frame - last_keyframe_dropped >
 *                         keyframe_gap, ptam_mapmaker_queue_size < max_queue and the report has records: ptam_kf_copy of the current
 *                         keyframe into a pooled clone (waited for: the mapmaker reads it on another queue),
 *                         ptam_mapmaker_add_keyframe(clone, the tracked pose, 0, report, the model's scene depth mean and sigma, tag),
 *                         last_keyframe_dropped = frame.  Otherwise NOTE for a TRACKED or RECOVERED frame whose report has records:
 *                         ptam_mapmaker_note_frame(report, tag).  A report that was not handed over is free again at once.
 *                     (e) the result.  tag = opts.tag_base + the state's frame at entry.
 *      Errors: a refusal in (a) or (b), or of the chain, leaves every state, estimator and pool where it was (tags that were released
 *      stay released, a take that succeeded stays taken: both only bring the handle up to date).  A failure in (d) — the mapmaker
 *      refusing — is returned behind the frames that were delivered; that camera's report is free again. */
typedef struct ptam_camera_tracker ptam_camera_tracker;
typedef struct {
    int32_t max_points;              /* the largest map the tracker takes */
    int32_t width, height;           /* of the frames: the context's image size */
    int32_t max_keyframes;           /* the relocaliser bank's capacity: the most keyframes a published map may hold */
    ptam_trackmap_opts trackmap;
    ptam_track_state_opts state;
    int32_t use_rotation_estimator;  /* 1: Tracker.UseRotationEstimator */
    int32_t keyframe_gap;            /* 20 (:148) */
    double rotation_blur;            /* 0.75: Tracker.RotationEstimatorBlur */
    uint64_t shuffle_seed;
    int64_t tag_base;
    int32_t max_queue;               /* 3 (:149) */
    int32_t reports, keyframes;      /* pool sizes; a keyframe clone that entered the map does not come back before _reset */
    int32_t pad_;
} ptam_camera_tracker_opts;
typedef struct {
    ptam_trackmap_result track;
    ptam_track_frame_state_info info;
    ptam_frame_report_info_t report;         /* as filled; the report itself may have gone to the mapmaker */
    ptam_map_take_result map_take;
    ptam_keyframes_take_result keyframes_take;
    int32_t added_keyframe, noted_frame, report_in_chain, queue_size;   /* queue_size: as asked in (d), before an add */
    int64_t tag;
} ptam_camera_track_result;
/* the reference's: trackmap and state defaults, estimator on, blur 0.75, gap 20, queue 3; max_points 8192, max_keyframes 64,
 * 8 reports, 32 keyframes, seed 0, tag_base 0; width / height 640 x 480 */
int ptam_camera_tracker_opts_default(ptam_camera_tracker_opts*);
int ptam_camera_tracker_create(ptam_ctx* ctx, const ptam_camera_tracker_opts* opts, ptam_map_snapshot* snapshot, ptam_mapmaker* mapmaker,
                               ptam_camera_tracker** out);
int ptam_camera_tracker_destroy(ptam_camera_tracker*);
/* Tracker::Reset (:52-62): the state at pose12 (ptam_track_state_reset), the estimator and the relocaliser's bank cleared, every
 * report and clone back in its pool (the map that named them is gone: ptam_mapmaker_request_reset is the caller's, before). */
int ptam_camera_tracker_reset(ptam_camera_tracker*, const double pose12[12]);
int ptam_camera_tracker_state(const ptam_camera_tracker*, ptam_track_state* out);
/* the inner handles, for drawing and tests; they stay the handle's.  _last_report: the report of the last frame (null before the
 * first); the next frame may refill it unless it went to the mapmaker. */
ptam_tracker* ptam_camera_tracker_tracker(ptam_camera_tracker*);
ptam_kf* ptam_camera_tracker_current_keyframe(ptam_camera_tracker*);
ptam_frame_report* ptam_camera_tracker_last_report(ptam_camera_tracker*);
/* free reports and free clones, for a caller that watches its pools */
int ptam_camera_tracker_pool(const ptam_camera_tracker*, int32_t* free_reports, int32_t* free_keyframes);
int ptam_camera_tracker_track_frames(int nb, ptam_camera_tracker* const* handles, const uint8_t* const* d_frames,
                                     ptam_camera_track_result* results);

/* ---- A session from the first frame: Tracker::TrackForInitialMap (src/Tracker.cc:181, :311-347) in the handle ---------------------------
 *      ptam_camera_tracker_enable_session gives the handle the reference's mnInitialStage state machine: it allocates the trails
 *      object (ptam_trails, max_initial_trails) and mFirstKF up front, so that a frame still allocates nothing, and puts the handle
 *      in TRAIL_TRACKING_NOT_STARTED with the state of Tracker::Reset (:49-65) at the identity.  PTAM_E_STATE while a report or a
 *      clone is out, or when the session is enabled already.  A handle WITHOUT it behaves as before: it tracks a map that exists,
 *      "no map" is PTAM_E_STATE, in ptam_camera_tracker_track_frames and in the session entry alike.
 *      ptam_camera_tracker_restart is the tracker's side of Tracker::Reset (:49-65): ptam_camera_tracker_reset at the identity plus
 *      stage NOT_STARTED; ptam_mapmaker_request_reset stays the caller's, before, as for _reset.
 *      ptam_camera_tracker_session_frames, for nb handles (pokes: nullable; pokes[i] != 0 is mbUserPressedSpacebar of camera i for
 *      this frame).  Each handle takes the branch its stage selects (:311-347); mnFrame counts in every stage (:111) and is NOT reset
 *      when the map is made:
 *        NOT_STARTED  no poke: MakeKeyFrame_Lite (:92) of the frame, nothing else (:321-323).  Poke (:315-320): MakeKeyFrame_Lite,
 *                     ptam_make_keyframe_rest (:354), ptam_kf_copy into mFirstKF (:355), ptam_trails_start (:356-369); STARTED.
 *        STARTED      all such cameras of the call go through ONE ptam_trails_advance_batch (:328); one such camera alone takes
 *                     ptam_make_keyframe_lite_dev + ptam_trails_advance, the same bits and the shorter path for one.  n_good < min_good_trails
 *                     (:329): the tracker's side of Reset() — trail_reset = 1, NOT_STARTED; no mapmaker reset is requested: the map
 *                     is empty in this stage by construction (a handle gets here only from NOT_STARTED, and leaves a map only
 *                     through _restart or a failed initialisation, which leaves the map empty).  Otherwise, with a poke
 *                     (:335-343): ptam_trails_read (vMatches, :338-340); two pooled clones receive mFirstKF and the current
 *                     keyframe (ptam_kf_copy, one ptam_ctx_sync: the mapmaker reads them on its queue);
 *                     ptam_mapmaker_request_init(first clone, second clone, the matches, opts.init, tag); COMPLETE, the request
 *                     pending.  Fewer than two free clones: PTAM_E_STATE, decided at the call's entry for every STARTED handle that
 *                     is poked, before anything is enqueued.
 *        COMPLETE, request pending: ptam_mapmaker_init_poll.  PENDING: MakeKeyFrame_Lite and the frame count, no error (the
 *                     reference's tracker is inside InitFromStereo meanwhile).  DONE and PTAM_INIT_MAP_OK: the motion model is
 *                     reset at result.tracker_pose (mse3CamFromWorld, :341; zero velocity) with `frame` and
 *                     `last_keyframe_dropped` kept, the estimator is reset, and THIS frame goes on to the tracking branch.  DONE
 *                     and not OK: the handle does the tracker's side of Reset(), the two clones go back to the pool and
 *                     init_status says why.  DEVIATION: the reference stays in COMPLETE without a map for ever (:127 never holds).
 *        COMPLETE with a map: the body of ptam_camera_tracker_track_frames on that subset, the same code.
 *      The trail-stage cameras run first, then the tracking subset; each subset obeys its batch call's conditions (different
 *      contexts, one device, one image size; for the tracking subset one set of options).  A refusal of the tracking subset is
 *      returned behind the trail-stage cameras' frames, which have been delivered (their session rows say so).
 *      A camera whose map has just been made and whose tracking call is refused keeps its request pending and its state: the next
 *      call reads the outcome again (init_done is reported with the frame that is delivered).
 *      results[i] is zero for a camera that did not track.  tag of a request: opts.tag_base + the state's frame at entry.  Reset()
 *      puts the frame count back to 0 (:63), so tags repeat from one session of a handle to the next.  The tag of a request that
 *      made no map stays in the mapmaker's released list until a tracking call of this handle's mapmaker reads it; it then names
 *      nothing here (the clones were freed when the outcome was read), or the clones of a later request that has made its map, which
 *      are the map's by then: either reading is right. */
enum { PTAM_TRAIL_TRACKING_NOT_STARTED, PTAM_TRAIL_TRACKING_STARTED, PTAM_TRAIL_TRACKING_COMPLETE };   /* mnInitialStage */
typedef struct {
    int32_t max_initial_trails;      /* 1000: Tracker.MaxInitialTrails (:360) */
    int32_t min_good_trails;         /* 10 (:329) */
    double min_shi_tomasi;           /* 70: the candidates' threshold (src/KeyFrame.cc:66-76) */
    ptam_rmap_init_opts init;
} ptam_camera_session_opts;
typedef struct {
    int32_t stage_before, stage_after;   /* PTAM_TRAIL_TRACKING_* */
    int32_t poked;                       /* the poke was consumed (:317, :337, :52) */
    int32_t n_trails;                    /* a start: the trails made */
    int32_t n_good, n_alive;             /* an advance: nGoodTrails, the list's length afterwards */
    int32_t trail_reset;                 /* :329-332 */
    int32_t init_requested, init_done;   /* the request went out with this frame | its outcome was read with this frame */
    int32_t init_status;                 /* PTAM_INIT_MAP_*, with init_done */
    int32_t tracked, pad_;               /* the frame went through the tracking branch: results[i] is filled */
    int64_t init_tag;                    /* with init_requested */
} ptam_camera_session_result;
/* 1000 / 10 / 70, ptam_rmap_init_opts_default.  PTAM_E_ARG: a null pointer */
int ptam_camera_session_opts_default(ptam_camera_session_opts*);
/* opts nullable: the defaults.  PTAM_E_ARG: a null handle, max_initial_trails < 1, min_good_trails < 0 */
int ptam_camera_tracker_enable_session(ptam_camera_tracker*, const ptam_camera_session_opts* opts);
int ptam_camera_tracker_restart(ptam_camera_tracker*);
int ptam_camera_tracker_session_frames(int nb, ptam_camera_tracker* const* handles, const uint8_t* const* d_frames, const uint8_t* pokes,
                                       ptam_camera_track_result* results, ptam_camera_session_result* session);
/* the inner trails object (null without a session) and the last request's full result (PTAM_E_STATE before one was read), for drawing
 * and tests; *stage (nullable): mnInitialStage, PTAM_TRAIL_TRACKING_COMPLETE without a session */
ptam_trails* ptam_camera_tracker_trails(ptam_camera_tracker*);
int ptam_camera_tracker_init_result(const ptam_camera_tracker*, ptam_rmap_init_result* out);
int ptam_camera_tracker_stage(const ptam_camera_tracker*, int32_t* stage);

/* ---- The camera calibrator's optimiser: CameraCalibrator::OptimizeOneStep (src/CameraCalibrator.cc:215-269) with
 *      CalibImage::GuessInitialPose and CalibImage::Project (src/CalibImage.cc:514-648) and ATANCamera::RefreshParams /
 *      GetCameraParameterDerivs / UpdateParams / DisableRadialDistortion (src/ATANCamera.cc:27-66, 211-252), fp64 throughout.
 *      The checkerboard finder (CalibImage::MakeFromImage, CalibCornerPatch) is NOT here: the corners come from the caller's
 *      detector, each a pixel position (Params.v2Pos) and an integer grid position (irGridPos); the world point of a corner is
 *      (gx, gy, 0).  A ptam_calibrator lives on a ptam_ctx and uses its device, its queue and its image size; the context's own
 *      camera plays no part.  All its memory is allocated by ptam_calib_create.
 *      The camera of the moment — the five parameters, RefreshParams of them and of params + 0.001 e_i (the forward
 *      differences of GetCameraParameterDerivs) — lives on the device and is refreshed there by every step; the host never
 *      holds it between steps.
 *      ptam_calib_add_images: GuessInitialPose with the camera of the moment (src/CameraCalibrator.cc:105-106), one workgroup
 *      per image: UnProject of every corner, the 2n x 9 DLT matrix, its right null vector by one-sided Jacobi (as the DLT of
 *      ptam_homography_init), the 2x2 top-left fix-up (:563-583), Gram-Schmidt and the translation (:586-605).
 *      DEVIATION (sign): the reference takes get_VT()[8] with whatever sign LAPACK gives it, so a camera can end up BEHIND the
 *      grid; Project then skips every corner and mdMeanPixelError is 0 / 0.  Here the null vector has the sign for which the
 *      translation's z is positive.  An image whose guess is not finite or whose z is 0 gets PTAM_CALIB_GUESS_REFUSED in
 *      status_out and is not added (the images after it move up).
 *      ptam_calib_optimize: `steps` times OptimizeOneStep, one kernel launch per step plus one closing launch, enqueued back to
 *      back, ONE host wait at the end.  Per measurement the skip tests (v3Cam[2] <= 0.001, Camera.Invalid()), the error, the
 *      2x6 pose Jacobian (GetProjectionDerivs, generator_field) and the 2x5 camera Jacobian by the reference's forward
 *      differences of 0.001 (column 4 zero when w == 0).  The system has an arrowhead shape — a 6x6 block D_n = I + sum Jp^T Jp
 *      per view, the shared 5x5 block C = I + sum Jc^T Jc, 6x5 couplings B_n — and is solved by block elimination: Cholesky of
 *      every D_n, the 5x5 reduced system (C - sum B_n^T D_n^-1 B_n) delta_c = (Jc^T e - sum B_n^T D_n^-1 e_n), then
 *      delta_n = D_n^-1 (e_n - B_n delta_c); params += 0.1 delta_c, pose_n = SE3::exp(0.1 delta_n) * pose_n (:265-268).
 *      DEVIATION (no truncation): the reference takes the SVD of the dense (6 views + 5)^2 matrix and back-substitutes with
 *      TooN's condition cut, which drops singular values below 1e-9 of the largest.  The matrix is I + J^T J, so nothing is ever
 *      singular; the two solutions agree while the condition number stays well below 1e9 and differ beyond it.
 *      With disable_distortion, params[4] is 0 at the start of every step (:226); with w == 0 its column is zero and its row of
 *      the 5x5 system is the prior alone, so it stays exactly 0.
 *      DEVIATION (nothing to adjust): when no measurement survives the skip tests the reference divides by zero (:260).  Here
 *      such a step changes nothing — the update is gated on the device by the step's own count — and a call whose FIRST step
 *      finds no measurement returns status PTAM_CALIB_NO_MEASUREMENTS with parameters and poses as they were.
 *      Every sum is reduced in a fixed order: two runs on the same input give the same bits, and `steps` steps in one call give
 *      the same bits as `steps` calls of one step. */
typedef struct ptam_calibrator ptam_calibrator;
enum { PTAM_CALIB_OK = 0, PTAM_CALIB_NO_MEASUREMENTS = 1 };
enum { PTAM_CALIB_GUESS_OK = 0, PTAM_CALIB_GUESS_REFUSED = 1 };
enum { PTAM_CALIB_MAX_IMAGES = 65536, PTAM_CALIB_MAX_CORNERS = 4194304, PTAM_CALIB_MAX_STEPS = 65536 };
typedef struct { int32_t gx, gy; double u, v; } ptam_calib_corner;   /* irGridPos, Params.v2Pos */
typedef struct {
    int32_t status;               /* PTAM_CALIB_OK / PTAM_CALIB_NO_MEASUREMENTS */
    int32_t n_measurements;       /* nTotalMeas of the last step */
    int32_t steps;                /* the steps of this call */
    int32_t pad_;
    double  params[5];            /* Camera.Parameters after the call */
    double  rms;                  /* mdMeanPixelError of the last step: computed before that step's update (:260) */
    double  pixel_aspect_ratio;   /* ATANCamera::PixelAspectRatio: fy * height / (fx * width) */
} ptam_calib_result;
/* PTAM_E_ARG: max_images outside [1, PTAM_CALIB_MAX_IMAGES], max_corners_total outside [4, PTAM_CALIB_MAX_CORNERS].  The handle
 * starts as after ptam_calib_reset(h, NULL, 0). */
int ptam_calib_create(ptam_ctx*, int max_images, int max_corners_total, ptam_calibrator** out);
int ptam_calib_destroy(ptam_calibrator*);
/* CameraCalibrator::Reset (:156-165): params (NULL: mvDefaultParams = 0.5, 0.75, 0.5, 0.5, 0.1), DisableRadialDistortion when
 * disable_distortion, no images.  PTAM_E_ARG: a non-finite parameter, fx or fy of 0. */
int ptam_calib_reset(ptam_calibrator*, const double* params /* 5 or NULL */, int disable_distortion);
int ptam_calib_counts(ptam_calibrator*, int32_t* n_images, int32_t* n_corners);
/* n images; image k's corners are corners[first_corner[k] .. first_corner[k + 1]), first_corner[0] == 0.  status_out: n entries of
 * PTAM_CALIB_GUESS_*.  One host wait (a second one only when an image was refused by the device). */
int ptam_calib_add_images(ptam_calibrator*, int n, const int32_t* first_corner /* n + 1 */, const ptam_calib_corner* corners,
                          int32_t* status_out);
/* mse3CamFromWorld of every image, 12 doubles each: R row-major, then t. */
int ptam_calib_set_poses(ptam_calibrator*, const double* poses /* 12 x images */);
int ptam_calib_read_poses(ptam_calibrator*, double* poses /* 12 x images */);
/* rms_history (nullable): `steps` entries, mdMeanPixelError of every step; written with status PTAM_CALIB_OK only. */
int ptam_calib_optimize(ptam_calibrator*, int steps, ptam_calib_result* result, double* rms_history);
int ptam_calib_params(ptam_calibrator*, double params[5]);
/* What Draw3DGrid(Camera, true) draws for one image (src/CalibImage.cc:493-501): Camera.Project(project(mse3CamFromWorld * v3)) of
 * every corner, 2 doubles each, and valid = the corner passes Project's skip tests.  A corner with v3Cam[2] <= 0.001 has
 * (0, 0) and valid 0; the error the reference draws is the corner's own position minus projected_uv. */
int ptam_calib_residuals(ptam_calibrator*, int image, double* projected_uv /* 2 x corners */, int32_t* valid);
/* PTAM_E_ARG, with nothing written and the handle byte for byte as it was: a null pointer (rms_history excepted); an image with
 * fewer than 4 corners; a grid position twice in one image; a non-finite corner position, pose or parameter; steps < 1 or
 * > PTAM_CALIB_MAX_STEPS; more images or corners than the handle was created for; fx or fy of 0; an image index outside the
 * handle's images.  PTAM_E_STATE: ptam_calib_optimize or ptam_calib_set_poses without images. */

/* ---- sharded global BA: measurements sharded by point across ranks ----------- */
/* A collective hook: all-reduce (sum) `count` doubles in place at device pointer `dptr`,
 * ordered on `stream` (hipStream_t).  Return 0 on success. */
typedef int (*ptam_allreduce_f64_fn)(void* user, double* dptr, size_t count, void* stream);
/* Attach a communicator to a bundle: `rank`'s bundle holds ALL cameras but only its shard of the
 * points (and every measurement of those points).  With a hook attached, Compute all-reduces the
 * camera system (S lower blocks + E), the error scalars and the median histogram per trial.
 * Failure semantics: what decides the SEQUENCE of collectives is itself collective — the abort flag, a shard that cannot
 * be prepared, a rank without measurements — so every rank leaves Compute at the same trial with an error or a result.
 * A failure that strikes ONE rank between two collectives of a trial (a HIP error, an allocation failure, the hook
 * returning non-zero) is returned by that rank at once; the others are by then inside (or on their way into) the next
 * all-reduce and can only be released by the communicator: the hook MUST time out or be abortable (RCCL: the
 * communicator's own abort / watchdog; torch.distributed: the process group's timeout), after which the process group is
 * to be torn down — the bundle's device state is undefined. */
int ptam_ba_set_comm(ptam_ba* ba, int rank, int world, ptam_allreduce_f64_fn fn, void* user);

/* built-in RCCL implementation of the hook (librccl is dlopen'ed on first use) */
typedef struct ptam_rccl ptam_rccl;
int ptam_rccl_unique_id(uint8_t id_out[128]);
int ptam_rccl_create(ptam_ctx* ctx, const uint8_t id[128], int rank, int world, ptam_rccl** out);
int ptam_rccl_destroy(ptam_rccl* c);
int ptam_rccl_allreduce_f64(void* comm /* ptam_rccl* */, double* dptr, size_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PTAM_HIP_H */
