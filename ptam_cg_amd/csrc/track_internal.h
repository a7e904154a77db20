// track_internal.h — launch helpers the resident TrackMap chain (trackmap.hip) uses from the other translation units.
// Every helper only enqueues on the context's stream; slot ranges and counts live in DEVICE memory (d_range = {begin, end},
// d_n), because which patches are searched and how many are found is decided on the device (no host round trip inside a
// tracked frame).
#pragma once
#include "common.h"
#include "keyframe.h"

struct TemplateJob {          // device-side form of ptam_template_query (keyframe handle resolved to its level image)
    const uint8_t* im;
    int w, h;
    int search_level;
    int cx, cy;
    double wi[4];
};

struct TmSrc {   // MapPoint::pPatchSourceKF / nSourceLevel / irCenter, resolved to the level image
    const uint8_t* im;
    int w, h;
    int cx, cy;
};

// patch.hip
// Level::vImplaneCorners of one level of kf, built on the context's stream unless cached (bImplaneCornersCached)
int kf_build_implane(ptam_ctx* ctx, ptam_kf* kf, int level);
int patch_launch_templates_dev(ptam_ctx* ctx, int n_cap, const TemplateJob* d_jobs, uint8_t* d_tmpl, ptam_template_result* d_res,
                               const int* d_range);
// d_tres (nullable): a query whose template came out bad (Finder.TemplateBad(), src/Tracker.cc:876) is not searched
int patch_launch_search_dev(ptam_ctx* ctx, const ptam_kf* kf, int n_cap, const ptam_patch_query* d_q, const uint8_t* d_tmpl,
                            ptam_patch_result* d_r, const int* d_range, const ptam_template_result* d_tres);
// sub-pixel refinement of the patches the coarse search found (queries taken from the search's own queries / results)
int patch_launch_subpix_dev(ptam_ctx* ctx, const ptam_kf* kf, int n_cap, const ptam_patch_query* d_q, const ptam_patch_result* d_pr,
                            const uint8_t* d_tmpl, ptam_subpix_result* d_sr, const int* d_range, int max_its);
// keyframe.hip: KeyFrame::MakeKeyFrame_Lite of a device-resident frame, enqueued on `stream`
int kf_make_lite_on(ptam_ctx* ctx, ptam_kf* kf, const uint8_t* d_im, hipStream_t stream);
// the same in pieces, for a caller that fuses the pyramid and the compaction into launches of its own (keyframe_device.h)
struct PyrArgs;
void kf_lite_begin(ptam_kf* kf, const uint8_t* d_src, PyrArgs* a_out, int* gx, int* gy);
void kf_launch_detect(ptam_kf* kf, hipStream_t stream);
// FAST detection for nb keyframes of equal geometry in one launch: their KfLevels sit at d_items + i * stride + off_levels
void kf_launch_detect_batch(int nb, const KfLevels& L, const void* d_items, size_t stride, size_t off_levels, hipStream_t stream);   // (L: the common geometry)
// tracker_run.hip: a frame's two random orders drawn on the device (ptam_tracker_draw_shuffles), enqueued on st: n entries into each
// of perm_a / perm_b.  keys: 4 n 64-bit words of work for a map of more than TR_DRAW_LDS_MAX points (not looked at otherwise)
enum { TR_DRAW_LDS_MAX = 8192 };
int tr_draw_shuffles_on(hipStream_t st, int n, uint64_t seed, uint64_t frame, int* perm_a, int* perm_b, unsigned long long* keys);
// the same for the cameras of a batch chain whose maps hold at most TR_DRAW_LDS_MAX points: a job table in device memory, one launch
struct TrDrawJob {
    unsigned long long seed, frame;
    int* perm_a;
    int* perm_b;
    int n, pad_;
};
int tr_draw_shuffles_batch_on(hipStream_t st, int nb, int n_max, const TrDrawJob* d_jobs);
// trackmap.hip: the context a tracker was created with
ptam_ctx* tracker_ctx(const ptam_tracker* t);
// motion.hip
// The bTryCoarse heuristics (src/Tracker.cc:503-514) on a copy of the caller's options and a copy of the model: coarse when the camera
// moves fast enough and CoarseMax allows it; after a recovery — the model's just_recovered, which is cleared, or `recovering`: the
// relocaliser runs in front of this very TrackMap — coarse in any case, with CoarseMax and CoarseRange doubled.  -> doubled or not
bool track_coarse_heuristics(ptam_trackmap_opts* o, ptam_motion_model* m, bool recovering);
// the scene depth of src/Tracker.cc:692-696, the part of ptam_motion_update a recovered frame keeps
void motion_update_scene_depth(ptam_motion_model* m, const ptam_trackmap_result* r);
// the camera position of an se3CfromW: se3CfromW.inverse().get_translation() = -R^T t (KeyFrameLinearDist, src/MapMaker.cc:696-703)
static inline void se3_camera_position(const double p[12], double out[3]) {
    for (int k = 0; k < 3; k++) out[k] = -(p[k] * p[9] + p[3 + k] * p[10] + p[6 + k] * p[11]);
}
// pvs.hip
struct PoseArg {   // a pose handed over by value
    double v[12];
    int use;
};
// host_pose (nullable): the pose as a kernel argument, also written to d_pose; otherwise d_pose is read
// d_finder_bad (nullable): word i * finder_stride bytes further on is set when point i's warp is rejected (PatchFinder::mbTemplateBad)
int pvs_launch_dev(ptam_ctx* ctx, int n, const ptam_pvs_point* d_pts, double* d_pose, const double* host_pose, ptam_pvs_result* d_out,
                   int* d_finder_bad = nullptr, int finder_stride = 0);

// pose.hip: the ten-iteration loop on a measurement list whose length sits in device memory, with the extras of the chain
struct PoseChainIo {
    // TrackerData state of the measurements when the loop ends (v3Cam, v2Image, m2CamDerivs as left by the last
    // ProjectAndDerivs / LinearUpdate), scattered to td_base + td_index[i] * td_stride bytes (ptam_projection each); null: no
    void* td_base;
    const int* td_index;
    int td_stride;
    // scene depth statistics over the measurements (src/Tracker.cc:680-690): {sum z, sum z^2, count}; null: no
    double* depth_out;
    // the frame's result block in host-mapped memory: the loop's last act is to publish the pose (12 doubles at
    // result_pose), the depth sums (3 doubles at result_depth) and then the sequence word the host spins on; null: no
    double* result_pose;
    double* result_depth;
    unsigned long long* result_seq;
    unsigned long long seq;
};
// one frame of a batch (ptam_track_map_frames_batch): what pose_launch_chain takes as arguments, in device memory
struct PoseBatchItem {
    int n_cap;                      // capacity of the list (its length sits at n_dev)
    const int* n_dev;
    const ptam_pose_meas* meas;
    const ptam_projection* entry;
    double* pose_io;
    int32_t* flags;                 // outlier flags (nullable)
    double* updates;                // scratch: the iterations' updates
    void* st;                       // scratch of the general kernel (lists of more than 1024 measurements)
    PoseChainIo io;
};
int pose_launch_chain_batch(ptam_ctx* ctx, int nb, int n_cap_max, const PoseBatchItem* d_items, const ptam_gn_opts* opts);
int pose_chain_scratch(ptam_ctx* ctx, int n_cap, void** st_out, double** updates_out);
#define POSE_CHAIN_LONG (1ull << 63)   // in the published sequence word: "the list is longer than the register-resident kernel holds" (pose.hip)
int pose_launch_chain(ptam_ctx* ctx, int n_cap, const int* d_n, const ptam_pose_meas* d_meas, const ptam_projection* d_entry,
                      double* d_pose_inout, const ptam_gn_opts* opts, int32_t* d_outlier_flags, const PoseChainIo& io, int mode = 0);
