// sbi.h — what motion.hip's tracked frame needs of the rotation estimator (sbi.hip)
#pragma once
#include "common.h"

// The estimator's step for one frame (src/Tracker.cc:94-108 + :1018-1020): this frame's SmallBlurryImage from kf's level 3 into the
// free slot, aligned against last frame's (against itself on the first frame after a reset); two launches and one mapped wait.
// Nothing of the estimator's state changes until sbi_estimator_commit: a frame that fails later is simply stepped again.
int sbi_estimator_step(ptam_rotation_estimator* e, const ptam_kf* kf, ptam_sbi_alignment* out);
void sbi_estimator_commit(ptam_rotation_estimator* e);   // this frame's image becomes "last"
ptam_ctx* sbi_estimator_ctx(const ptam_rotation_estimator* e);

// ---- a batch of frames (ptam_track_frames_batch): the estimators' steps as two launches for all frames ----
// One frame with an estimator, in device memory: this frame's SmallBlurryImage is made from l3 into the estimator's free slot, aligned
// against the target (last frame's; its own after a reset), and thread 0 of the align workgroup predicts the frame's pose.
struct SbiBatchRec {
    const uint8_t* l3;              // make: aLevels[3].im of the frame's keyframe
    uint8_t* small;                 //       mimSmall / mimTemplate / mimImageJacs of the free slot
    float* tmpl;
    float* jacs;
    const float* tgt_tmpl;          // align: the target's mimTemplate / mimImageJacs
    const float* tgt_jacs;
    double velocity[6];             // predict: the model's velocity and the pose it starts from
    double start_pose[12];
    double* pose_out;               // the frame's pose on the device (the PVS pass reads it)
    ptam_sbi_alignment* h_align;    // host-mapped: the alignment and the predicted pose
    double* h_pose_in;
};
// the make / align part of e's record for a frame whose keyframe is kf, and "pending" as sbi_estimator_step leaves it (host only)
int sbi_batch_rec(ptam_rotation_estimator* e, const ptam_kf* kf, SbiBatchRec* rec);
void sbi_estimator_rollback(ptam_rotation_estimator* e);   // forget the pending slot: the estimator is where it was
// the two launches on `st` for n records at d_recs; lead: an estimator of the batch (all share image size and blur)
int sbi_batch_launch_make(const ptam_rotation_estimator* lead, int n, const SbiBatchRec* d_recs, hipStream_t st);
// nb_detect > 0: the same launch also runs the FAST detection of nb_detect keyframes of geometry *L (kf_launch_detect_batch's job and
// arguments) in workgroups behind the align ones
struct KfLevels;
int sbi_batch_launch_align(const ptam_rotation_estimator* lead, int n, const SbiBatchRec* d_recs, hipStream_t st, int nb_detect = 0,
                           const KfLevels* L = nullptr, const void* det_items = nullptr, size_t det_stride = 0, size_t det_off = 0);
// ---- a batch's recovering cameras (ptam_track_frames_recover_batch): Relocaliser::AttemptRecovery inside the frames' chain ----
// One recovering camera, in device memory.  Its relocaliser image is made by a make launch of its own (the blur differs from the
// estimators') from an SbiBatchRec whose l3 / small / tmpl / jacs are filled; row y of the SSD launch takes record y's image against
// every entry of its bank into the camera's OWN table (a bank may serve several cameras); an align workgroup behind the estimators'
// takes the arg-min, aligns, and thread 0 forms mse3Best, decides `good` and writes pose, result and gate.
struct SbiRelocRec {
    const float* cur;               // the scratch image's mimTemplate
    const float* bank_tmpl;         // entry 0's mimTemplate / mimImageJacs
    const float* bank_jacs;
    const double* bank_poses;       // se3CfromW of the entries, 12 doubles each
    double* ssd;                    // [count]
    int count, pad_;
    double max_score;
    double* pose_out;               // the frame's pose on the device, written when good
    ptam_reloc_result* h_reloc;     // host-mapped
    int* gate;                      // 1: good, the frame's TrackMap kernels run; 0: they return at once
};
// refusals, host only: PTAM_E_ARG / PTAM_E_STATE as ptam_track_frames_recover_batch lists them
int sbi_reloc_check(const ptam_sbi_bank* b, const ptam_sbi* scratch, int device, const ptam_kf* kf);
void sbi_reloc_rec(const ptam_sbi_bank* b, const ptam_sbi* scratch, const ptam_kf* kf, SbiBatchRec* make_rec, SbiRelocRec* rec);
void sbi_reloc_commit(ptam_sbi* scratch);   // the scratch holds an image
ptam_ctx* sbi_bank_ctx(const ptam_sbi_bank* b);
// the camera positions (-R^T t, 3 doubles each) of the bank's host mirror of its poses: *count entries; nullptr while a pose was never set
const double* sbi_bank_camera_positions(const ptam_sbi_bank* b, int* count);
// the launches on `st`; ctx: the lead tracker's (halfSample variant, camera), b: a bank of the batch (image size)
int sbi_reloc_launch_make(ptam_ctx* ctx, const ptam_sbi_bank* b, double blur, int n, const SbiBatchRec* d_recs, hipStream_t st);
int sbi_reloc_launch_ssd(const ptam_sbi_bank* b, int n, int max_count, const SbiRelocRec* d_rrecs, hipStream_t st);
// sbi_batch_launch_align with n_reloc relocaliser workgroups between the n_est estimator ones (n_est may be 0) and the detection's
int sbi_recover_launch_align(ptam_ctx* ctx, const ptam_sbi_bank* b, int n_est, const SbiBatchRec* d_recs, int n_reloc, const SbiRelocRec* d_rrecs,
                             hipStream_t st, int nb_detect, const KfLevels* L, const void* det_items, size_t det_stride, size_t det_off);
// ---- the keyframe section of a ptam_map_snapshot (ptam_snapshot_keyframes_enable), as ptam_rmap_publish fills it ----
// Host only, before a slot is taken; all of them return at once for a snapshot that was never enabled.
struct ptam_map_snapshot;
bool sbi_snapshot_kf_enabled(ptam_map_snapshot* snap);
// PTAM_E_LIMIT: n_kf above max_keyframes; PTAM_E_ARG: a keyframe whose level 3 is not the snapshot's frame size / 8
int sbi_snapshot_kf_check(ptam_map_snapshot* snap, int n_kf, const ptam_kf* const* kfs);
// the first keyframe of map (map_id, epoch) whose image slot s does not hold: the slot's count for the same map, else 0
int sbi_snapshot_kf_first_missing(const ptam_map_snapshot* snap, int s, long long map_id, long long epoch, int n_kf);
// on ctx's queue: the pose table [0, n_kf) device to device into slot s, and ONE make launch (grid x = n_kf - first) for the
// entries [first, n_kf); d_l3: their level-3 addresses, in device memory
int sbi_snapshot_kf_enqueue(ptam_ctx* ctx, ptam_map_snapshot* snap, int s, int n_kf, const double* d_poses, int first, const uint8_t* const* d_l3);
// after the publish's wait, before its commit: what slot s now holds
void sbi_snapshot_kf_stamp(ptam_map_snapshot* snap, int s, int n_kf, int first, long long map_id, long long epoch, long long generation);
bool sbi_estimator_fits_bank(const ptam_rotation_estimator* e, const ptam_sbi_bank* b);   // same frame size
bool sbi_estimators_alike(const ptam_rotation_estimator* a, const ptam_rotation_estimator* b);   // same image size and blur
