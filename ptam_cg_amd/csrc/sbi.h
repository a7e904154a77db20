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
bool sbi_estimators_alike(const ptam_rotation_estimator* a, const ptam_rotation_estimator* b);   // same image size and blur
