// sbi.h — what motion.hip's tracked frame needs of the rotation estimator (sbi.hip)
#pragma once
#include "common.h"

// The estimator's step for one frame (src/Tracker.cc:94-108 + :1018-1020): this frame's SmallBlurryImage from kf's level 3 into the
// free slot, aligned against last frame's (against itself on the first frame after a reset); two launches and one mapped wait.
// Nothing of the estimator's state changes until sbi_estimator_commit: a frame that fails later is simply stepped again.
int sbi_estimator_step(ptam_rotation_estimator* e, const ptam_kf* kf, ptam_sbi_alignment* out);
void sbi_estimator_commit(ptam_rotation_estimator* e);   // this frame's image becomes "last"
ptam_ctx* sbi_estimator_ctx(const ptam_rotation_estimator* e);
