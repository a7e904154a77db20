// homography.h — HomographyInit::Compute on the device (homography.hip), as the trails object calls it on its own match table.
#pragma once
#include "common.h"

// PTAM_E_ARG unless the options are usable for n matches (ptam_hip.h lists the refusals); nothing is written
int homog_check(int n, const ptam_homography_opts* opts);
// device scratch and pinned staging a call with n matches and `trials` hypotheses takes from the context
void homog_sizes(int n, int trials, size_t* scratch_bytes, size_t* pinned_bytes);
// The whole of Compute on n matches: d_matches on the device, or (d_matches == nullptr) h_matches on the host, uploaded first.
// Arguments checked by the caller (homog_check).  Two launches, one read-back, one host wait.
int homog_run(ptam_ctx* ctx, int n, const ptam_homography_match* d_matches, const ptam_homography_match* h_matches,
              const ptam_homography_opts* opts, double se3_second_from_first[12], ptam_homography_info* info, uint8_t* inlier_out);
