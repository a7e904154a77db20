// trails_internal.h — what ptam_rmap_init_from_stereo (maprmap_init.hip) needs of trails.hip: where a trails object keeps its live
// list, and the two kernels of InitFromStereo's match table and point loop as launches on tables in device memory.
#pragma once
#include "common.h"
#include "keyframe.h"

struct TrailsView {
    ptam_ctx* ctx;
    int w, h, started, n_live;
    const ptam_trail* d_trails;        // the live list, in list order
    ptam_homography_match* d_out;      // the object's own staging: room for max_trails matches
};
void trails_view(const ptam_trails* t, TrailsView* out);
// the match table of src/MapMaker.cc:272-279 from n trails: one launch, enqueues only
int trails_matches_enqueue(ptam_ctx* ctx, int n, const ptam_trail* d_trails, ptam_homography_match* d_out);
// the point loop of :310-367 on n matches: status[i] and, where it is PTAM_INIT_MADE, pts[i]; one launch, enqueues only
int init_points_enqueue(ptam_ctx* ctx, const ptam_kf* first, const ptam_kf* second, const double se3_second_from_first[12], int subpix_max_its,
                        int n, const ptam_trail* d_matches, int* d_status, ptam_new_map_point* d_pts);
