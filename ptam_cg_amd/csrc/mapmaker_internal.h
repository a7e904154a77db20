// mapmaker_internal.h — the launch chain of mapmaker.hip (epi_select / epi_point / epi_emit per visited level), for the callers that
// write its busy list on the device and leave its records there (ptam_rmap_insert_keyframe, maprmap.hip).
#pragma once
#include "common.h"
#include "keyframe.h"

struct EpiBusy {        // a busy measurement of kSrc: nLevel, v2RootPos
    double x, y;
    int level, pad_;
};
// the chain's header: {n_busy, n_out, n_kept, pad}, then one ptam_epipolar_level_stats per visited level
enum { EPI_HDR_BYTES = 16 + sizeof(ptam_epipolar_level_stats) * PTAM_LEVELS };
struct EpiRun {         // one chain's work memory in the context's scratch
    int nl, sum, most;              // visited levels; the sum and the maximum of their maximal-corner counts
    int n_max[PTAM_LEVELS];
    EpiBusy* d_busy;                // n_busy + sum + 1: the caller's entries first, a made point's SRC_ROOT behind them
    void* d_kept;                   // most + 1 kept candidates
    int* d_status;                  // most + 1
    ptam_new_map_point* d_pts;      // most + 1: a level's points by kept candidate
    ptam_new_map_point* d_out;      // sum + 1: the made points, in the order of ptam_add_map_points_epipolar
    int* d_hdr;                     // EPI_HDR_BYTES
};
// what refuses a chain without touching the device: the level list (PTAM_E_ARG), a source without MakeKeyFrame_Rest (PTAM_E_STATE)
int epi_check(const ptam_kf* src, const ptam_epipolar_opts* opts);
// the visited levels' maximal-corner counts -> run.nl / sum / most / n_max
int epi_sizes(ptam_ctx* ctx, const ptam_kf* src, const ptam_epipolar_opts* opts, EpiRun& run);
// the target's implane tables (bImplaneCornersCached, src/MapMaker.cc:609-614) and the scratch for n_busy caller's entries
int epi_carve(ptam_ctx* ctx, ptam_kf* target, const ptam_epipolar_opts* opts, int n_busy, EpiRun& run);
// the three launches per visited level, enqueued on the context's stream; d_busy[0, n_busy) and d_hdr = {n_busy, 0, ...} are
// written by work enqueued before
int epi_launch_chain(ptam_ctx* ctx, const ptam_kf* src, const double src_pose[12], const ptam_kf* target, const double target_pose[12],
                     const ptam_epipolar_opts* opts, const EpiRun& run);
