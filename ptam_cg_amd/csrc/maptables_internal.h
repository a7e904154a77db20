// maptables_internal.h — the device cores of the map-table edits (maptables.hip).  Every pointer is a device pointer; a core only
// enqueues on the stream.  The host-table entries ptam_map_* wrap them between an upload into the context's scratch and a download,
// the resident forms ptam_rmap_* (maprmap.hip) hand them the handle's own buffers.
#pragma once
#include "common.h"

enum { MT_TILE = 1024, MT_SCAN_CHUNK = 1024 };
// what a gate word holds while no refusal has been decided (a memset of 0x7f bytes); a lower value is the offending row
enum { MT_GATE_OPEN = 0x7f7f7f7f };
static inline int mt_tiles(int n) { return (int)(((long long)n + MT_TILE - 1) / MT_TILE); }

// ---- the outlier loop of MapMaker::BundleAdjust (src/MapMaker.cc:916-932)
struct MtOutliersDev {
    int n_meas, n_never, n_outliers;
    int n_never_out;                    // n_never + the list's NEVER_RETRY entries (known from the list)
    const ptam_map_meas* meas;
    const ptam_map_pair* never;
    const ptam_map_outlier* outliers;
    uint8_t* bad;                       // in place
    ptam_map_refind_point* points;      // nullable: the point rows whose `bad` follows the byte
    const int* gate;                    // nullable: flags and bad are written only while *gate == MT_GATE_OPEN
    uint8_t* flag;                      // work: n_meas bytes
    int* tot;                           // work: 3 counts (rows kept, new never pairs, new failure pairs)
    int* tiles;                         // work: mt_tiles(max(n_meas, n_outliers))
    ptam_map_pair* new_never;           // work: n_outliers
    ptam_map_meas* meas_out;            // n_meas
    ptam_map_pair* never_out;           // n_never_out
    ptam_map_pair* failure_new;         // where the new failure pairs go, in list order: n_outliers
};
int mt_apply_outliers_core(hipStream_t st, const MtOutliersDev& d);

// ---- MapMaker::HandleBadPoints (:131-153) with Map::MoveBadPointsToTrash (src/Map.cc:20-30)
enum { MT_T_KEPT = 0, MT_T_MEAS, MT_T_NEVER, MT_T_NEW, MT_T_FAIL, MT_T_MARKED, MT_T_COUNT };
struct MtBadDev {
    int n_points, n_meas, n_never, n_new, n_failure, n_columns;
    const uint8_t* bad;                 // nullable
    const int32_t *outlier_count, *inlier_count;   // nullable together
    const ptam_map_meas* meas;
    const ptam_map_pair* never;
    const int32_t* new_queue;
    const ptam_map_pair* failure;
    uint8_t* removed;                   // work: n_points
    int* tot;                           // work: MT_T_COUNT counts
    int* tiles;                         // work: mt_tiles(the longest table)
    int32_t *new_index, *kept;          // n_points each
    ptam_map_meas* meas_out;
    ptam_map_pair* never_out;
    int32_t* new_out;
    ptam_map_pair* failure_out;
    const void* col_in[PTAM_MAP_MAX_COLUMNS];
    void* col_out[PTAM_MAP_MAX_COLUMNS];
    int col_dwords[PTAM_MAP_MAX_COLUMNS];
};
int mt_handle_bad_points_core(hipStream_t st, const MtBadDev& d);

// ---- the table side of AddPointEpipolar (:670-685) and of InitFromStereo's point loop (:352-362)
struct MtAdd {
    int n_meas, n_made, n_points;
    int a, b;                 // rows of meas before the two insertions: the ends of the lower / the higher keyframe's run;
                              // a < 0: every thread finds both by a binary search in the table
    int kf_lo, kf_hi;         // the two keyframes, ascending
    int src_is_lo, target_source;
    const ptam_map_meas* meas;
    const ptam_new_map_point* made;
    ptam_map_meas* out;
    int src_kf;
    // the new points' rows, each nullable: row i of a column is new point i
    ptam_map_refind_point* points;
    ptam_map_point_source* sources;
    double* points3;
    uint8_t* bad;
    int32_t *outlier_count, *inlier_count;
    int32_t* new_queue;
};
int mt_add_points_core(hipStream_t st, const MtAdd& p);

// ---- MapMaker::ReFind* (:1028-1081), maprefind.hip: ptam_map_refind behind its pointer checks.  Host tables (h_: checked on the host,
//      uploaded, the merged tables come down) or resident ones (d_: valid by the handle's invariant; the merged tables are written
//      into d_meas_merged / d_never_merged, room for n_meas / n_never + the call's pair count, and nothing of them comes down).
struct MrTables {
    int n_kf, n_points, n_meas, n_never;
    const ptam_kf* const* kfs;                  // host, always
    const double* h_poses;
    const ptam_map_refind_point* h_points;
    const ptam_map_meas* h_meas;
    const ptam_map_pair* h_never;
    const double* d_poses;
    const ptam_map_refind_point* d_points;
    const ptam_map_meas* d_meas;
    const ptam_map_pair* d_never;
    ptam_map_meas* d_meas_merged;
    ptam_map_pair* d_never_merged;
    const uint8_t* work_bad;                    // resident NEW_POINTS: bBad of each work entry's point (host)
};
// found_out / found_subpix / never_out may be null with resident tables.  *merged_written (nullable): the merged tables were built
// (not when the call has no pair to visit).  traffic (nullable): bytes this call moved up / down over the host link.
int mr_run(ptam_ctx* ctx, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, const MrTables& t, int n_work, const void* work,
           const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix,
           ptam_map_pair* never_out, int out_cap, ptam_map_meas* meas_merged, ptam_map_pair* never_merged, int* merged_written,
           unsigned long long traffic[2]);

// ---- MapMaker::BundleAdjust (:768-933), mapba.hip: ptam_map_bundle_adjust behind its argument checks.  The tables of one call are
//      on the host (they go up into the scratch, the adjusted poses and points come down) or resident (the d_ pointers; adjusted in
//      place, the poses come down into the mirror).  The O(K) camera marshalling reads h_poses / h_fixed either way.
struct MbaTables {
    int K, N, M;
    const double* h_poses;              // host: the caller's array or the resident map's mirror
    const uint8_t* h_fixed;
    const double* h_points3;            // host tables: null with resident ones
    const ptam_map_meas* h_meas;
    double* d_poses;                    // resident tables: all null with host ones
    const uint8_t* d_fixed;
    double* d_points3;
    const ptam_map_meas* d_meas;
    ptam_map_refind_point* d_points;    // resident, nullable: pv.world follows points3 after an accepted bundle
    double* poses_out;                  // host: where the poses come down after an accepted bundle
    double* points3_out;                // host, nullable: the points
};
// traffic (nullable): the bytes this layer moved up / down over the host link (the bundle's own result words apart)
int mba_run(ptam_ctx* ctx, const ptam_ba_opts* opts, int mode, const MbaTables& t, const volatile unsigned char* abort_flag,
            ptam_map_ba_result* res, ptam_map_outlier* outliers, int32_t* cam_kf, int32_t* point_ids, unsigned long long traffic[2]);
