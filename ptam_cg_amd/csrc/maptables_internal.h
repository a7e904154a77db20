// maptables_internal.h — the device cores of the map calls: the table edits (mt_*_core, maptables.hip), the re-find (mr_core,
// maprefind.hip) and the bundle (mba_core, mapba.hip); the scene depth and the global transform are declared with the stage
// (map_stage.h).  Every table pointer is a device pointer; what is host by nature (the keyframe handles, the pose / fixed mirror) says
// so.  The host-table entries ptam_map_* check their tables (map_tables_check.h), stage them up into the call's one scratch block
// beside the core's work (a layout function over a Carver, run twice), run the core and stage the results down; the resident forms
// ptam_rmap_* (maprmap*.hip) hand the cores the handle's own buffers.
#pragma once
#include "common.h"
#include "map_stage.h"
#include "map_tables_check.h"
#include "maprefind_plan.h"
#include "refind_internal.h"   // RpDev, RpPair, KfLevels: the re-find core's work

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
// the call's result from the core's counts as they came down
static inline ptam_map_bad_points_result mt_bad_result(const int* counts, int n_points, int n_new) {
    ptam_map_bad_points_result r = {};
    r.n_marked = counts[MT_T_MARKED];
    r.n_kept = counts[MT_T_KEPT];
    r.n_removed = n_points - r.n_kept;
    r.n_meas_out = counts[MT_T_MEAS];
    r.n_never_out = counts[MT_T_NEVER];
    r.n_new_out = counts[MT_T_NEW];
    r.n_new_dropped = n_new - r.n_new_out;
    r.n_failure_out = counts[MT_T_FAIL];
    return r;
}

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
// what the keyframes and the counts decide of an MtAdd; a = b = -1 (the kernel searches) until the caller knows better
static inline MtAdd mt_add_head(int src_kf, int target_kf, int target_source, int n_meas, int n_made, int n_points) {
    MtAdd p = {};
    p.n_meas = n_meas;
    p.n_made = n_made;
    p.n_points = n_points;
    p.a = p.b = -1;
    p.kf_lo = src_kf < target_kf ? src_kf : target_kf;
    p.kf_hi = src_kf < target_kf ? target_kf : src_kf;
    p.src_is_lo = src_kf < target_kf;
    p.src_kf = src_kf;
    p.target_source = target_source;
    return p;
}

// ---- InitFromStereo's point loop (:310-367) behind its kernel: the records whose status is PTAM_INIT_MADE compacted in match order
//      (the ordered compaction, tiles of MT_TILE matches), and how many matches ended in each status.
//      tot: MT_MADE_WORDS ints = {made, count of status 0..3}; tiles: mt_tiles(n); in / out: n records each
enum { MT_MADE_WORDS = 5 };
int mt_made_records_core(hipStream_t st, int n, const int32_t* status, const ptam_new_map_point* in, ptam_new_map_point* out, int* tiles, int* tot);

// ---- the sort of 64-bit keys (maptables.hip): n keys in a, ascending, into a or b (n keys of room each) -> the buffer that holds
//      them.  Only enqueues on st.  Every key must lie below ~0 (a short last tile is filled with it).
unsigned long long* mt_sort_keys(hipStream_t st, int n, unsigned long long* a, unsigned long long* b);

// ---- the work lists of mr_run from the resident queues (maptables.hip); keys_a / keys_b: n 64-bit keys of room each
//      mqNewQueue's entries whose point is not bad, in queue order (the ordered compaction): wpts = the points, wentry = their
//      entries; *total = how many.  tiles: mt_tiles(n_new)
int mt_queue_good_core(hipStream_t st, int n_new, const int32_t* new_queue, const uint8_t* bad, int* wpts, int* wentry, int* tiles, int* total);
//      wrank[i] = the place of wpts[i] among the n_good points in index order (no point twice: the queue's rule)
int mt_queue_rank_core(hipStream_t st, int n_good, const int* wpts, int* wrank, unsigned long long* keys_a, unsigned long long* keys_b);
//      mvFailureQueue sorted by (kf, point), duplicates kept (:1074)
int mt_failure_sorted_core(hipStream_t st, int n_failure, const ptam_map_pair* failure, ptam_map_pair* out, unsigned long long* keys_a,
                           unsigned long long* keys_b);

// ---- MapMaker::ReFind* (:1028-1081), maprefind.hip: the re-find on tables in device memory.  The merged tables are written into
//      d_meas_merged / d_never_merged (each nullable; room for n_meas / n_never + the plan's pair count).
struct MrTables {
    int n_kf, n_points, n_meas, n_never;
    const ptam_kf* const* kfs;                  // host by nature: the level records are read from the handles
    const double* d_poses;
    const ptam_map_refind_point* d_points;
    const ptam_map_meas* d_meas;
    const ptam_map_pair* d_never;
    ptam_map_meas* d_meas_merged;
    ptam_map_pair* d_never_merged;
};
struct MrWork {   // the core's pieces of the call's stage: mr_layout
    KfLevels* Ls;
    int *w0, *w1, *cnt, *slot, *ord_f, *ord_n, *h_cnt;
    ptam_map_meas* found;
    int32_t* subpix;
    ptam_map_pair* nev;
    RpPair* pairs;
    RpDev chain;
};
// what every form of the call asks of its arguments before the plan
int mr_check_call(ptam_ctx* ctx, const ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_kf, const ptam_kf* const* kfs);
void mr_layout(Carver& c, Carver& pin, int n_kf, const MrPlan& plan, bool merged, MrWork& w);   // merged: a merged table is asked for
// what the layout and the passes need of a plan: a host plan's (mr_shape), or that of work lists kernels have built into w.w0 /
// w.w1 (ptam_rmap_refind_queue, which lays out for the queue's length and runs for the count of good points)
struct MrShape {
    int mode, kf0;
    int n_wp;                           // NEW_POINTS: the points that make pairs
    int n_wq;                           // FAILURE_QUEUE: the pairs
    int pairs, per_pass;
};
MrShape mr_shape(const MrPlan& plan);
void mr_layout_shape(Carver& c, Carver& pin, int n_kf, const MrShape& shape, bool merged, MrWork& w);
// shape.pairs > 0; the work lists are in w.w0 / w.w1 (NEW_POINTS: wpts, wrank; FAILURE_QUEUE: the sorted pairs in w.w0).  Uploads
// the level records, runs the passes, orders and merges, waits for the counts and queues the call's lists to come down (found_out /
// found_subpix / never_out nullable together).  points_consumed and n_bad_points are left zero: the owner of the work list knows
// them.  The call's last wait is the caller's, behind whatever else it brings down.
int mr_run(MapStage& s, ptam_refinder* finder, const MrTables& t, const MrShape& shape, const MrWork& w, const volatile unsigned char* stop_flag,
           ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix, ptam_map_pair* never_out);
// plan.pairs > 0.  The work lists of a host plan up, then mr_run, then what the plan says of a stopped queue.
int mr_core(MapStage& s, ptam_refinder* finder, const MrTables& t, const MrPlan& plan, const MrWork& w, const volatile unsigned char* stop_flag,
            ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix, ptam_map_pair* never_out);

// ---- MapMaker::BundleAdjust (:768-933), mapba.hip: the bundle on tables in device memory, adjusted in place.
struct MbaTables {
    int K, N, M;
    const double* h_poses;              // host by nature: the pose / fixed mirror the O(K) camera marshalling reads
    const uint8_t* h_fixed;
    double* d_poses;
    const uint8_t* d_fixed;
    double* d_points3;
    const ptam_map_meas* d_meas;
    ptam_map_refind_point* d_points;    // nullable: pv.world follows points3 after an accepted bundle
};
struct MbaWork {   // the core's pieces of the call's stage: mba_layout
    char* cleared;                      // [header | role | point marks | rows per point], zeroed as one
    size_t clear_bytes;
    int *role, *pt_mark, *pt_rows, *cam_id, *cam_kf, *pt_id, *pt_of, *blk, *sel_row, *ord, *orow, *opt, *first;
    double* pts_sel;
    ptam_map_outlier* out;
    char* h_sel;                        // pinned: the header and the camera list of the selection's wait
};
void mba_layout(Carver& c, Carver& pin, int K, int N, int M, MbaWork& w);
// Selection, its one wait, the camera marshalling, ingest and Compute(), the scatter and the outlier routing.  The outliers and the
// point ids are queued to come down; the call's last wait is the caller's, behind whatever it brings down of the adjusted tables
// (res->accepted > 0).  n_routed (nullable): the routing runs whether or not `outliers` is given, the routed list stays in w.out for
// the launches the caller queues behind it, and *n_routed is its length.
int mba_core(MapStage& s, const ptam_ba_opts* opts, int mode, const MbaTables& t, const MbaWork& w, const volatile unsigned char* abort_flag,
             ptam_map_ba_result* res, ptam_map_outlier* outliers, int32_t* cam_kf, int32_t* point_ids, int* n_routed = nullptr);
