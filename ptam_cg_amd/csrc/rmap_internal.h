// rmap_internal.h — ptam_rmap, the resident map, as its four files share it: maprmap.hip (the handle, upload / download, the edits,
// the resident forms of bundle, re-find and transform), maprmap_keyframe.hip (a keyframe into the map), maprmap_publish.hip
// (serials, frame reports, the map to the tracker) and maprmap_init.hip (the first map: InitFromStereo, the plane alignment, clear).
// Every table has two buffers of one capacity.  A kernel that rebuilds a table reads buf[cur] and writes buf[cur ^ 1]; the host
// flips cur after the call's wait has read the refusal word.  Rows appended behind a table's count change nothing until the count
// moves, which it does after the same wait.
#pragma once
#include <algorithm>

#include "framereport_internal.h"   // ptam_frame_report: what the map takes from the tracker
#include "maptables_internal.h"

enum { RM_NO_ROW = MT_GATE_OPEN };
// the handle's device words: refusal words (a memset of 0x7f bytes = RM_NO_ROW), then the cores' counts
enum { RM_W_MEAS = 0, RM_W_NEVER, RM_W_NEW, RM_W_FAILURE, RM_W_POINTS, RM_W_CALL, RM_W_ERRS = 8, RM_W_TOT = 8, RM_WORDS = 16 };
static_assert(RM_WORDS * sizeof(int) == PTAM_RMAP_WORD_BYTES, "the word block is what the header says a call brings down");
static_assert(RM_W_TOT + MT_T_COUNT <= RM_WORDS, "the cores' counts fit behind the refusal words");
// ptam_rmap_bundle_adjust_routed: the routed list's outliers per action (POINT_BAD, FAILURE_QUEUE, NEVER_RETRY), behind the three
// counts of mt_apply_outliers_core
enum { RM_W_TALLY = RM_W_TOT + 3 };
static_assert(RM_W_TALLY + 3 <= RM_WORDS, "the tally fits behind the outlier core's counts");

// the tables of ptam_rmap_download, then the serial column: one int64 per point, strictly increasing, the seventh point-side column
enum { RM_SERIALS = PTAM_RMAP_TABLES, RM_TABLES };
static const size_t RM_ROW_BYTES[RM_TABLES] = {96, 1, 24, sizeof(ptam_map_refind_point), sizeof(ptam_map_point_source), 1, 4, 4,
                                               sizeof(ptam_map_meas), sizeof(ptam_map_pair), 4, sizeof(ptam_map_pair), sizeof(long long)};
enum { RM_N_KF = 0, RM_N_POINTS, RM_N_MEAS, RM_N_NEVER, RM_N_NEW, RM_N_FAILURE, RM_N_COUNTS };
static const int RM_COUNT_OF[RM_TABLES] = {RM_N_KF, RM_N_KF, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS,
                                           RM_N_MEAS, RM_N_NEVER, RM_N_NEW, RM_N_FAILURE, RM_N_POINTS};
static inline bool rm_point_side(int w) { return RM_COUNT_OF[w] == RM_N_POINTS; }

struct RmTable {
    char* buf[2] = {nullptr, nullptr};
    size_t cap = 0;   // rows, of both buffers
    int cur = 0;
    char* now() const { return buf[cur]; }
    char* alt() const { return buf[cur ^ 1]; }
};

struct ptam_rmap {
    ptam_ctx* ctx;
    int n[RM_N_COUNTS];
    RmTable t[RM_TABLES];
    long long map_id, next_serial;     // process-wide | the next serial this handle gives out (never reused)
    long long kf_epoch;                // successful uploads: keyframes are appended, or all replaced by an upload (ptam_snapshot_keyframes_enable)
    std::vector<const ptam_kf*> kfs;   // host only
    std::vector<double> h_poses;       // the mirror: K x 12
    std::vector<uint8_t> h_fixed;
    int* d_words;
    unsigned long long h2d, d2h;
    int refusal_table, refusal_row;
    void* d_init;                      // ptam_rmap_init_from_stereo from a host match table: the trails and their matches (grown on demand)
    size_t d_init_bytes;
};

// typed access: rm_meas(m) is the table as it stands, rm_meas_alt(m) the buffer a rebuilding kernel writes
#define RM_TABLE(name, T, w)                                            \
    static inline T* rm_##name(ptam_rmap* m) { return (T*)m->t[w].now(); } \
    static inline T* rm_##name##_alt(ptam_rmap* m) { return (T*)m->t[w].alt(); }
RM_TABLE(poses, double, PTAM_RMAP_KF_POSES)
RM_TABLE(fixed, uint8_t, PTAM_RMAP_KF_FIXED)
RM_TABLE(points3, double, PTAM_RMAP_POINTS3)
RM_TABLE(points, ptam_map_refind_point, PTAM_RMAP_REFIND_POINTS)
RM_TABLE(sources, ptam_map_point_source, PTAM_RMAP_SOURCES)
RM_TABLE(bad, uint8_t, PTAM_RMAP_BAD)
RM_TABLE(outlier_count, int32_t, PTAM_RMAP_OUTLIER_COUNT)
RM_TABLE(inlier_count, int32_t, PTAM_RMAP_INLIER_COUNT)
RM_TABLE(meas, ptam_map_meas, PTAM_RMAP_MEAS)
RM_TABLE(never, ptam_map_pair, PTAM_RMAP_NEVER)
RM_TABLE(new_queue, int32_t, PTAM_RMAP_NEW_QUEUE)
RM_TABLE(failure, ptam_map_pair, PTAM_RMAP_FAILURE)
RM_TABLE(serials, long long, RM_SERIALS)
#undef RM_TABLE

// ---- maprmap.hip: what a call on the handle is made of
// the call's stage: its copies feed the handle's traffic counters
static inline MapStage rm_stage(ptam_rmap* m) { return MapStage(m->ctx, &m->h2d, &m->d2h); }
// table w holds at least `rows` rows in both buffers; growth doubles, keeps the live rows and is the only allocation of a call
int rm_room(ptam_rmap* m, int w, long long rows);
int rm_room_points(ptam_rmap* m, long long rows);   // every point-side table
int rm_words_reset(ptam_rmap* m);                   // the refusal words open, the counts zero
// the call's wait: the words come down with it, into RM_WORDS ints of the stage's pinned block
int rm_words_wait(MapStage& s, ptam_rmap* m, int* h_words);
int rm_refuse(ptam_rmap* m, int table, int row);
// mt_add_points_core on the handle's buffers; d_made: the records in device memory.  One wait, then the counts move.
int rm_add_points_device(ptam_rmap* m, int src_kf, int target_kf, int target_source, int n_made, const ptam_new_map_point* d_made);
// ---- maprmap_keyframe.hip
// steps (d)-(g) of ptam_rmap_insert_keyframe for kSrc = keyframe src_kf (rows [busy_first, busy_first + n_busy) of the measurement
// table are its run) against keyframe target_kf; run: sized by epi_sizes; levels: run.nl entries
struct EpiRun;
int rm_epipolar_points(ptam_rmap* m, int src_kf, const ptam_kf* src, const double src_pose[12], int target_kf, const ptam_epipolar_opts* epi,
                       EpiRun& run, int busy_first, int n_busy, int32_t* n_made, ptam_epipolar_level_stats* levels);
// ---- maprmap_publish.hip
// out[i] = first + i: the serials of points that a call appends (or, at an upload, of all of them)
void rm_give_serials(hipStream_t st, int n, long long first, long long* out);

// what every consumer asks of a frame report, on the host
static inline int rm_report_usable(const ptam_rmap* m, const ptam_frame_report* rep) {
    ARG_TRY(rep && rep->ctx->device == m->ctx->device);
    ARG_TRY(rep->info.n_records > 0 && rep->info.n_records <= rep->max_records);
    ARG_TRY(rep->info.map_id == m->map_id);
    return PTAM_OK;
}

#ifdef __HIPCC__
// the index of `key` in the strictly increasing list s[0..n), or -1
__device__ __forceinline__ int rm_find_serial(const long long* __restrict__ s, int n, long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (s[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && s[lo] == key ? lo : -1;
}
#endif
