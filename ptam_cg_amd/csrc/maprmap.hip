// maprmap.hip — ptam_rmap, the resident map (ptam_hip.h): the tables of the ptam_map_* calls kept in device memory, and the
// resident forms of the calls of one MapMaker::run() iteration (src/MapMaker.cc:57-114) that edit them:
//   ptam_rmap_upload / download     the whole map up (checked on the device), any row range down
//   ptam_rmap_apply_outliers        ptam_map_apply_outliers      } the cores of maptables.hip on the handle's buffers
//   ptam_rmap_handle_bad_points     ptam_map_handle_bad_points   }
//   ptam_rmap_add_points            ptam_map_add_points          }
//   ptam_rmap_add_keyframe          the table side of AddKeyFrameFromTopOfQueue (:501-506)
//   ptam_rmap_note_tracked          the tracker's iteration set into the two counts (src/Tracker.cc:987-998)
//   ptam_rmap_scene_depth           ptam_map_scene_depth's kernel (mapalign.hip)
//   ptam_rmap_bundle_adjust         mba_run (mapba.hip) on the handle's buffers: adjusted in place, the poses into the mirror
//   ptam_rmap_refind                mr_run (maprefind.hip): the merged tables into the second buffers, the resident queue popped
//   ptam_rmap_apply_global_transform  map_apply_kernel (mapalign.hip): the pixel vectors straight into the point rows
//   ptam_rmap_closest_keyframes     ClosestKeyFrame / NClosestKeyFrames (:711-752): rm_closest_kernel on the resident pose table
//   ptam_rmap_insert_keyframe       AddKeyFrameFromTopOfQueue (:493-518) after MakeKeyFrame_Rest as one call: the keyframe's rows, its
//                                   re-find (mr_run), the closest keyframe, the busy list from the resident measurement table
//                                   (rm_busy_kernel), the epipolar chain of mapmaker.hip, and mt_add_points_core on the chain's output
//   ptam_rmap_publish               the map as the tracker wants it into a ptam_map_snapshot's free slot (rm_publish_kernel): rows, patch
//                                   sources resolved through a per-keyframe level record, serials; the hand-over is snapshot_slots.h;
//                                   with a keyframe section in the snapshot also the pose table and the missing keyframe SBIs (sbi.hip)
//   ptam_rmap_point_serials / resolve_serials   the serial column (one int64 per point, strictly increasing, given by rm_serials_kernel)
//                                   and a binary search in it (rm_resolve_kernel)
//   ptam_rmap_note_reports / insert_keyframe_report   the tracker's frame reports (framereport.hip) into the counts (rm_note_reports_kernel)
//                                   and into a new keyframe's rows (rm_report_rows_kernel): records resolved by serial where they lie
// Every table has two buffers of one capacity.  A kernel that rebuilds a table reads buf[cur] and writes buf[cur ^ 1]; the host
// flips cur after the call's wait has read the refusal word.  Rows appended behind a table's count change nothing until the count
// moves, which it does after the same wait.
// The new kernels check (rm_check_*), append (rm_add_keyframe_kernel) and count (rm_note_tracked_kernel).  Their atomics: atomicMin
// on a refusal word (only a thread that has found an offence issues one), atomicMin on an owner word per point / per row, integer
// atomicAdd on the counts.  Nothing is handed between workgroups inside a launch: an owner word is written by one launch and
// compared by the next.
#include <algorithm>
#include <atomic>

#include "maptables_internal.h"
#include "kf_dist_device.h"       // mba_centre, mba_linear_dist, mba_pair_less, mba_block_least
#include "mapmaker_internal.h"    // EpiBusy, EpiRun, the epipolar chain
#include "refind_internal.h"      // ptam_refinder
#include "snapshot_internal.h"    // ptam_map_snapshot: ptam_rmap_publish fills its free slot
#include "sbi.h"                  // the snapshot's keyframe section: ptam_rmap_publish fills it too
#include "framereport_internal.h" // ptam_frame_report: ptam_rmap_note_reports, ptam_rmap_insert_keyframe_report

namespace {

enum { RM_NO_ROW = MT_GATE_OPEN };
// the handle's device words: refusal words (a memset of 0x7f bytes = RM_NO_ROW), then the cores' counts
enum { RM_W_MEAS = 0, RM_W_NEVER, RM_W_NEW, RM_W_FAILURE, RM_W_POINTS, RM_W_CALL, RM_W_ERRS = 8, RM_W_TOT = 8, RM_WORDS = 16 };
static_assert(RM_WORDS * sizeof(int) == PTAM_RMAP_WORD_BYTES, "the word block is what the header says a call brings down");
static_assert(RM_W_TOT + MT_T_COUNT <= RM_WORDS, "the cores' counts fit behind the refusal words");

const size_t RM_ROW_BYTES[PTAM_RMAP_TABLES] = {96, 1, 24, sizeof(ptam_map_refind_point), sizeof(ptam_map_point_source), 1, 4, 4,
                                               sizeof(ptam_map_meas), sizeof(ptam_map_pair), 4, sizeof(ptam_map_pair)};
enum { RM_N_KF = 0, RM_N_POINTS, RM_N_MEAS, RM_N_NEVER, RM_N_NEW, RM_N_FAILURE, RM_N_COUNTS };
const int RM_COUNT_OF[PTAM_RMAP_TABLES] = {RM_N_KF, RM_N_KF, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS, RM_N_POINTS,
                                           RM_N_MEAS, RM_N_NEVER, RM_N_NEW, RM_N_FAILURE};

struct RmTable {
    char* buf[2] = {nullptr, nullptr};
    size_t cap = 0;   // rows, of both buffers
    int cur = 0;
    char* now() const { return buf[cur]; }
    char* alt() const { return buf[cur ^ 1]; }
};

}   // namespace

struct ptam_rmap {
    ptam_ctx* ctx;
    int n[RM_N_COUNTS];
    RmTable t[PTAM_RMAP_TABLES];
    RmTable serial;                    // the seventh point-side column: one int64 per point, strictly increasing; no table of download
    long long map_id, next_serial;     // process-wide | the next serial this handle gives out (never reused)
    long long kf_epoch;                // successful uploads: keyframes are appended, or all replaced by an upload (ptam_snapshot_keyframes_enable)
    std::vector<const ptam_kf*> kfs;   // host only
    std::vector<double> h_poses;       // the mirror: K x 12
    std::vector<uint8_t> h_fixed;
    int* d_words;
    unsigned long long h2d, d2h;
    int refusal_table, refusal_row;
};

namespace {

__device__ __forceinline__ unsigned long long rm_key(int kf, int point) { return ((unsigned long long)(unsigned)kf << 32) | (unsigned)point; }
__device__ __forceinline__ void rm_offend(int* err, int row) { atomicMin(err, row); }

// one thread per row of a sorted table: the ranges, and the row against its predecessor (strictly ascending by (kf, point))
template <class Row, bool MEAS>
__global__ void __launch_bounds__(256) rm_check_sorted_kernel(int n, const Row* __restrict__ t, int n_kf, int n_points, int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Row r = t[i];
    bool off = r.kf < 0 || r.kf >= n_kf || r.point < 0 || r.point >= n_points;
    if constexpr (MEAS) off = off || r.level < 0 || r.level >= PTAM_LEVELS || r.source < PTAM_MAP_SRC_TRACKER || r.source > PTAM_MAP_SRC_EPIPOLAR;
    if (i > 0 && !off) {
        const int pk = t[i - 1].kf, pp = t[i - 1].point;
        off = rm_key(pk, pp) >= rm_key(r.kf, r.point);   // (an out-of-range predecessor offends at its own, lower row)
    }
    if (off) rm_offend(err, i);
}
// mvFailureQueue: any order, duplicates allowed, indices in range
__global__ void __launch_bounds__(256) rm_check_pairs_kernel(int n, const ptam_map_pair* __restrict__ t, int n_kf, int n_points, int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ptam_map_pair r = t[i];
    if (r.kf < 0 || r.kf >= n_kf || r.point < 0 || r.point >= n_points) rm_offend(err, i);
}
// mqNewQueue: in range; owner[point] = the lowest entry that names the point (owner: 0xff bytes before the launch)
__global__ void __launch_bounds__(256) rm_queue_owner_kernel(int n, const int32_t* __restrict__ q, int n_points, unsigned* __restrict__ owner,
                                                              int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = q[i];
    if (p < 0 || p >= n_points) rm_offend(err, i);
    else atomicMin(owner + p, (unsigned)i);
}
// ... and, in the next launch: an entry that is not its point's owner repeats a lower one
__global__ void __launch_bounds__(256) rm_queue_repeat_kernel(int n, const int32_t* __restrict__ q, int n_points, const unsigned* __restrict__ owner,
                                                               int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = q[i];
    if (p >= 0 && p < n_points && owner[p] != (unsigned)i) rm_offend(err, i);
}
// the redundant columns of the point side, bit for bit, and the patch source's range
__global__ void __launch_bounds__(256) rm_check_points_kernel(int n, const double* __restrict__ points3, const ptam_map_refind_point* __restrict__ pts,
                                                               const ptam_map_point_source* __restrict__ src, const uint8_t* __restrict__ bad, int n_kf,
                                                               int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ptam_map_refind_point& p = pts[i];
    bool off = p.src_kf < 0 || p.src_kf >= n_kf || p.src_kf != src[i].src_kf || p.bad != (int)bad[i] || p.src_level < 0 || p.src_level >= PTAM_LEVELS;
    for (int j = 0; j < 3; j++) off = off || __double_as_longlong(p.pv.world[j]) != __double_as_longlong(points3[(size_t)3 * i + j]);
    if (off) rm_offend(err, i);
}

// ptam_rmap_apply_outliers, before the flag kernel, one thread per outlier (o.meas is inside the table: checked on the host):
// the outlier names its row; the row's owner; a NEVER_RETRY pair is not in never
__global__ void __launch_bounds__(256) rm_outliers_check_kernel(int n, const ptam_map_outlier* __restrict__ o, const ptam_map_meas* __restrict__ meas,
                                                                 int n_never, const ptam_map_pair* __restrict__ never, unsigned* __restrict__ owner,
                                                                 int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ptam_map_outlier r = o[i];
    bool off = meas[r.meas].kf != r.kf || meas[r.meas].point != r.point;
    atomicMin(owner + r.meas, (unsigned)i);
    if (!off && r.action == PTAM_MAP_OUT_NEVER_RETRY) {
        const unsigned long long key = rm_key(r.kf, r.point);
        int lo = 0, hi = n_never;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (rm_key(never[mid].kf, never[mid].point) < key) lo = mid + 1;
            else hi = mid;
        }
        off = lo < n_never && rm_key(never[lo].kf, never[lo].point) == key;   // :947-948: no pair is in both sets
    }
    if (off) rm_offend(err, i);
}
// ... and, in the next launch: an outlier that is not its row's owner names a row that a lower one names
__global__ void __launch_bounds__(256) rm_outliers_twice_kernel(int n, const ptam_map_outlier* __restrict__ o, const unsigned* __restrict__ owner,
                                                                 int* __restrict__ err) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (owner[o[i].meas] != (unsigned)i) rm_offend(err, i);
}

// :501-506, one thread per measurement of the new keyframe: its run, appended behind the table's last row
__global__ void __launch_bounds__(256) rm_add_keyframe_kernel(int n, const ptam_map_kf_row* __restrict__ rows, int kf, ptam_map_meas* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ptam_map_kf_row r = rows[i];
    ptam_map_meas m;
    m.kf = kf;
    m.point = r.point;
    m.level = r.level;
    m.source = PTAM_MAP_SRC_TRACKER;
    m.root_pos[0] = r.root_pos[0];
    m.root_pos[1] = r.root_pos[1];
    out[i] = m;
}

// NEW_POINTS from the resident queue: bBad of each entry's point, for the host's walk of :1056-1059
__global__ void __launch_bounds__(256) rm_queue_bad_kernel(int n, const int32_t* __restrict__ q, const uint8_t* __restrict__ bad, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = bad[q[i]];
}
// the point rows' pixel vectors into a packed table, for the caller that asked for them
__global__ void __launch_bounds__(256) rm_pack_pvs_kernel(int n, const ptam_map_refind_point* __restrict__ rows, ptam_pvs_point* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rows[i].pv;
}

// src/Tracker.cc:987-998, one thread per entry of the iteration set
__global__ void __launch_bounds__(256) rm_note_tracked_kernel(int n, const int32_t* __restrict__ points, const uint8_t* __restrict__ outlier,
                                                               int32_t* __restrict__ outlier_count, int32_t* __restrict__ inlier_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicAdd((outlier[i] ? outlier_count : inlier_count) + points[i], 1);
}

// ClosestKeyFrame / NClosestKeyFrames (:711-752), ONE WORKGROUP: the n_pick keyframes other than `self` that come first by
// (KeyFrameLinearDist(self, k), k) — a strictly lower distance wins, equal distances go to the lower index (the `<` of :745,
// partial_sort on the pairs of :716-722).  The order is total, so pass r takes the least pair above pass r - 1's: no list of the
// taken ones.  only >= 0: keyframe `only` is the one candidate (its distance is what is asked for).
// out: {count, pad}, n_pick distances, n_pick indices
__global__ void __launch_bounds__(1024) rm_closest_kernel(int K, const double* __restrict__ pose, int self, int only, int n_pick, int* __restrict__ hdr,
                                                          double* __restrict__ out_d, int32_t* __restrict__ out_k) {
    __shared__ double s_d[16], s_pd;
    __shared__ int s_k[16], s_pk;
    const int tid = threadIdx.x;
    double c0[3];
    mba_centre(pose + (size_t)12 * self, c0);
    double pd = 0.0;
    int pk = -1, r = 0;
    for (; r < n_pick; r++) {
        double bd = 0.0;
        int bk = -1;
        for (int k = tid; k < K; k += 1024) {
            if (k == self || (only >= 0 && k != only)) continue;
            const double d = mba_linear_dist(c0, pose + (size_t)12 * k);
            if (pk >= 0 && !mba_pair_less(pd, pk, d, k)) continue;   // taken by an earlier pass
            if (bk < 0 || mba_pair_less(d, k, bd, bk)) bd = d, bk = k;
        }
        mba_block_least(bd, bk, s_d, s_k);
        if (tid == 0) {
            s_pd = bd, s_pk = bk;
            if (bk >= 0) out_d[r] = bd, out_k[r] = bk;
        }
        __syncthreads();
        pd = s_pd, pk = s_pk;
        __syncthreads();   // (s_pd / s_pk are rewritten by the next pass)
        if (pk < 0) break;   // (uniform: nothing left, which only distances that are not numbers bring about)
    }
    if (tid == 0) hdr[0] = r, hdr[1] = 0;
}

// kSrc.mMeasurements as ThinCandidates sees them (:415-441), one thread per row of the new keyframe's run in the resident
// measurement table: the busy list of the epipolar chain (mapmaker.hip) and its count
__global__ void __launch_bounds__(256) rm_busy_kernel(int n, const ptam_map_meas* __restrict__ run, EpiBusy* __restrict__ busy, int* __restrict__ hdr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) hdr[0] = n;
    if (i >= n) return;
    const ptam_map_meas m = run[i];
    EpiBusy b;
    b.x = m.root_pos[0];
    b.y = m.root_pos[1];
    b.level = m.level;
    b.pad_ = 0;
    busy[i] = b;
}

// the next serials of the handle, one thread per new point
__global__ void __launch_bounds__(256) rm_serials_kernel(int n, long long first, long long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = first + i;
}
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
// ptam_rmap_resolve_serials, one thread per entry: the serial's current point index, -1 and a count for one that is gone
__global__ void __launch_bounds__(256) rm_resolve_kernel(int n, const long long* __restrict__ keys, int n_points, const long long* __restrict__ serials,
                                                          int32_t* __restrict__ index_out, int* __restrict__ n_gone) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int at = rm_find_serial(serials, n_points, keys[i]);
    index_out[i] = at;
    if (at < 0) atomicAdd(n_gone, 1);
}
// where a report's records lie, as ptam_rmap_note_reports sends it up
struct RmReportRef {
    const ptam_frame_record* rec;
    int n, pad_;
};
static_assert(sizeof(RmReportRef) == 16, "what ptam_hip.h says a report costs the call");
// src/Tracker.cc:987-998 from frame reports, one thread per record, a row of workgroups per report (blockIdx.y): the record's serial
// resolved as rm_resolve_kernel does, a live point's count bumped as rm_note_tracked_kernel does
__global__ void __launch_bounds__(256) rm_note_reports_kernel(const RmReportRef* __restrict__ reports, int n_points, const long long* __restrict__ serials,
                                                               int32_t* __restrict__ outlier_count, int32_t* __restrict__ inlier_count,
                                                               int* __restrict__ n_gone) {
    const RmReportRef r = reports[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.n) return;
    const ptam_frame_record rec = r.rec[i];
    const int at = rm_find_serial(serials, n_points, rec.serial);
    if (at < 0) atomicAdd(n_gone, 1);
    else atomicAdd((rec.outlier ? outlier_count : inlier_count) + at, 1);
}
// :501-506 from a frame report, ONE WORKGROUP: every record's serial resolved, the live ones appended in order behind the table's
// last row (tiles of 1024 records, the count of live records carried from tile to tile: no atomic decides where a row lands).
// The records ascend by serial and so do the points: the run is sorted and unique.  tot: {rows written, records gone}
__global__ void __launch_bounds__(1024) rm_report_rows_kernel(int n, const ptam_frame_record* __restrict__ rec, int n_points,
                                                               const long long* __restrict__ serials, int kf, ptam_map_meas* __restrict__ out,
                                                               int* __restrict__ tot) {
    __shared__ int ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        ptam_frame_record r;
        int at = -1;
        if (i < n) {
            r = rec[i];
            at = rm_find_serial(serials, n_points, r.serial);
        }
        const bool keep = at >= 0;
        const unsigned long long mk = __ballot(keep);
        if (lane == 0) ws[wid] = __popcll(mk);
        __syncthreads();
        int off = __popcll(mk & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wid) off += ws[w];
            total += ws[w];
        }
        if (keep) {
            ptam_map_meas m;
            m.kf = kf;
            m.point = at;
            m.level = r.level;
            m.source = PTAM_MAP_SRC_TRACKER;
            m.root_pos[0] = r.root_pos[0];
            m.root_pos[1] = r.root_pos[1];
            out[run + off] = m;
        }
        run += total;
        __syncthreads();   // (the wave counts are rewritten by the next tile)
    }
    if (tid == 0) tot[0] = run, tot[1] = n - run;
}
// a keyframe as ptam_rmap_publish sends it up: the four level images
struct RmKfRecord {
    const uint8_t* im[PTAM_LEVELS];
    int w[PTAM_LEVELS], h[PTAM_LEVELS];
};
static_assert(sizeof(RmKfRecord) == 64 && sizeof(RmKfRecord) <= PTAM_RMAP_KF_RECORD_BYTES, "the record ptam_hip.h describes");
// ptam_rmap_publish, one thread per point: the tracker's row, its patch source resolved to the level image, its serial
// (src_kf and src_level are in range by the handle's invariant: rm_check_points_kernel, mt_add_points_core)
__global__ void __launch_bounds__(256) rm_publish_kernel(int n, const ptam_map_refind_point* __restrict__ rows, const long long* __restrict__ serials,
                                                          const RmKfRecord* __restrict__ kfs, ptam_pvs_point* __restrict__ pts, TmSrc* __restrict__ src,
                                                          long long* __restrict__ serials_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ptam_map_refind_point r = rows[i];
    const RmKfRecord& k = kfs[r.src_kf];
    TmSrc s;
    s.im = k.im[r.src_level];
    s.w = k.w[r.src_level];
    s.h = k.h[r.src_level];
    s.cx = r.center_x;
    s.cy = r.center_y;
    pts[i] = r.pv;
    src[i] = s;
    serials_out[i] = serials[i];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline size_t rm_up256(size_t b) { return (b + 255) & ~(size_t)255; }
struct RmCarve {   // offsets into the context's scratch
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += rm_up256(bytes > 0 ? bytes : 1);
        return at;
    }
};
inline unsigned rm_blocks(long long n) { return (unsigned)((n + 255) / 256); }

int rm_up(ptam_rmap* m, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return PTAM_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->ctx->stream));
    m->h2d += bytes;
    return PTAM_OK;
}
int rm_down(ptam_rmap* m, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return PTAM_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, m->ctx->stream));
    m->d2h += bytes;
    return PTAM_OK;
}

// table w holds at least `rows` rows in both buffers; growth doubles, keeps the live rows and is the only allocation of a call
int rm_room_of(ptam_rmap* m, RmTable& t, int w, size_t row_bytes, int live_rows, long long rows) {
    if ((size_t)rows <= t.cap) return PTAM_OK;
    ARG_TRY(rows < (1ll << 31));
    const size_t cap = std::max(std::max((size_t)rows, 2 * t.cap), (size_t)64);
    char* nb[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++)
        if (hipMalloc((void**)&nb[k], cap * row_bytes) != hipSuccess) {
            if (nb[0]) (void)hipFree(nb[0]);
            ptam_set_error("ptam_rmap: no device memory for %zu rows of table %d", cap, w);
            return PTAM_E_HIP;
        }
    hipStream_t st = m->ctx->stream;
    const size_t live = (size_t)live_rows * row_bytes;
    hipError_t e = live > 0 ? hipMemcpyAsync(nb[t.cur], t.now(), live, hipMemcpyDeviceToDevice, st) : hipSuccess;
    if (e == hipSuccess) e = ptam_stream_wait(st);   // (nothing queued reads the old buffers any more)
    if (e != hipSuccess) {
        (void)hipFree(nb[0]);
        (void)hipFree(nb[1]);
        ptam_set_error("ptam_rmap: growing table %d failed: %s", w, hipGetErrorString(e));
        return PTAM_E_HIP;
    }
    for (int k = 0; k < 2; k++)
        if (t.buf[k]) HIP_TRY(hipFree(t.buf[k]));
    t.buf[0] = nb[0];
    t.buf[1] = nb[1];
    t.cap = cap;
    return PTAM_OK;
}
int rm_room(ptam_rmap* m, int w, long long rows) { return rm_room_of(m, m->t[w], w, RM_ROW_BYTES[w], m->n[RM_COUNT_OF[w]], rows); }
enum { RM_SERIAL_COLUMN = PTAM_RMAP_TABLES + 1 };   // (what a failed growth of the serial column calls it)
int rm_room_serials(ptam_rmap* m, long long rows) { return rm_room_of(m, m->serial, RM_SERIAL_COLUMN, sizeof(long long), m->n[RM_N_POINTS], rows); }
int rm_room_points(ptam_rmap* m, long long rows) {
    for (int w = PTAM_RMAP_POINTS3; w <= PTAM_RMAP_INLIER_COUNT; w++)
        if (int rc = rm_room(m, w, rows)) return rc;
    return rm_room_serials(m, rows);
}

// out[i] = first + i: the serials of points that a call appends (or, at an upload, of all of them)
void rm_give_serials(hipStream_t st, int n, long long first, long long* out) {
    if (n > 0) hipLaunchKernelGGL(rm_serials_kernel, dim3(rm_blocks(n)), dim3(256), 0, st, n, first, out);
}

// the refusal words open, the counts zero
int rm_words_reset(ptam_rmap* m) {
    HIP_TRY(hipMemsetAsync(m->d_words, 0x7f, RM_W_ERRS * sizeof(int), m->ctx->stream));
    HIP_TRY(hipMemsetAsync(m->d_words + RM_W_TOT, 0, (RM_WORDS - RM_W_TOT) * sizeof(int), m->ctx->stream));
    return PTAM_OK;
}
// the call's wait: the words come down with it
int rm_words_wait(ptam_rmap* m, const int** words) {
    void* hp;
    if (int rc = ctx_pinned(m->ctx, 256, &hp)) return rc;
    if (int rc = rm_down(m, hp, m->d_words, RM_WORDS * sizeof(int))) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    *words = (const int*)hp;
    return PTAM_OK;
}
int rm_refuse(ptam_rmap* m, int table, int row) {
    m->refusal_table = table;
    m->refusal_row = row;
    ptam_set_error("bad argument: ptam_rmap table %d, row %d (found on the device)", table, row);
    return PTAM_E_ARG;
}

template <class T>
T* rm_now(ptam_rmap* m, int w) { return (T*)m->t[w].now(); }
template <class T>
T* rm_alt(ptam_rmap* m, int w) { return (T*)m->t[w].alt(); }

// a new keyframe's measurement list, checked where it is: sorted by point, none repeated, in range
int rm_check_kf_rows(int n_points, int n_rows, const ptam_map_kf_row* rows) {
    for (int i = 0; i < n_rows; i++) {
        ARG_TRY(rows[i].point >= 0 && rows[i].point < n_points && rows[i].level >= 0 && rows[i].level < PTAM_LEVELS);
        ARG_TRY(i == 0 || rows[i - 1].point < rows[i].point);
    }
    return PTAM_OK;
}
// :501-506 enqueued: the pose and the flag behind the keyframe tables' counts, the rows behind the measurement table's
int rm_add_keyframe_enqueue(ptam_rmap* m, const double pose12[12], const uint8_t* fx, int n_rows, const ptam_map_kf_row* rows) {
    const int K = m->n[RM_N_KF], M = m->n[RM_N_MEAS];
    if (int rc = rm_room(m, PTAM_RMAP_KF_POSES, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_KF_FIXED, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)M + n_rows)) return rc;
    void* sc;
    if (int rc = ctx_scratch(m->ctx, rm_up256((size_t)n_rows * sizeof(ptam_map_kf_row)) + 256, &sc)) return rc;
    if (int rc = rm_up(m, rm_now<double>(m, PTAM_RMAP_KF_POSES) + (size_t)12 * K, pose12, 96)) return rc;
    if (int rc = rm_up(m, rm_now<uint8_t>(m, PTAM_RMAP_KF_FIXED) + K, fx, 1)) return rc;
    if (n_rows > 0) {
        if (int rc = rm_up(m, sc, rows, (size_t)n_rows * sizeof(ptam_map_kf_row))) return rc;
        hipLaunchKernelGGL(rm_add_keyframe_kernel, dim3(rm_blocks(n_rows)), dim3(256), 0, m->ctx->stream, n_rows, (const ptam_map_kf_row*)sc, K,
                           rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS) + M);
        HIP_TRY(hipGetLastError());
    }
    return PTAM_OK;
}
// the same from a frame report: room for every record, the live ones appended by the device; their count comes down in a wait
int rm_add_keyframe_enqueue_report(ptam_rmap* m, const double pose12[12], const uint8_t* fx, const ptam_frame_report* rep, int* n_rows) {
    const int K = m->n[RM_N_KF], M = m->n[RM_N_MEAS], R = rep->info.n_records;
    if (int rc = rm_room(m, PTAM_RMAP_KF_POSES, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_KF_FIXED, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)M + R)) return rc;
    if (int rc = rm_up(m, rm_now<double>(m, PTAM_RMAP_KF_POSES) + (size_t)12 * K, pose12, 96)) return rc;
    if (int rc = rm_up(m, rm_now<uint8_t>(m, PTAM_RMAP_KF_FIXED) + K, fx, 1)) return rc;
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_report_rows_kernel, dim3(1), dim3(1024), 0, m->ctx->stream, R, (const ptam_frame_record*)rep->rec, m->n[RM_N_POINTS],
                       (const long long*)m->serial.now(), K, rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS) + M, m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    const int live = hw[RM_W_TOT];
    if (live < 0 || live > R) {
        ptam_set_error("ptam_rmap_insert_keyframe_report: %d rows from %d records", live, R);
        return PTAM_E_STATE;
    }
    *n_rows = live;
    return PTAM_OK;
}
// ... and the counts moved: the keyframe is the map's
void rm_add_keyframe_commit(ptam_rmap* m, const ptam_kf* kf, const double pose12[12], uint8_t fx, int n_rows) {
    m->kfs.push_back(kf);
    m->h_poses.insert(m->h_poses.end(), pose12, pose12 + 12);
    m->h_fixed.push_back(fx);
    m->n[RM_N_KF] += 1;
    m->n[RM_N_MEAS] += n_rows;
}

// rm_closest_kernel on the first K rows of the pose table and its result down: 8 + 12 n_pick bytes, one wait.  -> the pinned words
// {count, pad}, n_pick distances, n_pick indices
int rm_closest(ptam_rmap* m, int K, int self, int only, int n_pick, const int** hdr, const double** dist, const int32_t** idx) {
    const size_t bytes = 8 + (size_t)12 * n_pick;
    void *sc, *hp;
    if (int rc = ctx_scratch(m->ctx, bytes, &sc)) return rc;
    if (int rc = ctx_pinned(m->ctx, bytes, &hp)) return rc;
    char* b = (char*)sc;
    hipLaunchKernelGGL(rm_closest_kernel, dim3(1), dim3(1024), 0, m->ctx->stream, K, (const double*)rm_now<double>(m, PTAM_RMAP_KF_POSES), self, only,
                       n_pick, (int*)b, (double*)(b + 8), (int32_t*)(b + 8 + (size_t)8 * n_pick));
    HIP_TRY(hipGetLastError());
    if (int rc = rm_down(m, hp, sc, bytes)) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    *hdr = (const int*)hp;
    *dist = (const double*)((const char*)hp + 8);
    *idx = (const int32_t*)((const char*)hp + 8 + (size_t)8 * n_pick);
    return PTAM_OK;
}


// mt_add_points_core on the handle's buffers; d_made: the records in device memory.  One wait, then the counts move.
int rm_add_points_device(ptam_rmap* m, int src_kf, int target_kf, int target_source, int n_made, const ptam_new_map_point* d_made) {
    const int N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], Q = m->n[RM_N_NEW];
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)M + 2ll * n_made)) return rc;
    if (int rc = rm_room_points(m, (long long)N + n_made)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEW_QUEUE, (long long)Q + n_made)) return rc;
    MtAdd p = {};
    p.n_meas = M;
    p.n_made = n_made;
    p.n_points = N;
    p.a = p.b = -1;   // found in the resident table by the kernel
    p.kf_lo = std::min(src_kf, target_kf);
    p.kf_hi = std::max(src_kf, target_kf);
    p.src_is_lo = src_kf < target_kf;
    p.src_kf = src_kf;
    p.target_source = target_source;
    p.meas = rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    p.made = d_made;
    p.out = rm_alt<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    // the point side: behind the counts
    p.points = rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS) + N;
    p.sources = rm_now<ptam_map_point_source>(m, PTAM_RMAP_SOURCES) + N;
    p.points3 = rm_now<double>(m, PTAM_RMAP_POINTS3) + (size_t)3 * N;
    p.bad = rm_now<uint8_t>(m, PTAM_RMAP_BAD) + N;
    p.outlier_count = rm_now<int32_t>(m, PTAM_RMAP_OUTLIER_COUNT) + N;
    p.inlier_count = rm_now<int32_t>(m, PTAM_RMAP_INLIER_COUNT) + N;
    p.new_queue = rm_now<int32_t>(m, PTAM_RMAP_NEW_QUEUE) + Q;
    if (int rc = mt_add_points_core(m->ctx->stream, p)) return rc;
    rm_give_serials(m->ctx->stream, n_made, m->next_serial, (long long*)m->serial.now() + N);   // behind the count, like the other rows
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    m->next_serial += n_made;
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->n[RM_N_MEAS] = M + 2 * n_made;
    m->n[RM_N_POINTS] = N + n_made;
    m->n[RM_N_NEW] = Q + n_made;
    return PTAM_OK;
}

}   // namespace

extern "C" {

int ptam_rmap_create(ptam_ctx* ctx, ptam_rmap** out) {
    ARG_TRY(ctx && out);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_rmap* m = new ptam_rmap();
    m->ctx = ctx;
    for (int i = 0; i < RM_N_COUNTS; i++) m->n[i] = 0;
    m->d_words = nullptr;
    m->h2d = m->d2h = 0;
    m->refusal_table = m->refusal_row = -1;
    static std::atomic<long long> map_ids{0};
    m->map_id = ++map_ids;
    m->next_serial = 1;
    m->kf_epoch = 0;
    if (hipMalloc((void**)&m->d_words, RM_WORDS * sizeof(int)) != hipSuccess) {
        delete m;
        ptam_set_error("ptam_rmap_create: no device memory");
        return PTAM_E_HIP;
    }
    *out = m;
    return PTAM_OK;
}

int ptam_rmap_destroy(ptam_rmap* m) {
    if (!m) return PTAM_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)ptam_stream_wait(m->ctx->stream);
    for (int w = 0; w < PTAM_RMAP_TABLES; w++)
        for (int k = 0; k < 2; k++)
            if (m->t[w].buf[k]) (void)hipFree(m->t[w].buf[k]);
    for (int k = 0; k < 2; k++)
        if (m->serial.buf[k]) (void)hipFree(m->serial.buf[k]);
    if (m->d_words) (void)hipFree(m->d_words);
    delete m;
    return PTAM_OK;
}

int ptam_rmap_reserve(ptam_rmap* m, int n_kf, int n_points, int n_meas, int n_never, int n_new, int n_failure) {
    ARG_TRY(m);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_new >= 0 && n_failure >= 0);
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int rows[RM_N_COUNTS] = {n_kf, n_points, n_meas, n_never, n_new, n_failure};
    for (int w = 0; w < PTAM_RMAP_TABLES; w++)
        if (int rc = rm_room(m, w, rows[RM_COUNT_OF[w]])) return rc;
    return rm_room_serials(m, n_points);
}

int ptam_rmap_counts(const ptam_rmap* m, ptam_rmap_counts_t* out) {
    ARG_TRY(m && out);
    out->n_kf = m->n[RM_N_KF];
    out->n_points = m->n[RM_N_POINTS];
    out->n_meas = m->n[RM_N_MEAS];
    out->n_never = m->n[RM_N_NEVER];
    out->n_new = m->n[RM_N_NEW];
    out->n_failure = m->n[RM_N_FAILURE];
    return PTAM_OK;
}

int ptam_rmap_last_refusal(const ptam_rmap* m, int* table, int* row) {
    ARG_TRY(m && table && row);
    *table = m->refusal_table;
    *row = m->refusal_row;
    return PTAM_OK;
}

int ptam_rmap_traffic(const ptam_rmap* m, unsigned long long* h2d_bytes, unsigned long long* d2h_bytes) {
    ARG_TRY(m && h2d_bytes && d2h_bytes);
    *h2d_bytes = m->h2d;
    *d2h_bytes = m->d2h;
    return PTAM_OK;
}

int ptam_rmap_upload(ptam_rmap* m, int n_kf, const ptam_kf* const* kfs, const double* kf_poses12, const uint8_t* kf_fixed, int n_points,
                     const double* points3, const ptam_map_refind_point* points, const ptam_map_point_source* sources, const uint8_t* bad,
                     const int32_t* outlier_count, const int32_t* inlier_count, int n_meas, const ptam_map_meas* meas, int n_never,
                     const ptam_map_pair* never, int n_new, const int32_t* new_queue, int n_failure, const ptam_map_pair* failure) {
    ARG_TRY(m);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_new >= 0 && n_failure >= 0);
    ARG_TRY((n_kf == 0 || (kf_poses12 && kf_fixed)) && (n_points == 0 || (points3 && points && sources && bad)));
    ARG_TRY((outlier_count != nullptr) == (inlier_count != nullptr));
    ARG_TRY((n_meas == 0 || meas) && (n_never == 0 || never) && (n_new == 0 || new_queue) && (n_failure == 0 || failure));
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int rows[RM_N_COUNTS] = {n_kf, n_points, n_meas, n_never, n_new, n_failure};
    for (int w = 0; w < PTAM_RMAP_TABLES; w++)
        if (int rc = rm_room(m, w, rows[RM_COUNT_OF[w]])) return rc;
    if (int rc = rm_room_serials(m, n_points)) return rc;
    const size_t Nz = (size_t)n_points;
    void* sc;
    if (int rc = ctx_scratch(m->ctx, rm_up256(Nz * sizeof(unsigned)) + 256, &sc)) return rc;
    unsigned* owner = (unsigned*)sc;
    hipStream_t st = m->ctx->stream;

    // ---- up, into the second buffers
    const void* src[PTAM_RMAP_TABLES] = {kf_poses12, kf_fixed, points3, points, sources, bad, outlier_count, inlier_count, meas, never, new_queue, failure};
    for (int w = 0; w < PTAM_RMAP_TABLES; w++) {
        const size_t bytes = (size_t)rows[RM_COUNT_OF[w]] * RM_ROW_BYTES[w];
        if (src[w]) {
            if (int rc = rm_up(m, m->t[w].alt(), src[w], bytes)) return rc;
        } else if (bytes > 0)
            HIP_TRY(hipMemsetAsync(m->t[w].alt(), 0, bytes, st));   // (the counts, when none are given)
    }
    rm_give_serials(st, n_points, m->next_serial, (long long*)m->serial.alt());   // every point a fresh serial: a new map to every tracker
    // ---- the checks, one thread per row
    if (int rc = rm_words_reset(m)) return rc;
    int* err = m->d_words;
    if (n_meas > 0)
        hipLaunchKernelGGL((rm_check_sorted_kernel<ptam_map_meas, true>), dim3(rm_blocks(n_meas)), dim3(256), 0, st, n_meas,
                           (const ptam_map_meas*)rm_alt<ptam_map_meas>(m, PTAM_RMAP_MEAS), n_kf, n_points, err + RM_W_MEAS);
    if (n_never > 0)
        hipLaunchKernelGGL((rm_check_sorted_kernel<ptam_map_pair, false>), dim3(rm_blocks(n_never)), dim3(256), 0, st, n_never,
                           (const ptam_map_pair*)rm_alt<ptam_map_pair>(m, PTAM_RMAP_NEVER), n_kf, n_points, err + RM_W_NEVER);
    if (n_failure > 0)
        hipLaunchKernelGGL(rm_check_pairs_kernel, dim3(rm_blocks(n_failure)), dim3(256), 0, st, n_failure,
                           (const ptam_map_pair*)rm_alt<ptam_map_pair>(m, PTAM_RMAP_FAILURE), n_kf, n_points, err + RM_W_FAILURE);
    if (n_new > 0) {
        HIP_TRY(hipMemsetAsync(owner, 0xff, Nz * sizeof(unsigned) > 0 ? Nz * sizeof(unsigned) : 4, st));
        const int32_t* q = rm_alt<int32_t>(m, PTAM_RMAP_NEW_QUEUE);
        hipLaunchKernelGGL(rm_queue_owner_kernel, dim3(rm_blocks(n_new)), dim3(256), 0, st, n_new, q, n_points, owner, err + RM_W_NEW);
        hipLaunchKernelGGL(rm_queue_repeat_kernel, dim3(rm_blocks(n_new)), dim3(256), 0, st, n_new, q, n_points, (const unsigned*)owner, err + RM_W_NEW);
    }
    if (n_points > 0)
        hipLaunchKernelGGL(rm_check_points_kernel, dim3(rm_blocks(n_points)), dim3(256), 0, st, n_points,
                           (const double*)rm_alt<double>(m, PTAM_RMAP_POINTS3),
                           (const ptam_map_refind_point*)rm_alt<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS),
                           (const ptam_map_point_source*)rm_alt<ptam_map_point_source>(m, PTAM_RMAP_SOURCES),
                           (const uint8_t*)rm_alt<uint8_t>(m, PTAM_RMAP_BAD), n_kf, err + RM_W_POINTS);
    HIP_TRY(hipGetLastError());
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    const int order[5][2] = {{RM_W_MEAS, PTAM_RMAP_MEAS}, {RM_W_NEVER, PTAM_RMAP_NEVER}, {RM_W_NEW, PTAM_RMAP_NEW_QUEUE},
                             {RM_W_FAILURE, PTAM_RMAP_FAILURE}, {RM_W_POINTS, PTAM_RMAP_REFIND_POINTS}};
    for (const auto& o : order)
        if (hw[o[0]] != RM_NO_ROW) return rm_refuse(m, o[1], hw[o[0]]);
    // ---- commit
    for (int w = 0; w < PTAM_RMAP_TABLES; w++) m->t[w].cur ^= 1;
    m->serial.cur ^= 1;
    m->next_serial += n_points;
    m->kf_epoch++;
    for (int i = 0; i < RM_N_COUNTS; i++) m->n[i] = rows[i];
    m->kfs.assign((size_t)n_kf, nullptr);
    if (kfs) std::copy(kfs, kfs + n_kf, m->kfs.begin());
    m->h_poses.assign(kf_poses12, kf_poses12 + (size_t)12 * n_kf);
    m->h_fixed.assign(kf_fixed, kf_fixed + n_kf);
    return PTAM_OK;
}

int ptam_rmap_download(ptam_rmap* m, int which, int first, int count, void* dst) {
    ARG_TRY(m && which >= 0 && which < PTAM_RMAP_TABLES);
    ARG_TRY(first >= 0 && count >= 0 && (long long)first + count <= m->n[RM_COUNT_OF[which]]);
    ARG_TRY(count == 0 || dst);
    if (count == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    const size_t rb = RM_ROW_BYTES[which];
    if (int rc = rm_down(m, dst, m->t[which].now() + (size_t)first * rb, (size_t)count * rb)) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    return PTAM_OK;
}

int ptam_rmap_bundle_adjust(ptam_rmap* m, const ptam_ba_opts* opts, int mode, const volatile unsigned char* abort_flag,
                            ptam_map_ba_result* res, ptam_map_outlier* outliers, int outlier_cap, int32_t* cam_kf, int32_t* point_ids) {
    ARG_TRY(m && res);
    ARG_TRY(mode == PTAM_MAP_BA_ALL || mode == PTAM_MAP_BA_RECENT);
    ARG_TRY(!outliers || outlier_cap >= m->n[RM_N_MEAS]);
    MbaTables t = {};
    t.K = m->n[RM_N_KF];
    t.N = m->n[RM_N_POINTS];
    t.M = m->n[RM_N_MEAS];
    t.h_poses = m->h_poses.data();
    t.h_fixed = m->h_fixed.data();
    t.d_poses = rm_now<double>(m, PTAM_RMAP_KF_POSES);
    t.d_fixed = rm_now<uint8_t>(m, PTAM_RMAP_KF_FIXED);
    t.d_points3 = rm_now<double>(m, PTAM_RMAP_POINTS3);
    t.d_meas = rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    t.d_points = rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS);
    t.poses_out = m->h_poses.data();   // the mirror follows an accepted bundle; the caller fetches the poses with ptam_rmap_download
    unsigned long long moved[2] = {0, 0};
    const int rc = mba_run(m->ctx, opts, mode, t, abort_flag, res, outliers, cam_kf, point_ids, moved);
    m->h2d += moved[0];
    m->d2h += moved[1];
    return rc;
}

int ptam_rmap_refind(ptam_rmap* m, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_work, const void* work,
                     const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix,
                     ptam_map_pair* never_out, int out_cap) {
    ARG_TRY(m && finder && res && n_work >= 0);
    ARG_TRY(mode == PTAM_MAP_REFIND_KEYFRAME || mode == PTAM_MAP_REFIND_NEW_POINTS || mode == PTAM_MAP_REFIND_FAILURE_QUEUE);
    ARG_TRY(work || n_work == 0);
    ARG_TRY(work || mode != PTAM_MAP_REFIND_KEYFRAME);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER], Q = m->n[RM_N_NEW], F = m->n[RM_N_FAILURE];
    ptam_map_refind_result zero = {};
    if (K == 0) {
        ARG_TRY(n_work == 0 || mode != PTAM_MAP_REFIND_KEYFRAME);
        *res = zero;
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    // the resident queue: it comes down (4 or 8 bytes an entry, and a bBad byte per new point), because the pair order is the host's
    const bool from_queue = work == nullptr;
    std::vector<int32_t> hq;
    std::vector<ptam_map_pair> hf;
    std::vector<uint8_t> hbad;
    if (from_queue && mode == PTAM_MAP_REFIND_NEW_POINTS && Q > 0) {
        hq.resize((size_t)Q);
        hbad.resize((size_t)Q);
        void* sc;
        if (int rc = ctx_scratch(m->ctx, rm_up256((size_t)Q), &sc)) return rc;
        hipLaunchKernelGGL(rm_queue_bad_kernel, dim3(rm_blocks(Q)), dim3(256), 0, st, Q, (const int32_t*)rm_now<int32_t>(m, PTAM_RMAP_NEW_QUEUE),
                           (const uint8_t*)rm_now<uint8_t>(m, PTAM_RMAP_BAD), (uint8_t*)sc);
        HIP_TRY(hipGetLastError());
        if (int rc = rm_down(m, hq.data(), rm_now<int32_t>(m, PTAM_RMAP_NEW_QUEUE), (size_t)Q * 4)) return rc;
        if (int rc = rm_down(m, hbad.data(), sc, (size_t)Q)) return rc;
        HIP_TRY(ptam_stream_wait(st));
        work = hq.data();
        n_work = Q;
    } else if (from_queue && mode == PTAM_MAP_REFIND_FAILURE_QUEUE && F > 0) {
        hf.resize((size_t)F);
        if (int rc = rm_down(m, hf.data(), rm_now<ptam_map_pair>(m, PTAM_RMAP_FAILURE), (size_t)F * sizeof(ptam_map_pair))) return rc;
        HIP_TRY(ptam_stream_wait(st));
        work = hf.data();
        n_work = F;
    } else if (!from_queue && mode == PTAM_MAP_REFIND_NEW_POINTS && n_work > 0) {   // the caller's list: bBad of its points
        const int32_t* w = (const int32_t*)work;
        for (int e = 0; e < n_work; e++) ARG_TRY(w[e] >= 0 && w[e] < N);
        hbad.resize((size_t)n_work);
        void* sc;
        const size_t o_b = rm_up256((size_t)n_work * 4);
        if (int rc = ctx_scratch(m->ctx, o_b + rm_up256((size_t)n_work), &sc)) return rc;
        if (int rc = rm_up(m, sc, w, (size_t)n_work * 4)) return rc;
        hipLaunchKernelGGL(rm_queue_bad_kernel, dim3(rm_blocks(n_work)), dim3(256), 0, st, n_work, (const int32_t*)sc,
                           (const uint8_t*)rm_now<uint8_t>(m, PTAM_RMAP_BAD), (uint8_t*)sc + o_b);
        HIP_TRY(hipGetLastError());
        if (int rc = rm_down(m, hbad.data(), (char*)sc + o_b, (size_t)n_work)) return rc;
        HIP_TRY(ptam_stream_wait(st));
    }
    const long long pairs = mode == PTAM_MAP_REFIND_KEYFRAME ? (n_work ? N : 0) : mode == PTAM_MAP_REFIND_NEW_POINTS ? (long long)K * n_work : n_work;
    ARG_TRY(pairs + M < (1ll << 31) && pairs + V < (1ll << 31));
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, M + pairs)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, V + pairs)) return rc;
    MrTables t = {};
    t.n_kf = K;
    t.n_points = N;
    t.n_meas = M;
    t.n_never = V;
    t.kfs = m->kfs.data();
    t.d_poses = rm_now<double>(m, PTAM_RMAP_KF_POSES);
    t.d_points = rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS);
    t.d_meas = rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    t.d_never = rm_now<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    t.d_meas_merged = rm_alt<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    t.d_never_merged = rm_alt<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    t.work_bad = hbad.empty() ? nullptr : hbad.data();
    int written = 0;
    unsigned long long moved[2] = {0, 0};
    ptam_map_refind_result r = {};
    const int rc = mr_run(m->ctx, finder, opts, mode, t, n_work, work, stop_flag, &r, found_out, found_subpix, never_out, out_cap, nullptr, nullptr,
                          &written, moved);
    m->h2d += moved[0];
    m->d2h += moved[1];
    if (rc) return rc;
    if (written) {   // the merged tables become the map's
        m->t[PTAM_RMAP_MEAS].cur ^= 1;
        m->t[PTAM_RMAP_NEVER].cur ^= 1;
        m->n[RM_N_MEAS] = M + r.n_found;
        m->n[RM_N_NEVER] = V + r.n_never;
    }
    if (from_queue && mode == PTAM_MAP_REFIND_NEW_POINTS && r.points_consumed > 0) {   // popped from the front (:1055)
        const int left = Q - r.points_consumed;
        if (left > 0) {
            HIP_TRY(hipMemcpyAsync(rm_alt<int32_t>(m, PTAM_RMAP_NEW_QUEUE), rm_now<int32_t>(m, PTAM_RMAP_NEW_QUEUE) + r.points_consumed,
                                   (size_t)left * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(ptam_stream_wait(st));
            m->t[PTAM_RMAP_NEW_QUEUE].cur ^= 1;
        }
        m->n[RM_N_NEW] = left;
    }
    if (from_queue && mode == PTAM_MAP_REFIND_FAILURE_QUEUE && !r.stopped) m->n[RM_N_FAILURE] = 0;   // mvFailureQueue.clear() (:1080)
    *res = r;
    return PTAM_OK;
}

int ptam_rmap_apply_global_transform(ptam_rmap* m, const double se3_new_from_old[12], ptam_pvs_point* out_rows) {
    ARG_TRY(m && se3_new_from_old);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS];
    if (K + N == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    hipStream_t st = m->ctx->stream;
    // poses: into the second buffer; points3 in place, the pixel vectors (pv.world among them) into the point rows: nothing refuses
    // the call once the kernel runs
    if (int rc = map_transform_core(m->ctx, se3_new_from_old, K, rm_now<double>(m, PTAM_RMAP_KF_POSES), rm_alt<double>(m, PTAM_RMAP_KF_POSES), N,
                                    rm_now<double>(m, PTAM_RMAP_POINTS3), rm_now<ptam_map_point_source>(m, PTAM_RMAP_SOURCES),
                                    (ptam_pvs_point*)rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS), (int)sizeof(ptam_map_refind_point)))
        return rc;
    m->h2d += 256;   // the aligner's record
    if (K > 0)
        if (int rc = rm_down(m, m->h_poses.data(), rm_alt<double>(m, PTAM_RMAP_KF_POSES), (size_t)K * 96)) return rc;   // the mirror
    if (out_rows && N > 0) {
        void* sc;   // (the aligner's record in the scratch has been queued for reading; the packed rows go behind it)
        if ((size_t)256 + (size_t)N * sizeof(ptam_pvs_point) > m->ctx->d_scratch_cap) {
            HIP_TRY(ptam_stream_wait(st));
        }
        if (int rc = ctx_scratch(m->ctx, 256 + (size_t)N * sizeof(ptam_pvs_point), &sc)) return rc;
        ptam_pvs_point* packed = (ptam_pvs_point*)((char*)sc + 256);
        hipLaunchKernelGGL(rm_pack_pvs_kernel, dim3(rm_blocks(N)), dim3(256), 0, st, N,
                           (const ptam_map_refind_point*)rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS), packed);
        HIP_TRY(hipGetLastError());
        if (int rc = rm_down(m, out_rows, packed, (size_t)N * sizeof(ptam_pvs_point))) return rc;
    }
    HIP_TRY(ptam_stream_wait(st));
    m->t[PTAM_RMAP_KF_POSES].cur ^= 1;
    return PTAM_OK;
}

int ptam_rmap_apply_outliers(ptam_rmap* m, int n_outliers, const ptam_map_outlier* outliers, ptam_map_outliers_result* res) {
    ARG_TRY(m && res && n_outliers >= 0 && (n_outliers == 0 || outliers));
    const int n_meas = m->n[RM_N_MEAS], n_never = m->n[RM_N_NEVER], n_failure = m->n[RM_N_FAILURE];
    ARG_TRY((long long)n_never + n_outliers < (1ll << 31) && (long long)n_failure + n_outliers < (1ll << 31));
    ptam_map_outliers_result r = {};
    for (int i = 0; i < n_outliers; i++) {   // what the list alone decides
        const ptam_map_outlier& o = outliers[i];
        ARG_TRY(o.action >= PTAM_MAP_OUT_POINT_BAD && o.action <= PTAM_MAP_OUT_NEVER_RETRY);
        ARG_TRY(o.meas >= 0 && o.meas < n_meas);
        if (o.action == PTAM_MAP_OUT_NEVER_RETRY) r.n_never_added++;
        else if (o.action == PTAM_MAP_OUT_FAILURE_QUEUE) r.n_failure_added++;
        else r.n_point_bad++;
    }
    r.n_meas_out = n_meas - r.n_failure_added - r.n_never_added;
    r.n_never_out = n_never + r.n_never_added;
    r.n_failure_out = n_failure + r.n_failure_added;
    if (n_outliers == 0) {
        *res = r;
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, r.n_never_out)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_FAILURE, (long long)n_failure + n_outliers)) return rc;   // (the compaction's room, not only its count)

    const size_t Mz = (size_t)n_meas, Oz = (size_t)n_outliers;
    RmCarve c;
    const size_t o_outl = c.take(Oz * sizeof(ptam_map_outlier)), o_flag = c.take(Mz), o_owner = c.take(Mz * sizeof(unsigned)),
                 o_tiles = c.take((size_t)mt_tiles(std::max(n_meas, n_outliers)) * sizeof(int)), o_nn = c.take(Oz * sizeof(ptam_map_pair));
    void* sc;
    if (int rc = ctx_scratch(m->ctx, c.off, &sc)) return rc;
    char* b = (char*)sc;
    hipStream_t st = m->ctx->stream;
    if (int rc = rm_up(m, b + o_outl, outliers, Oz * sizeof(ptam_map_outlier))) return rc;
    if (int rc = rm_words_reset(m)) return rc;
    HIP_TRY(hipMemsetAsync(b + o_owner, 0xff, Mz * sizeof(unsigned), st));   // (n_meas > 0: an outlier names a row)
    int* err = m->d_words + RM_W_CALL;
    const ptam_map_outlier* d_outl = (const ptam_map_outlier*)(b + o_outl);
    hipLaunchKernelGGL(rm_outliers_check_kernel, dim3(rm_blocks(n_outliers)), dim3(256), 0, st, n_outliers, d_outl,
                       (const ptam_map_meas*)rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS), n_never,
                       (const ptam_map_pair*)rm_now<ptam_map_pair>(m, PTAM_RMAP_NEVER), (unsigned*)(b + o_owner), err);
    hipLaunchKernelGGL(rm_outliers_twice_kernel, dim3(rm_blocks(n_outliers)), dim3(256), 0, st, n_outliers, d_outl, (const unsigned*)(b + o_owner), err);
    MtOutliersDev d = {};
    d.n_meas = n_meas;
    d.n_never = n_never;
    d.n_outliers = n_outliers;
    d.n_never_out = r.n_never_out;
    d.meas = rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    d.never = rm_now<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    d.outliers = d_outl;
    d.bad = rm_now<uint8_t>(m, PTAM_RMAP_BAD);
    d.points = rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS);
    d.gate = err;
    d.flag = (uint8_t*)(b + o_flag);
    d.tot = m->d_words + RM_W_TOT;
    d.tiles = (int*)(b + o_tiles);
    d.new_never = (ptam_map_pair*)(b + o_nn);
    d.meas_out = rm_alt<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    d.never_out = rm_alt<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    d.failure_new = rm_now<ptam_map_pair>(m, PTAM_RMAP_FAILURE) + n_failure;   // behind the count
    if (int rc = mt_apply_outliers_core(st, d)) return rc;
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    if (hw[RM_W_CALL] != RM_NO_ROW) return rm_refuse(m, PTAM_RMAP_OUTLIERS, hw[RM_W_CALL]);
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->t[PTAM_RMAP_NEVER].cur ^= 1;
    m->n[RM_N_MEAS] = r.n_meas_out;
    m->n[RM_N_NEVER] = r.n_never_out;
    m->n[RM_N_FAILURE] = r.n_failure_out;
    *res = r;
    return PTAM_OK;
}

int ptam_rmap_handle_bad_points(ptam_rmap* m, ptam_map_bad_points_result* res, int32_t* kept_out, int32_t* new_index_out) {
    ARG_TRY(m && res);
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER], Q = m->n[RM_N_NEW], F = m->n[RM_N_FAILURE];
    const size_t Nz = (size_t)N;
    RmCarve c;
    const size_t o_rem = c.take(Nz), o_tiles = c.take((size_t)mt_tiles(std::max(std::max(N, M), std::max(std::max(V, Q), F))) * sizeof(int)),
                 o_ni = c.take(Nz * 4), o_kept = c.take(Nz * 4);
    void* sc;
    if (int rc = ctx_scratch(m->ctx, c.off, &sc)) return rc;
    char* b = (char*)sc;
    hipStream_t st = m->ctx->stream;
    if (int rc = rm_words_reset(m)) return rc;
    MtBadDev d = {};
    d.n_points = N;
    d.n_meas = M;
    d.n_never = V;
    d.n_new = Q;
    d.n_failure = F;
    d.bad = rm_now<uint8_t>(m, PTAM_RMAP_BAD);
    d.outlier_count = rm_now<int32_t>(m, PTAM_RMAP_OUTLIER_COUNT);
    d.inlier_count = rm_now<int32_t>(m, PTAM_RMAP_INLIER_COUNT);
    d.meas = rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    d.never = rm_now<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    d.new_queue = rm_now<int32_t>(m, PTAM_RMAP_NEW_QUEUE);
    d.failure = rm_now<ptam_map_pair>(m, PTAM_RMAP_FAILURE);
    d.removed = (uint8_t*)(b + o_rem);
    d.tot = m->d_words + RM_W_TOT;
    d.tiles = (int*)(b + o_tiles);
    d.new_index = (int32_t*)(b + o_ni);
    d.kept = (int32_t*)(b + o_kept);
    d.meas_out = rm_alt<ptam_map_meas>(m, PTAM_RMAP_MEAS);
    d.never_out = rm_alt<ptam_map_pair>(m, PTAM_RMAP_NEVER);
    d.new_out = rm_alt<int32_t>(m, PTAM_RMAP_NEW_QUEUE);
    d.failure_out = rm_alt<ptam_map_pair>(m, PTAM_RMAP_FAILURE);
    // the point-side tables, all compacted; a survivor's bad byte is 0 (it would not have survived)
    const int cols[5] = {PTAM_RMAP_POINTS3, PTAM_RMAP_REFIND_POINTS, PTAM_RMAP_SOURCES, PTAM_RMAP_OUTLIER_COUNT, PTAM_RMAP_INLIER_COUNT};
    d.n_columns = 6;
    for (int k = 0; k < 5; k++) {
        d.col_in[k] = m->t[cols[k]].now();
        d.col_out[k] = m->t[cols[k]].alt();
        d.col_dwords[k] = (int)(RM_ROW_BYTES[cols[k]] / 4);
    }
    d.col_in[5] = m->serial.now();   // the serials: compacted in order, so still strictly increasing
    d.col_out[5] = m->serial.alt();
    d.col_dwords[5] = (int)(sizeof(long long) / 4);
    if (N > 0) HIP_TRY(hipMemsetAsync(m->t[PTAM_RMAP_BAD].alt(), 0, Nz, st));
    if (int rc = mt_handle_bad_points_core(st, d)) return rc;
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    const int* hc = hw + RM_W_TOT;
    ptam_map_bad_points_result r = {};
    r.n_marked = hc[MT_T_MARKED];
    r.n_kept = hc[MT_T_KEPT];
    r.n_removed = N - r.n_kept;
    r.n_meas_out = hc[MT_T_MEAS];
    r.n_never_out = hc[MT_T_NEVER];
    r.n_new_out = hc[MT_T_NEW];
    r.n_new_dropped = Q - r.n_new_out;
    r.n_failure_out = hc[MT_T_FAIL];
    for (int w = PTAM_RMAP_POINTS3; w < PTAM_RMAP_TABLES; w++) m->t[w].cur ^= 1;
    m->serial.cur ^= 1;
    m->n[RM_N_POINTS] = r.n_kept;
    m->n[RM_N_MEAS] = r.n_meas_out;
    m->n[RM_N_NEVER] = r.n_never_out;
    m->n[RM_N_NEW] = r.n_new_out;
    m->n[RM_N_FAILURE] = r.n_failure_out;
    if (kept_out || new_index_out) {   // (the scratch is untouched until the next call)
        if (kept_out)
            if (int rc = rm_down(m, kept_out, b + o_kept, (size_t)r.n_kept * 4)) return rc;
        if (new_index_out)
            if (int rc = rm_down(m, new_index_out, b + o_ni, Nz * 4)) return rc;
        HIP_TRY(ptam_stream_wait(st));
    }
    *res = r;
    return PTAM_OK;
}

int ptam_rmap_add_points(ptam_rmap* m, int src_kf, int target_kf, int target_source, int n_made, const ptam_new_map_point* made) {
    ARG_TRY(m && n_made >= 0 && (n_made == 0 || made));
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], Q = m->n[RM_N_NEW];
    ARG_TRY((long long)N + n_made < (1ll << 31) && (long long)M + 2ll * n_made < (1ll << 31) && (long long)Q + n_made < (1ll << 31));
    ARG_TRY(src_kf >= 0 && src_kf < K && target_kf >= 0 && target_kf < K && src_kf != target_kf);
    ARG_TRY(target_source >= PTAM_MAP_SRC_TRACKER && target_source <= PTAM_MAP_SRC_EPIPOLAR);
    for (int i = 0; i < n_made; i++) ARG_TRY(made[i].level >= 0 && made[i].level < PTAM_LEVELS);
    if (n_made == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    // (the tables' room first: growing one waits for the stream, and the records are read from the scratch after it)
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)M + 2ll * n_made)) return rc;
    if (int rc = rm_room_points(m, (long long)N + n_made)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEW_QUEUE, (long long)Q + n_made)) return rc;
    void* sc;
    if (int rc = ctx_scratch(m->ctx, rm_up256((size_t)n_made * sizeof(ptam_new_map_point)), &sc)) return rc;
    if (int rc = rm_up(m, sc, made, (size_t)n_made * sizeof(ptam_new_map_point))) return rc;
    return rm_add_points_device(m, src_kf, target_kf, target_source, n_made, (const ptam_new_map_point*)sc);
}

int ptam_rmap_add_keyframe(ptam_rmap* m, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows, const ptam_map_kf_row* rows) {
    ARG_TRY(m && pose12 && n_rows >= 0 && (n_rows == 0 || rows));
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS];
    ARG_TRY((long long)K + 1 < (1ll << 31) && (long long)M + n_rows < (1ll << 31));
    if (int rc = rm_check_kf_rows(N, n_rows, rows)) return rc;   // the small list is checked where it is
    HIP_TRY(hipSetDevice(m->ctx->device));
    const uint8_t fx = fixed ? 1 : 0;
    if (int rc = rm_add_keyframe_enqueue(m, pose12, &fx, n_rows, rows)) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    rm_add_keyframe_commit(m, kf, pose12, fx, n_rows);
    return PTAM_OK;
}

int ptam_rmap_note_tracked(ptam_rmap* m, int n, const int32_t* points, const uint8_t* outlier_flags) {
    ARG_TRY(m && n >= 0 && (n == 0 || (points && outlier_flags)));
    const int N = m->n[RM_N_POINTS];
    for (int i = 0; i < n; i++) ARG_TRY(points[i] >= 0 && points[i] < N);
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    const size_t o_flags = rm_up256((size_t)n * 4);
    void* sc;
    if (int rc = ctx_scratch(m->ctx, o_flags + rm_up256((size_t)n), &sc)) return rc;
    char* b = (char*)sc;
    if (int rc = rm_up(m, b, points, (size_t)n * 4)) return rc;
    if (int rc = rm_up(m, b + o_flags, outlier_flags, (size_t)n)) return rc;
    hipLaunchKernelGGL(rm_note_tracked_kernel, dim3(rm_blocks(n)), dim3(256), 0, m->ctx->stream, n, (const int32_t*)b, (const uint8_t*)(b + o_flags),
                       rm_now<int32_t>(m, PTAM_RMAP_OUTLIER_COUNT), rm_now<int32_t>(m, PTAM_RMAP_INLIER_COUNT));
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    return PTAM_OK;
}

int ptam_rmap_scene_depth(ptam_rmap* m, ptam_scene_depth* out) {
    ARG_TRY(m);
    const int K = m->n[RM_N_KF];
    ARG_TRY(K == 0 || out);
    if (K == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = map_scene_depth_core(m->ctx, K, rm_now<double>(m, PTAM_RMAP_KF_POSES), rm_now<double>(m, PTAM_RMAP_POINTS3), m->n[RM_N_MEAS],
                                      rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS), out))
        return rc;
    m->d2h += (size_t)K * sizeof(ptam_scene_depth);   // (written by the kernel into host-mapped memory)
    return PTAM_OK;
}

int ptam_rmap_closest_keyframes(ptam_rmap* m, int kf, int n, int32_t* out_kf, double* out_dist, int32_t* n_out) {
    ARG_TRY(m && out_kf && out_dist && n_out);
    const int K = m->n[RM_N_KF];
    ARG_TRY(kf >= 0 && kf < K && n >= 1);
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int n_pick = std::min(n, K - 1);
    const int* hdr;
    const double* dist;
    const int32_t* idx;
    if (int rc = rm_closest(m, K, kf, -1, n_pick, &hdr, &dist, &idx)) return rc;
    const int got = std::min(std::max(hdr[0], 0), n_pick);
    std::copy(idx, idx + got, out_kf);
    std::copy(dist, dist + got, out_dist);
    *n_out = got;
    return PTAM_OK;
}

// what both consumers ask of a report, on the host
static int rm_report_usable(const ptam_rmap* m, const ptam_frame_report* rep) {
    ARG_TRY(rep && rep->ctx->device == m->ctx->device);
    ARG_TRY(rep->info.n_records > 0 && rep->info.n_records <= rep->max_records);
    ARG_TRY(rep->info.map_id == m->map_id);
    return PTAM_OK;
}

int ptam_rmap_note_reports(ptam_rmap* m, int n, ptam_frame_report* const* reports, ptam_rmap_note_result* res) {
    ARG_TRY(m && res && n >= 1 && n <= 65535 && reports);
    std::vector<RmReportRef> refs((size_t)n);
    int most = 0;
    long long all = 0;
    for (int i = 0; i < n; i++) {
        if (int rc = rm_report_usable(m, reports[i])) return rc;
        refs[(size_t)i] = RmReportRef{reports[i]->rec, reports[i]->info.n_records, 0};
        most = std::max(most, reports[i]->info.n_records);
        all += reports[i]->info.n_records;
    }
    ARG_TRY(all < (1ll << 31));
    HIP_TRY(hipSetDevice(m->ctx->device));
    void* sc;
    if (int rc = ctx_scratch(m->ctx, rm_up256((size_t)n * sizeof(RmReportRef)), &sc)) return rc;
    if (int rc = rm_up(m, sc, refs.data(), (size_t)n * sizeof(RmReportRef))) return rc;
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_note_reports_kernel, dim3(rm_blocks(most), (unsigned)n), dim3(256), 0, m->ctx->stream, (const RmReportRef*)sc,
                       m->n[RM_N_POINTS], (const long long*)m->serial.now(), rm_now<int32_t>(m, PTAM_RMAP_OUTLIER_COUNT),
                       rm_now<int32_t>(m, PTAM_RMAP_INLIER_COUNT), m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    res->n_records = (int32_t)all;
    res->n_gone = hw[RM_W_TOT];
    return PTAM_OK;
}

// ptam_rmap_insert_keyframe and ptam_rmap_insert_keyframe_report: the rows of step (a) from the host (rows) or from a report (rep)
static int rm_insert_keyframe(ptam_rmap* m, ptam_refinder* finder, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows,
                              const ptam_map_kf_row* rows, const ptam_frame_report* rep, const ptam_rmap_insert_opts* opts,
                              ptam_rmap_insert_result* res, int* n_rows_out) {
    // ---- refusals: nothing is enqueued before all of them have passed
    ARG_TRY(m && finder && kf && pose12 && opts && res && n_rows >= 0 && (n_rows == 0 || rows || rep));
    ptam_ctx* ctx = m->ctx;
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER];
    const bool refind = !opts->skip_refind, points = !opts->skip_points;
    ARG_TRY(finder->ctx->device == ctx->device && opts->refind.max_pairs_per_pass >= 0);
    ARG_TRY((long long)K + 1 < (1ll << 31) && (long long)M + n_rows + N < (1ll << 31) && (long long)V + N < (1ll << 31));
    if (!rep)
        if (int rc = rm_check_kf_rows(N, n_rows, rows)) return rc;
    ARG_TRY(opts->target_kf >= -1 && opts->target_kf < K);
    auto usable = [&](const ptam_kf* k) { return k && k->device == ctx->device && k->L.w[0] == ctx->params.width && k->L.h[0] == ctx->params.height; };
    ARG_TRY(usable(kf));
    if (refind || points)
        for (int k = 0; k < K; k++) ARG_TRY(usable(m->kfs[(size_t)k]));   // the re-find visits every source keyframe; any may be the target
    if (points) {
        if (int rc = epi_check(kf, &opts->epipolar)) return rc;
        if (K == 0) {
            ptam_set_error("ptam_rmap_insert_keyframe: the map has no keyframe to be the closest one");
            return PTAM_E_STATE;
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    EpiRun run = {};
    if (points) {   // (the corner counts of the new keyframe's levels, read from its handle: every made point is one of them)
        if (int rc = epi_sizes(ctx, kf, &opts->epipolar, run)) return rc;
        ARG_TRY((long long)N + run.sum < (1ll << 31) && (long long)M + n_rows + N + 2ll * run.sum < (1ll << 31) &&
                (long long)m->n[RM_N_NEW] + run.sum < (1ll << 31));
    }
    hipStream_t st = ctx->stream;
    ptam_rmap_insert_result r = {};
    r.kf = K;
    r.target_kf = -1;
    r.first_point = N;
    // ---- (a) the keyframe's rows; the counts move at once: nothing below can refuse the call
    const uint8_t fx = fixed ? 1 : 0;
    if (rep) {   // (n_rows was the bound: the records; now the live ones)
        if (int rc = rm_add_keyframe_enqueue_report(m, pose12, &fx, rep, &n_rows)) return rc;
    } else if (int rc = rm_add_keyframe_enqueue(m, pose12, &fx, n_rows, rows))
        return rc;
    rm_add_keyframe_commit(m, kf, pose12, fx, n_rows);
    if (n_rows_out) *n_rows_out = n_rows;
    // ---- (c) the target: it needs the poses alone, and its wait is (a)'s
    if (points) {
        const int* hdr;
        const double* dist;
        const int32_t* idx;
        if (int rc = rm_closest(m, K + 1, K, opts->target_kf, 1, &hdr, &dist, &idx)) return rc;
        if (hdr[0] != 1 || idx[0] < 0 || idx[0] >= K) {
            ptam_set_error("ptam_rmap_insert_keyframe: no closest keyframe among %d", K);
            return PTAM_E_STATE;
        }
        r.target_kf = idx[0];
        r.target_dist = dist[0];
    }
    // ---- (b) the re-find of the new keyframe; the merged tables become the map's
    if (refind) {
        const int32_t work = K;
        if (int rc = ptam_rmap_refind(m, finder, &opts->refind, PTAM_MAP_REFIND_KEYFRAME, 1, &work, nullptr, &r.refind, nullptr, nullptr, nullptr, 0)) return rc;
    }
    if (!points) {
        HIP_TRY(ptam_stream_wait(st));
        *res = r;
        return PTAM_OK;
    }
    // ---- (d) the busy list: the new keyframe's run is the tail of the table as (b) left it
    const int n_busy = m->n[RM_N_MEAS] - M;
    ptam_kf* target = const_cast<ptam_kf*>(m->kfs[(size_t)r.target_kf]);   // (its implane tables are cached on the handle)
    if (int rc = epi_carve(ctx, target, &opts->epipolar, n_busy, run)) return rc;
    HIP_TRY(hipMemsetAsync(run.d_hdr, 0, EPI_HDR_BYTES, st));
    hipLaunchKernelGGL(rm_busy_kernel, dim3(std::max(rm_blocks(n_busy), 1u)), dim3(256), 0, st, n_busy,
                       (const ptam_map_meas*)rm_now<ptam_map_meas>(m, PTAM_RMAP_MEAS) + M, run.d_busy, run.d_hdr);
    HIP_TRY(hipGetLastError());
    // ---- (e) the epipolar chain, (f) its count and stats
    if (int rc = epi_launch_chain(ctx, kf, pose12, target, m->h_poses.data() + (size_t)12 * r.target_kf, &opts->epipolar, run)) return rc;
    void* hp;
    if (int rc = ctx_pinned(ctx, EPI_HDR_BYTES, &hp)) return rc;
    if (int rc = rm_down(m, hp, run.d_hdr, EPI_HDR_BYTES)) return rc;
    HIP_TRY(ptam_stream_wait(st));
    const int made = ((const int*)hp)[1];
    if (made < 0 || made > run.sum) {
        ptam_set_error("ptam_rmap_insert_keyframe: %d points made, room for %d", made, run.sum);
        return PTAM_E_STATE;
    }
    std::memcpy(r.levels, (const char*)hp + 16, sizeof(ptam_epipolar_level_stats) * (size_t)run.nl);
    r.n_made = made;
    // ---- (g) the made points into the tables, straight from the chain's output
    if (made > 0)
        if (int rc = rm_add_points_device(m, K, r.target_kf, PTAM_MAP_SRC_EPIPOLAR, made, run.d_out)) return rc;
    *res = r;
    return PTAM_OK;
}

int ptam_rmap_insert_keyframe(ptam_rmap* m, ptam_refinder* finder, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows,
                              const ptam_map_kf_row* rows, const ptam_rmap_insert_opts* opts, ptam_rmap_insert_result* res) {
    ARG_TRY(n_rows == 0 || rows);
    return rm_insert_keyframe(m, finder, kf, pose12, fixed, n_rows, rows, nullptr, opts, res, nullptr);
}

int ptam_rmap_insert_keyframe_report(ptam_rmap* m, ptam_refinder* finder, const ptam_kf* kf, const double pose12[12], int fixed,
                                     ptam_frame_report* report, const ptam_rmap_insert_opts* opts, ptam_rmap_insert_result* res, int32_t* n_rows,
                                     int32_t* n_gone) {
    ARG_TRY(m);
    if (int rc = rm_report_usable(m, report)) return rc;
    int live = 0;
    if (int rc = rm_insert_keyframe(m, finder, kf, pose12, fixed, report->info.n_records, nullptr, report, opts, res, &live)) return rc;
    if (n_rows) *n_rows = live;
    if (n_gone) *n_gone = report->info.n_records - live;
    return PTAM_OK;
}

int ptam_rmap_point_serials(ptam_rmap* m, int first, int count, int64_t* out) {
    ARG_TRY(m && first >= 0 && count >= 0 && (long long)first + count <= m->n[RM_N_POINTS]);
    ARG_TRY(count == 0 || out);
    if (count == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = rm_down(m, out, (const long long*)m->serial.now() + first, (size_t)count * sizeof(long long))) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    return PTAM_OK;
}

int ptam_rmap_resolve_serials(ptam_rmap* m, int n, const int64_t* serials, int32_t* index_out, int32_t* n_gone) {
    ARG_TRY(m && n >= 0 && (n == 0 || (serials && index_out)));
    if (n_gone) *n_gone = 0;
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    const size_t o_idx = rm_up256((size_t)n * sizeof(long long));
    void* sc;
    if (int rc = ctx_scratch(m->ctx, o_idx + rm_up256((size_t)n * 4), &sc)) return rc;
    char* b = (char*)sc;
    if (int rc = rm_up(m, b, serials, (size_t)n * sizeof(long long))) return rc;
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_resolve_kernel, dim3(rm_blocks(n)), dim3(256), 0, m->ctx->stream, n, (const long long*)b, m->n[RM_N_POINTS],
                       (const long long*)m->serial.now(), (int32_t*)(b + o_idx), m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    if (int rc = rm_down(m, index_out, b + o_idx, (size_t)n * 4)) return rc;
    const int* hw;
    if (int rc = rm_words_wait(m, &hw)) return rc;
    if (n_gone) *n_gone = hw[RM_W_TOT];
    return PTAM_OK;
}

int ptam_rmap_publish(ptam_rmap* m, ptam_map_snapshot* snap, ptam_map_publish_result* res) {
    // ---- refusals: nothing is enqueued, and no slot is taken, before all of them have passed
    ARG_TRY(m && snap && res);
    ARG_TRY(snap->device == m->ctx->device);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS];
    for (int k = 0; k < K; k++) ARG_TRY(m->kfs[(size_t)k] && m->kfs[(size_t)k]->device == m->ctx->device);
    HIP_TRY(hipSetDevice(m->ctx->device));
    std::vector<RmKfRecord> recs((size_t)K);
    for (int k = 0; k < K; k++)
        for (int l = 0; l < PTAM_LEVELS; l++) {
            recs[(size_t)k].im[l] = m->kfs[(size_t)k]->L.im[l];
            recs[(size_t)k].w[l] = m->kfs[(size_t)k]->L.w[l];
            recs[(size_t)k].h[l] = m->kfs[(size_t)k]->L.h[l];
        }
    const bool with_kfs = sbi_snapshot_kf_enabled(snap);   // the keyframe section: poses, and the images the slot lacks
    if (with_kfs)
        if (int rc = sbi_snapshot_kf_check(snap, K, m->kfs.data())) return rc;
    const size_t o_l3 = rm_up256((size_t)K * sizeof(RmKfRecord));
    void* sc;
    if (int rc = ctx_scratch(m->ctx, o_l3 + rm_up256((size_t)K * sizeof(const uint8_t*)), &sc)) return rc;
    const int s = snap->slots.begin_write();
    if (s < 0) {
        ptam_set_error("ptam_rmap_publish: a publish into this snapshot is under way");
        return PTAM_E_STATE;
    }
    // ---- the free slot is this call's until the commit
    ptam_map_publish_result r = {};
    int grew = 0;
    int rc = snap_slot_room(snap, s, (size_t)std::max(N, 1), &grew);
    if (!rc) rc = rm_up(m, sc, recs.data(), (size_t)K * sizeof(RmKfRecord));
    const int kf_first = with_kfs ? sbi_snapshot_kf_first_missing(snap, s, m->map_id, m->kf_epoch, K) : K;
    std::vector<const uint8_t*> l3((size_t)(K - kf_first));   // (lives until the wait below)
    if (!rc && with_kfs) {
        for (int k = kf_first; k < K; k++) l3[(size_t)(k - kf_first)] = m->kfs[(size_t)k]->L.im[3];
        const uint8_t** d_l3 = (const uint8_t**)((char*)sc + o_l3);
        rc = rm_up(m, d_l3, l3.data(), l3.size() * sizeof(l3[0]));
        if (!rc) rc = sbi_snapshot_kf_enqueue(m->ctx, snap, s, K, rm_now<double>(m, PTAM_RMAP_KF_POSES), kf_first, d_l3);
    }
    if (!rc && N > 0) {
        SnapSlot& sl = snap->slot[s];
        hipLaunchKernelGGL(rm_publish_kernel, dim3(rm_blocks(N)), dim3(256), 0, m->ctx->stream, N,
                           (const ptam_map_refind_point*)rm_now<ptam_map_refind_point>(m, PTAM_RMAP_REFIND_POINTS), (const long long*)m->serial.now(),
                           (const RmKfRecord*)sc, sl.pts, sl.src, sl.serials);
        if (hipGetLastError() != hipSuccess) rc = PTAM_E_HIP;
    }
    if (!rc && ptam_stream_wait(m->ctx->stream) != hipSuccess) rc = PTAM_E_HIP;   // the call's one wait: the slot is whole
    if (rc) {
        if (rc == PTAM_E_HIP) ptam_set_error("ptam_rmap_publish: the gather failed: %s", hipGetErrorString(hipGetLastError()));
        if (with_kfs) sbi_snapshot_kf_stamp(snap, s, 0, 0, 0, 0, 0);   // (its images may be half of one map, half of another)
        snap->slots.abort_write();
        return rc;
    }
    SnapSlot& sl = snap->slot[s];
    sl.n = N;
    sl.map_id = m->map_id;
    sl.generation = snap->slots.next_generation();
    if (with_kfs) sbi_snapshot_kf_stamp(snap, s, K, kf_first, m->map_id, m->kf_epoch, sl.generation);
    r.generation = snap->slots.commit_write();
    r.map_id = m->map_id;
    r.n_points = N;
    r.n_kf = K;
    r.grew = grew;
    *res = r;
    return PTAM_OK;
}

}   // extern "C"

void maprmap_preload_kernels() {
    ptam_preload((const void*)rm_closest_kernel);
    ptam_preload((const void*)rm_busy_kernel);
    ptam_preload((const void*)rm_check_sorted_kernel<ptam_map_meas, true>);
    ptam_preload((const void*)rm_check_sorted_kernel<ptam_map_pair, false>);
    ptam_preload((const void*)rm_check_pairs_kernel);
    ptam_preload((const void*)rm_queue_owner_kernel);
    ptam_preload((const void*)rm_queue_repeat_kernel);
    ptam_preload((const void*)rm_check_points_kernel);
    ptam_preload((const void*)rm_outliers_check_kernel);
    ptam_preload((const void*)rm_outliers_twice_kernel);
    ptam_preload((const void*)rm_add_keyframe_kernel);
    ptam_preload((const void*)rm_note_tracked_kernel);
    ptam_preload((const void*)rm_queue_bad_kernel);
    ptam_preload((const void*)rm_pack_pvs_kernel);
    ptam_preload((const void*)rm_serials_kernel);
    ptam_preload((const void*)rm_resolve_kernel);
    ptam_preload((const void*)rm_publish_kernel);
    ptam_preload((const void*)rm_note_reports_kernel);
    ptam_preload((const void*)rm_report_rows_kernel);
}
