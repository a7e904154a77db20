// maprmap.hip — ptam_rmap, the resident map (ptam_hip.h): the tables of the ptam_map_* calls kept in device memory, and the
// resident forms of the calls of one MapMaker::run() iteration (src/MapMaker.cc:57-114) that edit them:
//   ptam_rmap_upload / download     the whole map up (checked on the device), any row range down
//   ptam_rmap_apply_outliers        ptam_map_apply_outliers      } the cores of maptables.hip on the handle's buffers
//   ptam_rmap_handle_bad_points     ptam_map_handle_bad_points   }
//   ptam_rmap_add_points            ptam_map_add_points          }
//   ptam_rmap_note_tracked          the tracker's iteration set into the two counts (src/Tracker.cc:987-998)
//   ptam_rmap_scene_depth           ptam_map_scene_depth's kernel (mapalign.hip)
//   ptam_rmap_bundle_adjust         mba_core (mapba.hip) on the handle's buffers: adjusted in place, the poses into the mirror
//   ptam_rmap_bundle_adjust_routed  the two above as one call: the routed outlier list stays in the bundle's work memory
//   ptam_rmap_refind                mr_core (maprefind.hip): the merged tables into the second buffers, the resident queue popped
//   ptam_rmap_refind_queue          the same from the resident queue, the work lists built by kernels (maptables.hip): mr_run
//   ptam_rmap_apply_global_transform  map_apply_kernel (mapalign.hip): the pixel vectors straight into the point rows
// A keyframe into the map is maprmap_keyframe.hip; serials, frame reports and the map to the tracker are maprmap_publish.hip; the
// handle itself and the rule of its two buffers per table are rmap_internal.h.
// The kernels here check (rm_check_*) and count (rm_note_tracked_kernel, rm_outliers_tally_kernel).  Their atomics: atomicMin on a
// refusal word (only a thread that has found an offence issues one), atomicMin on an owner word per point / per row, integer
// atomicAdd on the counts.
// Nothing is handed between workgroups inside a launch: an owner word is written by one launch and compared by the next.
#include <algorithm>
#include <atomic>

#include "rmap_internal.h"

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

// ptam_rmap_bundle_adjust_routed: what mc_outliers_tally counts on the host, one thread per routed outlier: how many of each action
// (a ballot per action and wave, one integer atomicAdd per wave and action that occurs: exact in any order).  tally: three ints,
// zeroed by the caller, in the order of the actions
__global__ void __launch_bounds__(256) rm_outliers_tally_kernel(int n, const ptam_map_outlier* __restrict__ o, int* __restrict__ tally) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int action = i < n ? o[i].action : 0;
#pragma unroll
    for (int a = PTAM_MAP_OUT_POINT_BAD; a <= PTAM_MAP_OUT_NEVER_RETRY; a++) {
        const unsigned long long mk = __ballot(action == a);
        if ((threadIdx.x & 63) == 0 && mk) atomicAdd(tally + (a - PTAM_MAP_OUT_POINT_BAD), __popcll(mk));
    }
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

}   // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------------
int rm_room(ptam_rmap* m, int w, long long rows) {
    RmTable& t = m->t[w];
    if ((size_t)rows <= t.cap) return PTAM_OK;
    ARG_TRY(rows < (1ll << 31));
    const size_t cap = std::max(std::max((size_t)rows, 2 * t.cap), (size_t)64), row_bytes = RM_ROW_BYTES[w];
    char* nb[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++)
        if (hipMalloc((void**)&nb[k], cap * row_bytes) != hipSuccess) {
            if (nb[0]) (void)hipFree(nb[0]);
            ptam_set_error("ptam_rmap: no device memory for %zu rows of table %d", cap, w);
            return PTAM_E_HIP;
        }
    hipStream_t st = m->ctx->stream;
    const size_t live = (size_t)m->n[RM_COUNT_OF[w]] * row_bytes;
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
int rm_room_points(ptam_rmap* m, long long rows) {
    for (int w = 0; w < RM_TABLES; w++)
        if (rm_point_side(w))
            if (int rc = rm_room(m, w, rows)) return rc;
    return PTAM_OK;
}
static int rm_room_all(ptam_rmap* m, const int rows[RM_N_COUNTS]) {
    for (int w = 0; w < RM_TABLES; w++)
        if (int rc = rm_room(m, w, rows[RM_COUNT_OF[w]])) return rc;
    return PTAM_OK;
}

int rm_words_reset(ptam_rmap* m) {
    HIP_TRY(hipMemsetAsync(m->d_words, 0x7f, RM_W_ERRS * sizeof(int), m->ctx->stream));
    HIP_TRY(hipMemsetAsync(m->d_words + RM_W_TOT, 0, (RM_WORDS - RM_W_TOT) * sizeof(int), m->ctx->stream));
    return PTAM_OK;
}
int rm_words_wait(MapStage& s, ptam_rmap* m, int* h_words) {
    STAGE_TRY(s.down(h_words, m->d_words, RM_WORDS * sizeof(int)));
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}
int rm_refuse(ptam_rmap* m, int table, int row) {
    m->refusal_table = table;
    m->refusal_row = row;
    ptam_set_error("bad argument: ptam_rmap table %d, row %d (found on the device)", table, row);
    return PTAM_E_ARG;
}

int rm_add_points_device(ptam_rmap* m, int src_kf, int target_kf, int target_source, int n_made, const ptam_new_map_point* d_made) {
    const int N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], Q = m->n[RM_N_NEW];
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)M + 2ll * n_made)) return rc;
    if (int rc = rm_room_points(m, (long long)N + n_made)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEW_QUEUE, (long long)Q + n_made)) return rc;
    MtAdd p = mt_add_head(src_kf, target_kf, target_source, M, n_made, N);   // (a, b: found in the resident table by the kernel)
    p.meas = rm_meas(m);
    p.made = d_made;
    p.out = rm_meas_alt(m);
    // the point side: behind the counts
    p.points = rm_points(m) + N;
    p.sources = rm_sources(m) + N;
    p.points3 = rm_points3(m) + (size_t)3 * N;
    p.bad = rm_bad(m) + N;
    p.outlier_count = rm_outlier_count(m) + N;
    p.inlier_count = rm_inlier_count(m) + N;
    p.new_queue = rm_new_queue(m) + Q;
    if (int rc = mt_add_points_core(m->ctx->stream, p)) return rc;
    rm_give_serials(m->ctx->stream, n_made, m->next_serial, rm_serials(m) + N);   // behind the count, like the other rows
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    m->next_serial += n_made;
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->n[RM_N_MEAS] = M + 2 * n_made;
    m->n[RM_N_POINTS] = N + n_made;
    m->n[RM_N_NEW] = Q + n_made;
    return PTAM_OK;
}

// ptam_rmap_refind's work list where the host can walk it, in one wait at most: the caller's (*work), or the resident queue brought
// down into `list` (*work == nullptr; *n_work becomes its length); for NEW_POINTS also bBad of each entry's point, into `bad`
static int rm_refind_work(ptam_rmap* m, int mode, int* n_work, const void** work, std::vector<char>& list, std::vector<uint8_t>& bad) {
    if (mode == PTAM_MAP_REFIND_KEYFRAME) return PTAM_OK;
    const bool from_queue = *work == nullptr, new_points = mode == PTAM_MAP_REFIND_NEW_POINTS;
    if (from_queue) *n_work = m->n[new_points ? RM_N_NEW : RM_N_FAILURE];
    const int n = *n_work;
    if (n == 0 || (!from_queue && !new_points)) return PTAM_OK;
    if (!from_queue)
        for (int e = 0; e < n; e++) ARG_TRY(((const int32_t*)*work)[e] >= 0 && ((const int32_t*)*work)[e] < m->n[RM_N_POINTS]);
    int32_t* d_list;
    uint8_t* d_bad;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver&) {
        d_list = c.piece<int32_t>(from_queue ? 0 : (size_t)n);
        d_bad = c.piece<uint8_t>(new_points ? (size_t)n : 0);
    }));
    if (from_queue) {
        const int w = new_points ? PTAM_RMAP_NEW_QUEUE : PTAM_RMAP_FAILURE;
        list.resize((size_t)n * RM_ROW_BYTES[w]);
        STAGE_TRY(s.down(list.data(), m->t[w].now(), list.size()));
        *work = list.data();
    } else
        STAGE_TRY(s.up(d_list, *work, (size_t)n * 4));
    if (new_points) {
        bad.resize((size_t)n);
        hipLaunchKernelGGL(rm_queue_bad_kernel, dim3(s.blocks(n)), dim3(256), 0, s.st, n, from_queue ? rm_new_queue(m) : d_list, rm_bad(m), d_bad);
        HIP_TRY(hipGetLastError());
        STAGE_TRY(s.down(bad.data(), d_bad, (size_t)n));
    }
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

// ---- what ptam_rmap_refind and ptam_rmap_refind_queue share around mr_core / mr_run
// the handle's tables as the re-find core takes them: the merged tables go into the second buffers
static MrTables rm_refind_tables(ptam_rmap* m) {
    MrTables t = {};
    t.n_kf = m->n[RM_N_KF];
    t.n_points = m->n[RM_N_POINTS];
    t.n_meas = m->n[RM_N_MEAS];
    t.n_never = m->n[RM_N_NEVER];
    t.kfs = m->kfs.data();
    t.d_poses = rm_poses(m);
    t.d_points = rm_points(m);
    t.d_meas = rm_meas(m);
    t.d_never = rm_never(m);
    t.d_meas_merged = rm_meas_alt(m);
    t.d_never_merged = rm_never_alt(m);
    return t;
}
// after the call's wait: the merged tables become the map's
static void rm_refind_commit(ptam_rmap* m, const ptam_map_refind_result& r) {
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->t[PTAM_RMAP_NEVER].cur ^= 1;
    m->n[RM_N_MEAS] += r.n_found;
    m->n[RM_N_NEVER] += r.n_never;
}
// the resident queue was the work: points_consumed entries leave mqNewQueue from the front (:1055); mvFailureQueue is cleared
// unless the call was stopped (:1080)
static int rm_queue_consumed(ptam_rmap* m, int mode, const ptam_map_refind_result& r) {
    if (mode == PTAM_MAP_REFIND_NEW_POINTS && r.points_consumed > 0) {
        const int left = m->n[RM_N_NEW] - r.points_consumed;
        if (left > 0) {
            HIP_TRY(hipMemcpyAsync(rm_new_queue_alt(m), rm_new_queue(m) + r.points_consumed, (size_t)left * 4, hipMemcpyDeviceToDevice, m->ctx->stream));
            HIP_TRY(ptam_stream_wait(m->ctx->stream));
            m->t[PTAM_RMAP_NEW_QUEUE].cur ^= 1;
        }
        m->n[RM_N_NEW] = left;
    }
    if (mode == PTAM_MAP_REFIND_FAILURE_QUEUE && !r.stopped) m->n[RM_N_FAILURE] = 0;
    return PTAM_OK;
}

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
    m->d_init = nullptr;
    m->d_init_bytes = 0;
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
    for (int w = 0; w < RM_TABLES; w++)
        for (int k = 0; k < 2; k++)
            if (m->t[w].buf[k]) (void)hipFree(m->t[w].buf[k]);
    if (m->d_words) (void)hipFree(m->d_words);
    if (m->d_init) (void)hipFree(m->d_init);
    delete m;
    return PTAM_OK;
}

int ptam_rmap_reserve(ptam_rmap* m, int n_kf, int n_points, int n_meas, int n_never, int n_new, int n_failure) {
    ARG_TRY(m);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_new >= 0 && n_failure >= 0);
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int rows[RM_N_COUNTS] = {n_kf, n_points, n_meas, n_never, n_new, n_failure};
    return rm_room_all(m, rows);
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
    if (int rc = rm_room_all(m, rows)) return rc;
    unsigned* owner;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        owner = c.room<unsigned>((size_t)n_points);
        hw = pin.piece<int>(RM_WORDS);
    }));
    hipStream_t st = s.st;

    // ---- up, into the second buffers
    const void* src[PTAM_RMAP_TABLES] = {kf_poses12, kf_fixed, points3, points, sources, bad, outlier_count, inlier_count, meas, never, new_queue, failure};
    for (int w = 0; w < PTAM_RMAP_TABLES; w++) {
        const size_t bytes = (size_t)rows[RM_COUNT_OF[w]] * RM_ROW_BYTES[w];
        if (src[w]) STAGE_TRY(s.up(m->t[w].alt(), src[w], bytes));
        else if (bytes > 0) HIP_TRY(hipMemsetAsync(m->t[w].alt(), 0, bytes, st));   // (the counts, when none are given)
    }
    rm_give_serials(st, n_points, m->next_serial, rm_serials_alt(m));   // every point a fresh serial: a new map to every tracker
    // ---- the checks, one thread per row
    if (int rc = rm_words_reset(m)) return rc;
    int* err = m->d_words;
    if (n_meas > 0)
        hipLaunchKernelGGL((rm_check_sorted_kernel<ptam_map_meas, true>), dim3(s.blocks(n_meas)), dim3(256), 0, st, n_meas, rm_meas_alt(m), n_kf,
                           n_points, err + RM_W_MEAS);
    if (n_never > 0)
        hipLaunchKernelGGL((rm_check_sorted_kernel<ptam_map_pair, false>), dim3(s.blocks(n_never)), dim3(256), 0, st, n_never, rm_never_alt(m), n_kf,
                           n_points, err + RM_W_NEVER);
    if (n_failure > 0)
        hipLaunchKernelGGL(rm_check_pairs_kernel, dim3(s.blocks(n_failure)), dim3(256), 0, st, n_failure, rm_failure_alt(m), n_kf, n_points,
                           err + RM_W_FAILURE);
    if (n_new > 0) {
        HIP_TRY(hipMemsetAsync(owner, 0xff, std::max((size_t)n_points, (size_t)1) * sizeof(unsigned), st));
        hipLaunchKernelGGL(rm_queue_owner_kernel, dim3(s.blocks(n_new)), dim3(256), 0, st, n_new, rm_new_queue_alt(m), n_points, owner, err + RM_W_NEW);
        hipLaunchKernelGGL(rm_queue_repeat_kernel, dim3(s.blocks(n_new)), dim3(256), 0, st, n_new, rm_new_queue_alt(m), n_points, owner, err + RM_W_NEW);
    }
    if (n_points > 0)
        hipLaunchKernelGGL(rm_check_points_kernel, dim3(s.blocks(n_points)), dim3(256), 0, st, n_points, rm_points3_alt(m), rm_points_alt(m),
                           rm_sources_alt(m), rm_bad_alt(m), n_kf, err + RM_W_POINTS);
    HIP_TRY(hipGetLastError());
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    const int order[5][2] = {{RM_W_MEAS, PTAM_RMAP_MEAS}, {RM_W_NEVER, PTAM_RMAP_NEVER}, {RM_W_NEW, PTAM_RMAP_NEW_QUEUE},
                             {RM_W_FAILURE, PTAM_RMAP_FAILURE}, {RM_W_POINTS, PTAM_RMAP_REFIND_POINTS}};
    for (const auto& o : order)
        if (hw[o[0]] != RM_NO_ROW) return rm_refuse(m, o[1], hw[o[0]]);
    // ---- commit
    for (int w = 0; w < RM_TABLES; w++) m->t[w].cur ^= 1;
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
    MapStage s = rm_stage(m);
    STAGE_TRY(s.down(dst, m->t[which].now() + (size_t)first * rb, (size_t)count * rb));
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

int ptam_rmap_bundle_adjust(ptam_rmap* m, const ptam_ba_opts* opts, int mode, const volatile unsigned char* abort_flag,
                            ptam_map_ba_result* res, ptam_map_outlier* outliers, int outlier_cap, int32_t* cam_kf, int32_t* point_ids) {
    ARG_TRY(m && res);
    ARG_TRY(mode == PTAM_MAP_BA_ALL || mode == PTAM_MAP_BA_RECENT);
    ARG_TRY(!outliers || outlier_cap >= m->n[RM_N_MEAS]);
    std::memset(res, 0, sizeof *res);
    if (mode == PTAM_MAP_BA_RECENT && m->n[RM_N_KF] < 8) return PTAM_OK;   // :790-793
    HIP_TRY(hipSetDevice(m->ctx->device));
    MbaTables t = {};
    t.K = m->n[RM_N_KF];
    t.N = m->n[RM_N_POINTS];
    t.M = m->n[RM_N_MEAS];
    t.h_poses = m->h_poses.data();
    t.h_fixed = m->h_fixed.data();
    t.d_poses = rm_poses(m);
    t.d_fixed = rm_fixed(m);
    t.d_points3 = rm_points3(m);
    t.d_meas = rm_meas(m);
    t.d_points = rm_points(m);
    MbaWork w;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) { mba_layout(c, pin, t.K, t.N, t.M, w); }));
    const int rc = mba_core(s, opts, mode, t, w, abort_flag, res, outliers, cam_kf, point_ids);
    if (rc) return rc;
    m->h2d += (unsigned long long)(res->n_adjust + res->n_fixed) * 97;   // the bundle's cameras, pose and flag: copied inside ba_dev_ingest
    // the mirror follows an accepted bundle; the caller fetches the poses with ptam_rmap_download
    if (res->accepted > 0) STAGE_TRY(s.down(m->h_poses.data(), t.d_poses, (size_t)t.K * 96));
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

int ptam_rmap_refind(ptam_rmap* m, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_work, const void* work,
                     const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix,
                     ptam_map_pair* never_out, int out_cap) {
    ARG_TRY(m && finder && res && n_work >= 0 && out_cap >= 0);
    ARG_TRY(mode == PTAM_MAP_REFIND_KEYFRAME || mode == PTAM_MAP_REFIND_NEW_POINTS || mode == PTAM_MAP_REFIND_FAILURE_QUEUE);
    ARG_TRY(work || n_work == 0);
    ARG_TRY(work || mode != PTAM_MAP_REFIND_KEYFRAME);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER];
    if (K == 0) {
        ARG_TRY(n_work == 0 || mode != PTAM_MAP_REFIND_KEYFRAME);
        *res = ptam_map_refind_result{};
        return PTAM_OK;
    }
    if (int rc = mr_check_call(m->ctx, finder, opts, mode, K, m->kfs.data())) return rc;
    HIP_TRY(hipSetDevice(m->ctx->device));
    // the resident queue comes down (4 or 8 bytes an entry, and a bBad byte per new point), because the pair order is the host's
    const bool from_queue = work == nullptr;
    std::vector<char> list;
    std::vector<uint8_t> work_bad;
    if (int rc = rm_refind_work(m, mode, &n_work, &work, list, work_bad)) return rc;
    MrPlan plan;
    ARG_TRY(mr_plan(mode, K, N, n_work, work, [&](int e, int) { return work_bad[(size_t)e] != 0; }, opts ? opts->max_pairs_per_pass : 0, &plan));
    ARG_TRY(plan.bound + M < (1ll << 31) && plan.bound + V < (1ll << 31));
    if (found_out || found_subpix || never_out) {
        ARG_TRY(plan.bound <= (long long)out_cap);
        ARG_TRY(plan.bound == 0 || (found_out && found_subpix && never_out));
    }
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, M + plan.bound)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, V + plan.bound)) return rc;
    ptam_map_refind_result r = mr_plan_nothing(plan, stop_flag && *stop_flag);
    if (plan.pairs > 0) {
        const MrTables t = rm_refind_tables(m);
        MrWork w;
        MapStage s = rm_stage(m);
        STAGE_TRY(s.carve([&](Carver& c, Carver& pin) { mr_layout(c, pin, K, plan, true, w); }));
        STAGE_TRY(mr_core(s, finder, t, plan, w, stop_flag, &r, found_out, found_subpix, never_out));
        HIP_TRY(ptam_stream_wait(s.st));
        rm_refind_commit(m, r);
    }
    if (from_queue)
        if (int rc = rm_queue_consumed(m, mode, r)) return rc;
    *res = r;
    return PTAM_OK;
}

// ptam_rmap_refind(work = NULL) with the work lists built where the queue lies: neither queue comes down, no list goes up.  The
// host learns the count of good new points (one word, one wait), from which pairs, per_pass and the passes follow; the layout is for
// the queue's length, known before.
int ptam_rmap_refind_queue(ptam_rmap* m, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, const volatile unsigned char* stop_flag,
                           ptam_map_refind_result* res) {
    ARG_TRY(m && finder && res);
    ARG_TRY(mode == PTAM_MAP_REFIND_NEW_POINTS || mode == PTAM_MAP_REFIND_FAILURE_QUEUE);
    const int K = m->n[RM_N_KF], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER], Q = m->n[RM_N_NEW], F = m->n[RM_N_FAILURE];
    *res = ptam_map_refind_result{};
    if (K == 0) return PTAM_OK;
    if (int rc = mr_check_call(m->ctx, finder, opts, mode, K, m->kfs.data())) return rc;
    HIP_TRY(hipSetDevice(m->ctx->device));
    const bool new_points = mode == PTAM_MAP_REFIND_NEW_POINTS;
    const int n_work = new_points ? Q : F;
    const long long bound = new_points ? (long long)K * Q : (long long)F;   // the pair count the capacities are held against (mr_plan)
    ARG_TRY(bound < (1ll << 31) && bound + M < (1ll << 31) && bound + V < (1ll << 31));
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, M + bound)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, V + bound)) return rc;
    const int max_per_pass = opts ? opts->max_pairs_per_pass : 0;
    const bool stop_now = stop_flag && *stop_flag;
    ptam_map_refind_result r = {};
    MrShape sh = {};
    sh.mode = mode;
    int n_good = 0;
    if (n_work > 0) {
        sh.n_wp = new_points ? Q : 0;
        sh.n_wq = new_points ? 0 : F;
        sh.pairs = (int)bound;
        sh.per_pass = mr_per_pass(mode, K, max_per_pass, sh.pairs);
        MrWork w;
        int *wentry, *tiles, *d_good, *h_word;
        unsigned long long *keys_a, *keys_b;
        MapStage s = rm_stage(m);
        STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
            mr_layout_shape(c, pin, K, sh, true, w);
            wentry = c.room<int>(new_points ? (size_t)Q : 0);
            tiles = c.room<int>(new_points ? (size_t)mt_tiles(Q) : 0);
            keys_a = c.piece<unsigned long long>((size_t)n_work);
            keys_b = c.piece<unsigned long long>((size_t)n_work);
            d_good = c.piece<int>(1);
            h_word = pin.piece<int>(1);
        }));
        // ---- the work lists, into w.w0 / w.w1
        if (new_points) {
            if (int rc = mt_queue_good_core(s.st, Q, rm_new_queue(m), rm_bad(m), w.w0, wentry, tiles, d_good)) return rc;
            STAGE_TRY(s.down(h_word, d_good, sizeof(int)));
            HIP_TRY(ptam_stream_wait(s.st));
            n_good = *h_word;
            if (n_good < 0 || n_good > Q) {
                ptam_set_error("ptam_rmap_refind_queue: %d good points of %d queue entries", n_good, Q);
                return PTAM_E_STATE;
            }
            if (int rc = mt_queue_rank_core(s.st, n_good, w.w0, w.w1, keys_a, keys_b)) return rc;
            sh.n_wp = n_good;
            sh.pairs = K * n_good;
        } else if (int rc = mt_failure_sorted_core(s.st, F, rm_failure(m), (ptam_map_pair*)w.w0, keys_a, keys_b))
            return rc;
        sh.per_pass = mr_per_pass(mode, K, max_per_pass, sh.pairs);
        if (sh.pairs > 0) {
            const MrTables t = rm_refind_tables(m);
            STAGE_TRY(mr_run(s, finder, t, sh, w, stop_flag, &r, nullptr, nullptr, nullptr));
            // a stopped walk of the new queue: the entries up to the last visited point are popped (mr_plan_consumed), and the
            // entry of that point is the one word of the list the host reads
            const int wp = r.n_pairs / K;
            if (new_points && r.stopped && wp > 0) {
                STAGE_TRY(s.down(h_word, wentry + (wp - 1), sizeof(int)));
                HIP_TRY(ptam_stream_wait(s.st));
                r.points_consumed = *h_word + 1;
                r.n_bad_points = r.points_consumed - wp;
            }
            HIP_TRY(ptam_stream_wait(s.st));
            rm_refind_commit(m, r);
        } else
            r.stopped = new_points && stop_now;   // (mr_plan_nothing)
        if (new_points && !r.stopped) {
            r.points_consumed = Q;
            r.n_bad_points = Q - n_good;
        }
    }
    if (int rc = rm_queue_consumed(m, mode, r)) return rc;
    *res = r;
    return PTAM_OK;
}

int ptam_rmap_apply_global_transform(ptam_rmap* m, const double se3_new_from_old[12], ptam_pvs_point* out_rows) {
    ARG_TRY(m && se3_new_from_old);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS];
    if (K + N == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    char *d_record, *h_record;
    ptam_pvs_point* packed;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_record = c.piece<char>(256);   // the aligner's record
        packed = c.piece<ptam_pvs_point>(out_rows ? (size_t)N : 0);
        h_record = pin.piece<char>(256);
    }));
    // poses: into the second buffer; points3 in place, the pixel vectors (pv.world among them) into the point rows: nothing refuses
    // the call once the kernel runs
    STAGE_TRY(map_transform_core(s, d_record, h_record, se3_new_from_old, K, rm_poses(m), rm_poses_alt(m), N, rm_points3(m), rm_sources(m),
                                 (ptam_pvs_point*)rm_points(m), (int)sizeof(ptam_map_refind_point)));
    STAGE_TRY(s.down(m->h_poses.data(), rm_poses_alt(m), (size_t)K * 96));   // the mirror
    if (out_rows && N > 0) {
        hipLaunchKernelGGL(rm_pack_pvs_kernel, dim3(s.blocks(N)), dim3(256), 0, s.st, N, rm_points(m), packed);
        HIP_TRY(hipGetLastError());
        STAGE_TRY(s.down(out_rows, packed, (size_t)N * sizeof(ptam_pvs_point)));
    }
    HIP_TRY(ptam_stream_wait(s.st));
    m->t[PTAM_RMAP_KF_POSES].cur ^= 1;
    return PTAM_OK;
}

int ptam_rmap_apply_outliers(ptam_rmap* m, int n_outliers, const ptam_map_outlier* outliers, ptam_map_outliers_result* res) {
    ARG_TRY(m && res && n_outliers >= 0 && (n_outliers == 0 || outliers));
    const int n_meas = m->n[RM_N_MEAS], n_never = m->n[RM_N_NEVER], n_failure = m->n[RM_N_FAILURE];
    ARG_TRY((long long)n_never + n_outliers < (1ll << 31) && (long long)n_failure + n_outliers < (1ll << 31));
    ptam_map_outliers_result r;   // what the list alone decides; the rest is looked at on the device
    ARG_TRY(mc_outliers_tally(n_outliers, outliers, n_meas, nullptr, n_never, nullptr, n_failure, &r) < 0);
    if (n_outliers == 0) {
        *res = r;
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(m->ctx->device));
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, r.n_never_out)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_FAILURE, (long long)n_failure + n_outliers)) return rc;   // (the compaction's room, not only its count)

    const size_t Mz = (size_t)n_meas, Oz = (size_t)n_outliers;
    MtOutliersDev d = {};
    d.n_meas = n_meas;
    d.n_never = n_never;
    d.n_outliers = n_outliers;
    d.n_never_out = r.n_never_out;
    ptam_map_outlier* d_outl;
    unsigned* owner;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d.outliers = d_outl = c.piece<ptam_map_outlier>(Oz);
        d.flag = c.piece<uint8_t>(Mz);   // (n_meas > 0: an outlier names a row)
        owner = c.piece<unsigned>(Mz);
        d.tiles = c.piece<int>((size_t)mt_tiles(std::max(n_meas, n_outliers)));
        d.new_never = c.piece<ptam_map_pair>(Oz);
        hw = pin.piece<int>(RM_WORDS);
    }));
    hipStream_t st = s.st;
    STAGE_TRY(s.up(d_outl, outliers, Oz * sizeof(ptam_map_outlier)));
    if (int rc = rm_words_reset(m)) return rc;
    HIP_TRY(hipMemsetAsync(owner, 0xff, Mz * sizeof(unsigned), st));
    int* err = m->d_words + RM_W_CALL;
    hipLaunchKernelGGL(rm_outliers_check_kernel, dim3(s.blocks(n_outliers)), dim3(256), 0, st, n_outliers, d.outliers, rm_meas(m), n_never, rm_never(m),
                       owner, err);
    hipLaunchKernelGGL(rm_outliers_twice_kernel, dim3(s.blocks(n_outliers)), dim3(256), 0, st, n_outliers, d.outliers, owner, err);
    d.meas = rm_meas(m);
    d.never = rm_never(m);
    d.bad = rm_bad(m);
    d.points = rm_points(m);
    d.gate = err;
    d.tot = m->d_words + RM_W_TOT;
    d.meas_out = rm_meas_alt(m);
    d.never_out = rm_never_alt(m);
    d.failure_new = rm_failure(m) + n_failure;   // behind the count
    if (int rc = mt_apply_outliers_core(st, d)) return rc;
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    if (hw[RM_W_CALL] != RM_NO_ROW) return rm_refuse(m, PTAM_RMAP_OUTLIERS, hw[RM_W_CALL]);
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->t[PTAM_RMAP_NEVER].cur ^= 1;
    m->n[RM_N_MEAS] = r.n_meas_out;
    m->n[RM_N_NEVER] = r.n_never_out;
    m->n[RM_N_FAILURE] = r.n_failure_out;
    *res = r;
    return PTAM_OK;
}

// ptam_rmap_bundle_adjust, then ptam_rmap_apply_outliers on the list mba_route_kernel left in the bundle's work memory: the list
// is neither brought down nor sent up.  What the host read off the list there — the counts per action — a kernel adds up here; the
// action and row ranges need no check, mba_route_kernel writes a row of the selection and one of the three actions in every entry.
int ptam_rmap_bundle_adjust_routed(ptam_rmap* m, const ptam_ba_opts* opts, int mode, const volatile unsigned char* abort_flag,
                                   ptam_map_ba_result* res, ptam_map_outliers_result* outliers_res) {
    ARG_TRY(m && res && outliers_res);
    ARG_TRY(mode == PTAM_MAP_BA_ALL || mode == PTAM_MAP_BA_RECENT);
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER], F = m->n[RM_N_FAILURE];
    std::memset(res, 0, sizeof *res);
    ptam_map_outliers_result r = {};   // of an empty list, until the bundle has routed one
    r.n_meas_out = M;
    r.n_never_out = V;
    r.n_failure_out = F;
    *outliers_res = r;
    if (mode == PTAM_MAP_BA_RECENT && K < 8) return PTAM_OK;   // :790-793
    HIP_TRY(hipSetDevice(m->ctx->device));
    MbaTables t = {};
    t.K = K;
    t.N = N;
    t.M = M;
    t.h_poses = m->h_poses.data();
    t.h_fixed = m->h_fixed.data();
    t.d_poses = rm_poses(m);
    t.d_fixed = rm_fixed(m);
    t.d_points3 = rm_points3(m);
    t.d_meas = rm_meas(m);
    t.d_points = rm_points(m);
    // the outlier stage's work beside the bundle's, in the call's one carve: a bundle has at most M outliers
    const size_t Mz = (size_t)std::max(M, 1);
    MbaWork w;
    MtOutliersDev d = {};
    unsigned* owner;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        mba_layout(c, pin, K, N, M, w);
        d.flag = c.piece<uint8_t>(Mz);
        owner = c.piece<unsigned>(Mz);
        d.tiles = c.piece<int>((size_t)mt_tiles((int)Mz));
        d.new_never = c.piece<ptam_map_pair>(Mz);
        hw = pin.piece<int>(RM_WORDS);
    }));
    const size_t hw_off = (size_t)((char*)hw - (char*)m->ctx->h_pinned);
    int n_out = 0;
    if (int rc = mba_core(s, opts, mode, t, w, abort_flag, res, nullptr, nullptr, nullptr, &n_out)) return rc;
    m->h2d += (unsigned long long)(res->n_adjust + res->n_fixed) * 97;   // the bundle's cameras, pose and flag: copied inside ba_dev_ingest
    if (res->accepted > 0) STAGE_TRY(s.down(m->h_poses.data(), t.d_poses, (size_t)K * 96));   // the mirror, whatever the outlier stage decides
    if (n_out == 0) {
        HIP_TRY(ptam_stream_wait(s.st));
        return PTAM_OK;
    }
    // ---- the outlier stage.  n_out has been on the host since Compute() returned: the room of both tables before its launches
    ARG_TRY((long long)V + n_out < (1ll << 31) && (long long)F + n_out < (1ll << 31));
    if (int rc = rm_room(m, PTAM_RMAP_NEVER, (long long)V + n_out)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_FAILURE, (long long)F + n_out)) return rc;
    // the words' landing place is a piece of the call's pinned layout.  mba_core has asked the context for pinned memory since (the
    // step ends, a request of its own): had that grown the block, it waited for the stream, and the piece lies at its offset in the
    // new, larger block
    hw = (int*)((char*)m->ctx->h_pinned + hw_off);
    hipStream_t st = s.st;
    if (int rc = rm_words_reset(m)) return rc;
    HIP_TRY(hipMemsetAsync(owner, 0xff, Mz * sizeof(unsigned), st));
    int* err = m->d_words + RM_W_CALL;
    d.n_meas = M;
    d.n_never = V;
    d.n_outliers = n_out;
    d.n_never_out = V + n_out;   // (the merge's launch bound: its kernel reads the live count of new pairs on the device)
    d.outliers = w.out;
    hipLaunchKernelGGL(rm_outliers_tally_kernel, dim3(s.blocks(n_out)), dim3(256), 0, st, n_out, d.outliers, m->d_words + RM_W_TALLY);
    hipLaunchKernelGGL(rm_outliers_check_kernel, dim3(s.blocks(n_out)), dim3(256), 0, st, n_out, d.outliers, rm_meas(m), V, rm_never(m), owner, err);
    hipLaunchKernelGGL(rm_outliers_twice_kernel, dim3(s.blocks(n_out)), dim3(256), 0, st, n_out, d.outliers, owner, err);
    d.meas = rm_meas(m);
    d.never = rm_never(m);
    d.bad = rm_bad(m);
    d.points = rm_points(m);
    d.gate = err;
    d.tot = m->d_words + RM_W_TOT;
    d.meas_out = rm_meas_alt(m);
    d.never_out = rm_never_alt(m);
    d.failure_new = rm_failure(m) + F;   // behind the count
    if (int rc = mt_apply_outliers_core(st, d)) return rc;
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    if (hw[RM_W_CALL] != RM_NO_ROW) return rm_refuse(m, PTAM_RMAP_OUTLIERS, hw[RM_W_CALL]);
    r.n_point_bad = hw[RM_W_TALLY + 0];
    r.n_failure_added = hw[RM_W_TALLY + 1];
    r.n_never_added = hw[RM_W_TALLY + 2];
    r.n_meas_out = M - r.n_failure_added - r.n_never_added;
    r.n_never_out = V + r.n_never_added;
    r.n_failure_out = F + r.n_failure_added;
    m->t[PTAM_RMAP_MEAS].cur ^= 1;
    m->t[PTAM_RMAP_NEVER].cur ^= 1;
    m->n[RM_N_MEAS] = r.n_meas_out;
    m->n[RM_N_NEVER] = r.n_never_out;
    m->n[RM_N_FAILURE] = r.n_failure_out;
    *outliers_res = r;
    return PTAM_OK;
}

int ptam_rmap_handle_bad_points(ptam_rmap* m, ptam_map_bad_points_result* res, int32_t* kept_out, int32_t* new_index_out) {
    ARG_TRY(m && res);
    HIP_TRY(hipSetDevice(m->ctx->device));
    const int N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS], V = m->n[RM_N_NEVER], Q = m->n[RM_N_NEW], F = m->n[RM_N_FAILURE];
    const size_t Nz = (size_t)N;
    MtBadDev d = {};
    d.n_points = N;
    d.n_meas = M;
    d.n_never = V;
    d.n_new = Q;
    d.n_failure = F;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d.removed = c.room<uint8_t>(Nz);
        d.tiles = c.room<int>((size_t)mt_tiles(std::max(std::max(N, M), std::max(std::max(V, Q), F))));
        d.new_index = c.room<int32_t>(Nz);
        d.kept = c.room<int32_t>(Nz);
        hw = pin.piece<int>(RM_WORDS);
    }));
    if (int rc = rm_words_reset(m)) return rc;
    d.bad = rm_bad(m);
    d.outlier_count = rm_outlier_count(m);
    d.inlier_count = rm_inlier_count(m);
    d.meas = rm_meas(m);
    d.never = rm_never(m);
    d.new_queue = rm_new_queue(m);
    d.failure = rm_failure(m);
    d.tot = m->d_words + RM_W_TOT;
    d.meas_out = rm_meas_alt(m);
    d.never_out = rm_never_alt(m);
    d.new_out = rm_new_queue_alt(m);
    d.failure_out = rm_failure_alt(m);
    // the point-side tables, all compacted (the serials in order, so still strictly increasing); a survivor's bad byte is 0 (it
    // would not have survived)
    for (int w = 0; w < RM_TABLES; w++)
        if (rm_point_side(w) && w != PTAM_RMAP_BAD) {
            d.col_in[d.n_columns] = m->t[w].now();
            d.col_out[d.n_columns] = m->t[w].alt();
            d.col_dwords[d.n_columns++] = (int)(RM_ROW_BYTES[w] / 4);
        }
    if (N > 0) HIP_TRY(hipMemsetAsync(rm_bad_alt(m), 0, Nz, s.st));
    if (int rc = mt_handle_bad_points_core(s.st, d)) return rc;
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    const ptam_map_bad_points_result r = mt_bad_result(hw + RM_W_TOT, N, Q);
    for (int w = PTAM_RMAP_POINTS3; w < RM_TABLES; w++) m->t[w].cur ^= 1;   // every table but the keyframes'
    m->n[RM_N_POINTS] = r.n_kept;
    m->n[RM_N_MEAS] = r.n_meas_out;
    m->n[RM_N_NEVER] = r.n_never_out;
    m->n[RM_N_NEW] = r.n_new_out;
    m->n[RM_N_FAILURE] = r.n_failure_out;
    if (kept_out || new_index_out) {   // (the scratch is untouched until the next call)
        if (kept_out) STAGE_TRY(s.down(kept_out, d.kept, (size_t)r.n_kept * 4));
        if (new_index_out) STAGE_TRY(s.down(new_index_out, d.new_index, Nz * 4));
        HIP_TRY(ptam_stream_wait(s.st));
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
    ptam_new_map_point* d_made;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver&) { d_made = c.piece<ptam_new_map_point>((size_t)n_made); }));
    STAGE_TRY(s.up(d_made, made, (size_t)n_made * sizeof(ptam_new_map_point)));
    return rm_add_points_device(m, src_kf, target_kf, target_source, n_made, d_made);
}

int ptam_rmap_note_tracked(ptam_rmap* m, int n, const int32_t* points, const uint8_t* outlier_flags) {
    ARG_TRY(m && n >= 0 && (n == 0 || (points && outlier_flags)));
    const int N = m->n[RM_N_POINTS];
    for (int i = 0; i < n; i++) ARG_TRY(points[i] >= 0 && points[i] < N);
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    int32_t* d_points;
    uint8_t* d_flags;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver&) {
        d_points = c.piece<int32_t>((size_t)n);
        d_flags = c.piece<uint8_t>((size_t)n);
    }));
    STAGE_TRY(s.up(d_points, points, (size_t)n * 4));
    STAGE_TRY(s.up(d_flags, outlier_flags, (size_t)n));
    hipLaunchKernelGGL(rm_note_tracked_kernel, dim3(s.blocks(n)), dim3(256), 0, s.st, n, d_points, d_flags, rm_outlier_count(m), rm_inlier_count(m));
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

int ptam_rmap_scene_depth(ptam_rmap* m, ptam_scene_depth* out) {
    ARG_TRY(m);
    const int K = m->n[RM_N_KF];
    ARG_TRY(K == 0 || out);
    if (K == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    ptam_scene_depth* h_out;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver&, Carver& pin) { h_out = pin.piece<ptam_scene_depth>((size_t)K); }));
    STAGE_TRY(map_scene_depth_core(s, K, rm_poses(m), rm_points3(m), m->n[RM_N_MEAS], rm_meas(m), h_out, out));
    m->d2h += (size_t)K * sizeof(ptam_scene_depth);   // (written by the kernel into host-mapped memory)
    return PTAM_OK;
}

}   // extern "C"

void maprmap_preload_kernels() {
    ptam_preload((const void*)rm_check_sorted_kernel<ptam_map_meas, true>);
    ptam_preload((const void*)rm_check_sorted_kernel<ptam_map_pair, false>);
    ptam_preload((const void*)rm_check_pairs_kernel);
    ptam_preload((const void*)rm_queue_owner_kernel);
    ptam_preload((const void*)rm_queue_repeat_kernel);
    ptam_preload((const void*)rm_check_points_kernel);
    ptam_preload((const void*)rm_outliers_check_kernel);
    ptam_preload((const void*)rm_outliers_twice_kernel);
    ptam_preload((const void*)rm_outliers_tally_kernel);
    ptam_preload((const void*)rm_note_tracked_kernel);
    ptam_preload((const void*)rm_queue_bad_kernel);
    ptam_preload((const void*)rm_pack_pvs_kernel);
}
