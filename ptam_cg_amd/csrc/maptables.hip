// maptables.hip — the edits of the map tables between the ptam_map_* calls, each as one call on the tables (ptam_hip.h):
//   ptam_map_apply_outliers     the outlier loop of MapMaker::BundleAdjust (src/MapMaker.cc:916-932)
//   ptam_map_handle_bad_points  MapMaker::HandleBadPoints (:131-153) with Map::MoveBadPointsToTrash (src/Map.cc:20-30)
//   ptam_map_add_points         the table side of AddPointEpipolar (:670-685) and of InitFromStereo's point loop (:352-362)
// and, for ptam_rmap_init_from_stereo (maprmap_init.hip), mt_made_records_core: the made records of InitFromStereo's point loop
// (:310-367) compacted in match order, with the count of every status; and, for ptam_rmap_refind_queue (maprmap.hip), the work lists
// of the re-find built from the resident queues: the good new points compacted in queue order and ranked by index, the failure
// pairs sorted — both through one sort of 64-bit keys (mt_sort_keys: a bitonic sort per tile in LDS, then merge passes by rank).
// All three set a flag per row, compact or merge the rows in order and remap the point column.  The one primitive is the ordered
// compaction mt_compact over a row source (keep / put / drop), three launches:
//   mt_count_kernel    one workgroup per tile of MT_TILE = 1024 rows, one row per thread: __ballot / __popcll per 64-lane wave,
//                      the 16 wave counts summed through LDS -> the tile's count
//   mt_scan_kernel     one workgroup: the tile counts -> exclusive offsets and the total, MT_SCAN_CHUNK = 1024 tile counts per
//                      round with the running sum carried from round to round (it walks the tile counts, not the table)
//   mt_scatter_kernel  the tiling of mt_count_kernel again: row -> tile offset + offset inside the tile
// No atomic decides where a row lands; the only atomics of the file add up counts (n_marked, the point loop's status counts).
// Sizes at which the compaction changes path (tests/test_gpu_map_edit.py runs n - 1, n, n + 1 of each):
//   64          rows: a second wave inside the tile
//   1024        rows (MT_TILE): a second workgroup
//   1024 * 1024 rows (MT_TILE * MT_SCAN_CHUNK): a second round of the tile-count scan
// The scan has no capacity of its own: any table of fewer than 2^31 rows is taken.
// Each entry is a host front that checks the tables and uploads them into the context's scratch, a core that takes device pointers
// and only enqueues (mt_*_core, maptables_internal.h) and a host back that downloads; the resident forms ptam_rmap_* (maprmap.hip)
// hand the same cores the tables a ptam_rmap keeps on the device.
#include <algorithm>

#include "maptables_internal.h"

__device__ __forceinline__ unsigned long long mt_key(int kf, int point) {   // (indices are >= 0: one unsigned compare orders (kf, point))
    return ((unsigned long long)(unsigned)kf << 32) | (unsigned)point;
}

// ---- the ordered compaction ----------------------------------------------------------------------------------------------------
// the thread's place among the tile's kept rows, in thread order, and the tile's count
__device__ __forceinline__ int mt_tile_offset(bool keep, int tid, int* ws, int& total) {
    const unsigned long long m = __ballot(keep);
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) ws[wid] = __popcll(m);
    __syncthreads();
    int off = __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
    for (int w = 0; w < MT_TILE / 64; w++) {
        const int c = ws[w];
        if (w < wid) off += c;
        total += c;
    }
    return off;
}

template <class Src>
__global__ void __launch_bounds__(MT_TILE) mt_count_kernel(Src s, int n, int* __restrict__ tile_cnt) {
    __shared__ int ws[MT_TILE / 64];
    const long long i = (long long)blockIdx.x * MT_TILE + threadIdx.x;
    const bool keep = i < n && s.keep((int)i);
    int total;
    mt_tile_offset(keep, threadIdx.x, ws, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(MT_SCAN_CHUNK) mt_scan_kernel(int n_tiles, int* __restrict__ tile_cnt, int* __restrict__ total_out) {
    __shared__ int ws[MT_SCAN_CHUNK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int run = 0;
    for (int b0 = 0; b0 < n_tiles; b0 += MT_SCAN_CHUNK) {
        const int t = b0 + tid;
        const int c = t < n_tiles ? tile_cnt[t] : 0;
        const int inc = wave_incl_scan_i32(c);
        __syncthreads();   // (the previous round's sums have been read)
        if (lane == 63) ws[wid] = inc;
        __syncthreads();
        int off = inc - c, tot = 0;
        for (int w = 0; w < MT_SCAN_CHUNK / 64; w++) {
            if (w < wid) off += ws[w];
            tot += ws[w];
        }
        if (t < n_tiles) tile_cnt[t] = run + off;
        run += tot;
    }
    if (tid == 0) *total_out = run;
}

template <class Src>
__global__ void __launch_bounds__(MT_TILE) mt_scatter_kernel(Src s, int n, const int* __restrict__ tile_off) {
    __shared__ int ws[MT_TILE / 64];
    const long long i = (long long)blockIdx.x * MT_TILE + threadIdx.x;
    const bool keep = i < n && s.keep((int)i);
    int total;
    const int off = mt_tile_offset(keep, threadIdx.x, ws, total);
    if (i >= n) return;
    if (keep) s.put((int)i, tile_off[blockIdx.x] + off);
    else s.drop((int)i);
}

// rows [0, n) of s, kept ones in order; *total (zeroed by the caller) = how many.  tile_cnt: room for mt_tiles(n)
template <class Src>
static void mt_compact(hipStream_t st, const Src& s, int n, int* tile_cnt, int* total) {
    if (n == 0) return;
    const int tiles = mt_tiles(n);
    hipLaunchKernelGGL(mt_count_kernel<Src>, dim3(tiles), dim3(MT_TILE), 0, st, s, n, tile_cnt);
    hipLaunchKernelGGL(mt_scan_kernel, dim3(1), dim3(MT_SCAN_CHUNK), 0, st, tiles, tile_cnt, total);
    hipLaunchKernelGGL(mt_scatter_kernel<Src>, dim3(tiles), dim3(MT_TILE), 0, st, s, n, (const int*)tile_cnt);
}

// ---- the row sources -----------------------------------------------------------------------------------------------------------
struct MtUnflaggedRows {   // the measurement rows no outlier erases
    const uint8_t* flag;
    const ptam_map_meas* in;
    ptam_map_meas* out;
    __device__ bool keep(int i) const { return flag[i] == 0; }
    __device__ void put(int i, int at) const { out[at] = in[i]; }
    __device__ void drop(int) const {}
};
struct MtNeverRows {   // the rows flagged NEVER_RETRY, as pairs: sorted, because they are rows of a sorted table
    const uint8_t* flag;
    const ptam_map_meas* in;
    ptam_map_pair* out;
    __device__ bool keep(int i) const { return flag[i] == PTAM_MAP_OUT_NEVER_RETRY; }
    __device__ void put(int i, int at) const {
        ptam_map_pair q;
        q.kf = in[i].kf;
        q.point = in[i].point;
        out[at] = q;
    }
    __device__ void drop(int) const {}
};
struct MtFailureOutliers {   // the outliers that go to the failure queue, in list order
    const ptam_map_outlier* in;
    ptam_map_pair* out;
    __device__ bool keep(int i) const { return in[i].action == PTAM_MAP_OUT_FAILURE_QUEUE; }
    __device__ void put(int i, int at) const {
        ptam_map_pair q;
        q.kf = in[i].kf;
        q.point = in[i].point;
        out[at] = q;
    }
    __device__ void drop(int) const {}
};
struct MtPoints {   // the exclusive scan over the points: new_index and kept
    const uint8_t* removed;
    int32_t* new_index;
    int32_t* kept;
    __device__ bool keep(int i) const { return removed[i] == 0; }
    __device__ void put(int i, int at) const {
        new_index[i] = at;
        kept[at] = i;
    }
    __device__ void drop(int i) const { new_index[i] = -1; }
};
template <class Row>
struct MtRemapRows {   // the rows of surviving points, `point` rewritten (ptam_map_meas, ptam_map_pair)
    const int32_t* new_index;
    const Row* in;
    Row* out;
    __device__ bool keep(int i) const { return new_index[in[i].point] >= 0; }
    __device__ void put(int i, int at) const {
        Row r = in[i];
        r.point = new_index[r.point];
        out[at] = r;
    }
    __device__ void drop(int) const {}
};
struct MtRemapQueue {   // mqNewQueue
    const int32_t* new_index;
    const int32_t* in;
    int32_t* out;
    __device__ bool keep(int i) const { return new_index[in[i]] >= 0; }
    __device__ void put(int i, int at) const { out[at] = new_index[in[i]]; }
    __device__ void drop(int) const {}
};
struct MtMadeRecords {   // InitFromStereo's point loop: the records whose status is PTAM_INIT_MADE, in match order
    const int32_t* status;
    const ptam_new_map_point* in;
    ptam_new_map_point* out;
    __device__ bool keep(int i) const { return status[i] == PTAM_INIT_MADE; }
    __device__ void put(int i, int at) const { out[at] = in[i]; }
    __device__ void drop(int) const {}
};

// ---- the kernels around it -----------------------------------------------------------------------------------------------------
// :916-932, one thread per outlier: the row's flag (no row is named twice) and bBad (the same byte may be set more than once).
// gate (nullable): the word in which the kernels launched before this one have published a refusal; then nothing is written
__global__ void __launch_bounds__(256) mt_outliers_kernel(int n, const ptam_map_outlier* __restrict__ o, uint8_t* __restrict__ flag,
                                                           uint8_t* __restrict__ bad, ptam_map_refind_point* __restrict__ points,
                                                           const int* __restrict__ gate) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (gate && *gate != MT_GATE_OPEN)) return;
    const ptam_map_outlier r = o[i];
    if (r.action == PTAM_MAP_OUT_POINT_BAD) {
        bad[r.point] = 1;
        if (points) points[r.point].bad = 1;
    } else
        flag[r.meas] = (uint8_t)r.action;
}

// out = A (sorted) merged with B (sorted, *nB_ptr rows); no key is in both: each row placed by a binary search in the other list
// (the rule of maprefind.hip's mr_merge_kernel)
__global__ void __launch_bounds__(256) mt_merge_kernel(int nA, const ptam_map_pair* __restrict__ A, const int* __restrict__ nB_ptr,
                                                        const ptam_map_pair* __restrict__ B, ptam_map_pair* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nB = *nB_ptr;
    if (t >= (long long)nA + nB) return;
    const bool fromA = t < nA;
    const int j = fromA ? (int)t : (int)(t - nA);
    const ptam_map_pair r = fromA ? A[j] : B[j];
    const ptam_map_pair* other = fromA ? B : A;
    const unsigned long long key = mt_key(r.kf, r.point);
    int lo = 0, hi = fromA ? nB : nA;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (mt_key(other[mid].kf, other[mid].point) < key) lo = mid + 1;
        else hi = mid;
    }
    out[(size_t)j + (size_t)lo] = r;
}

// :136, one thread per point
__global__ void __launch_bounds__(256) mt_mark_kernel(int n, const uint8_t* __restrict__ bad, const int32_t* __restrict__ n_out,
                                                       const int32_t* __restrict__ n_in, uint8_t* __restrict__ removed, int* __restrict__ n_marked) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool b = false, m = false;
    if (i < n) {
        b = bad && bad[i] != 0;
        m = n_out && n_out[i] > 20 && n_out[i] > n_in[i];
        removed[i] = b || m;
    }
    const unsigned long long newly = __ballot(m && !b);
    if ((threadIdx.x & 63) == 0 && newly) atomicAdd(n_marked, __popcll(newly));
}

// a point-side column, survivors to the front: threads over (surviving row, dword)
__global__ void __launch_bounds__(256) mt_gather_kernel(const int* __restrict__ n_kept_ptr, const int32_t* __restrict__ kept, int dwords,
                                                         const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const long long total = (long long)*n_kept_ptr * dwords, step = (long long)gridDim.x * 256;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += step) {
        const long long j = t / dwords;
        out[t] = in[(long long)kept[j] * dwords + (t - j * dwords)];
    }
}

// the end of keyframe kf's run in the sorted table (an upper bound on kf alone)
__device__ __forceinline__ int mt_run_end(const ptam_map_meas* __restrict__ m, int n, int kf) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (m[mid].kf <= kf) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// :673-682 / :352-362, one thread per output row: meas[0, a) | the lower keyframe's new rows | meas[a, b) | the higher one's | meas[b, n)
__global__ void __launch_bounds__(256) mt_add_rows_kernel(MtAdd p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.n_meas + 2ll * p.n_made) return;
    if (p.a < 0) {   // (the same for every thread: the two searches read ~20 cached rows each)
        p.a = mt_run_end(p.meas, p.n_meas, p.kf_lo);
        p.b = mt_run_end(p.meas, p.n_meas, p.kf_hi);
    }
    int old_row = -1, made_row = 0, lo = 0;
    if (t < p.a) old_row = (int)t;
    else if (t < (long long)p.a + p.n_made) made_row = (int)(t - p.a), lo = 1;
    else if (t < (long long)p.b + p.n_made) old_row = (int)(t - p.n_made);
    else if (t < (long long)p.b + 2ll * p.n_made) made_row = (int)(t - p.b - p.n_made);
    else old_row = (int)(t - 2ll * p.n_made);
    ptam_map_meas m;
    if (old_row >= 0) m = p.meas[old_row];
    else {
        const ptam_new_map_point& q = p.made[made_row];
        const bool src = lo == p.src_is_lo;
        m.kf = lo ? p.kf_lo : p.kf_hi;
        m.point = p.n_points + made_row;
        m.level = q.level;
        m.source = src ? (int)PTAM_MAP_SRC_ROOT : p.target_source;
        m.root_pos[0] = src ? q.src_root_pos[0] : q.target_pos[0];
        m.root_pos[1] = src ? q.src_root_pos[1] : q.target_pos[1];
    }
    p.out[t] = m;
}
// :651-666, one thread per new point: the point-side rows
__global__ void __launch_bounds__(256) mt_add_points_kernel(MtAdd p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_made) return;
    const ptam_new_map_point& q = p.made[i];
    if (p.points) {
        ptam_map_refind_point r;
        r.pv = q.point;
        r.src_kf = p.src_kf;
        r.src_level = q.level;
        r.center_x = q.center_x;
        r.center_y = q.center_y;
        r.bad = 0;
        r.pad_ = 0;
        p.points[i] = r;
    }
    if (p.sources) {
        ptam_map_point_source s;
        s.src_kf = p.src_kf;
        s.pad_ = 0;
        for (int j = 0; j < 3; j++) {
            s.center_nc[j] = q.center_nc[j];
            s.one_right_nc[j] = q.one_right_nc[j];
            s.one_down_nc[j] = q.one_down_nc[j];
        }
        p.sources[i] = s;
    }
    if (p.points3)
        for (int j = 0; j < 3; j++) p.points3[(size_t)3 * i + j] = q.point.world[j];
    if (p.bad) p.bad[i] = 0;
    if (p.outlier_count) p.outlier_count[i] = 0;
    if (p.inlier_count) p.inlier_count[i] = 0;
    if (p.new_queue) p.new_queue[i] = p.n_points + i;
}

// one thread per match: how many of each status 0..3 (a ballot per status and wave, one integer atomicAdd per wave and status
// that occurs: exact in any order).  counts: four ints, zeroed by the caller
__global__ void __launch_bounds__(256) mt_status_count_kernel(int n, const int32_t* __restrict__ status, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int code = i < n ? status[i] : -1;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const unsigned long long mk = __ballot(code == c);
        if ((threadIdx.x & 63) == 0 && mk) atomicAdd(counts + c, __popcll(mk));
    }
}

// ---- the sort of 64-bit keys -----------------------------------------------------------------------------------------------------
// Ascending, for the work lists of the re-find from the resident queues: (kf << 32 | point) of a failure pair, (point << 32 | place)
// of a good new point.  Equal keys are equal records, so no tie can change a byte: the output is a function of the input alone.
//   mt_sort_tile_kernel   one workgroup of MT_TILE threads per tile of MT_TILE keys, one key per thread, a bitonic network: the
//                         exchanges at a distance below 64 are lane exchanges inside the wave, the others go through LDS (8 KB a
//                         workgroup; thread t reads slot t ^ distance, distance >= 64: each 32-lane half reads 32 consecutive
//                         8-byte slots, one 256-byte bank row, so no two lanes of a half meet on a bank).  A short last tile is
//                         filled with ~0, above every key (a key's top bit is clear)
//   mt_sort_merge_kernel  one pass per doubling of the run length, one thread per key: runs 2j and 2j + 1 into one, each key placed
//                         by a binary search in the sibling run (the left run's keys before equal keys of the right run: the count
//                         of smaller keys for a left key, of smaller or equal keys for a right one) — the rule of mt_merge_kernel
// Sizes at which the path changes: 64 keys (a second wave), MT_TILE (a second tile: the first merge pass), 2 MT_TILE (a second pass).
__global__ void __launch_bounds__(MT_TILE) mt_sort_tile_kernel(int n, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long ks[MT_TILE];
    const int tid = threadIdx.x;
    const long long g = (long long)blockIdx.x * MT_TILE + tid;
    unsigned long long v = g < n ? in[g] : ~0ull;
    for (int size = 2; size <= MT_TILE; size <<= 1)
        for (int dist = size >> 1; dist > 0; dist >>= 1) {
            unsigned long long o;
            if (dist >= 64) {   // (the same for every thread)
                ks[tid] = v;
                __syncthreads();
                o = ks[tid ^ dist];
                __syncthreads();
            } else
                o = __shfl_xor(v, dist, 64);
            const bool lower = (tid & dist) == 0, ascending = (tid & size) == 0;
            v = (lower == ascending) ? (v < o ? v : o) : (v < o ? o : v);
        }
    if (g < n) out[g] = v;
}

__global__ void __launch_bounds__(256) mt_sort_merge_kernel(int n, int run, const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const long long base = g / (2ll * run) * (2ll * run), mid = base + run;
    const bool right = g >= mid;
    // the sibling run, cut at the table's end (a left run without a sibling: empty)
    long long lo = right ? base : (mid < n ? mid : (long long)n), hi = right ? mid : (mid + run < n ? mid + run : (long long)n);
    const long long sib = lo;
    const unsigned long long key = in[g];
    while (lo < hi) {
        const long long m = lo + (hi - lo) / 2;
        if (right ? in[m] <= key : in[m] < key) lo = m + 1;
        else hi = m;
    }
    out[base + (g - (right ? mid : base)) + (lo - sib)] = key;
}

// n keys in a, ascending, into a or b (n keys of room each): the buffer that holds them (maptables_internal.h)
unsigned long long* mt_sort_keys(hipStream_t st, int n, unsigned long long* a, unsigned long long* b) {
    if (n == 0) return a;
    hipLaunchKernelGGL(mt_sort_tile_kernel, dim3(mt_tiles(n)), dim3(MT_TILE), 0, st, n, (const unsigned long long*)a, b);
    unsigned long long *src = b, *dst = a;
    for (long long run = MT_TILE; run < n; run *= 2) {
        hipLaunchKernelGGL(mt_sort_merge_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, st, n, (int)run,
                           (const unsigned long long*)src, dst);
        std::swap(src, dst);
    }
    return src;
}

// ---- the work lists of the re-find, from the resident queues (MapMaker::ReFindNewlyMade / ReFindFromFailureQueue, :1048-1081) -------
struct MtGoodQueue {   // mqNewQueue's entries whose point is not bad (:1056-1059), in queue order: the point and the entry
    const int32_t* q;
    const uint8_t* bad;
    int* wpts;
    int* wentry;
    __device__ bool keep(int i) const { return bad[q[i]] == 0; }
    __device__ void put(int i, int at) const {
        wpts[at] = q[i];
        wentry[at] = i;
    }
    __device__ void drop(int) const {}
};
__global__ void __launch_bounds__(256) mt_point_keys_kernel(int n, const int* __restrict__ wpts, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = ((unsigned long long)(unsigned)wpts[i] << 32) | (unsigned)i;
}
// the sorted keys are the good points in index order: the key at place r belongs to the list's entry in its low word
__global__ void __launch_bounds__(256) mt_point_ranks_kernel(int n, const unsigned long long* __restrict__ keys, int* __restrict__ wrank) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < n) wrank[(unsigned)keys[r]] = r;
}
__global__ void __launch_bounds__(256) mt_pair_keys_kernel(int n, const ptam_map_pair* __restrict__ q, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = mt_key(q[i].kf, q[i].point);
}
__global__ void __launch_bounds__(256) mt_key_pairs_kernel(int n, const unsigned long long* __restrict__ keys, ptam_map_pair* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ptam_map_pair q;
    q.kf = (int)(keys[i] >> 32);
    q.point = (int)(unsigned)keys[i];
    out[i] = q;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// ---- the cores: device pointers in, launches on the stream, no wait (maptables_internal.h) ---------------------------------------
int mt_queue_good_core(hipStream_t st, int n_new, const int32_t* new_queue, const uint8_t* bad, int* wpts, int* wentry, int* tiles, int* total) {
    HIP_TRY(hipMemsetAsync(total, 0, sizeof(int), st));
    mt_compact(st, MtGoodQueue{new_queue, bad, wpts, wentry}, n_new, tiles, total);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
int mt_queue_rank_core(hipStream_t st, int n_good, const int* wpts, int* wrank, unsigned long long* keys_a, unsigned long long* keys_b) {
    if (n_good == 0) return PTAM_OK;
    const dim3 grid((n_good + 255) / 256);
    hipLaunchKernelGGL(mt_point_keys_kernel, grid, dim3(256), 0, st, n_good, wpts, keys_a);
    const unsigned long long* sorted = mt_sort_keys(st, n_good, keys_a, keys_b);
    hipLaunchKernelGGL(mt_point_ranks_kernel, grid, dim3(256), 0, st, n_good, sorted, wrank);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
int mt_failure_sorted_core(hipStream_t st, int n_failure, const ptam_map_pair* failure, ptam_map_pair* out, unsigned long long* keys_a,
                           unsigned long long* keys_b) {
    if (n_failure == 0) return PTAM_OK;
    const dim3 grid((n_failure + 255) / 256);
    hipLaunchKernelGGL(mt_pair_keys_kernel, grid, dim3(256), 0, st, n_failure, failure, keys_a);
    const unsigned long long* sorted = mt_sort_keys(st, n_failure, keys_a, keys_b);
    hipLaunchKernelGGL(mt_key_pairs_kernel, grid, dim3(256), 0, st, n_failure, sorted, out);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}


// the flags, the three compactions, the merge
int mt_apply_outliers_core(hipStream_t st, const MtOutliersDev& d) {
    HIP_TRY(hipMemsetAsync(d.flag, 0, d.n_meas > 0 ? (size_t)d.n_meas : 1, st));
    HIP_TRY(hipMemsetAsync(d.tot, 0, 3 * sizeof(int), st));
    if (d.n_outliers > 0)
        hipLaunchKernelGGL(mt_outliers_kernel, dim3((d.n_outliers + 255) / 256), dim3(256), 0, st, d.n_outliers, d.outliers, d.flag, d.bad,
                           d.points, d.gate);
    mt_compact(st, MtUnflaggedRows{d.flag, d.meas, d.meas_out}, d.n_meas, d.tiles, d.tot + 0);
    mt_compact(st, MtNeverRows{d.flag, d.meas, d.new_never}, d.n_meas, d.tiles, d.tot + 1);
    mt_compact(st, MtFailureOutliers{d.outliers, d.failure_new}, d.n_outliers, d.tiles, d.tot + 2);
    if (d.n_never_out > 0)
        hipLaunchKernelGGL(mt_merge_kernel, dim3((unsigned)(((long long)d.n_never_out + 255) / 256)), dim3(256), 0, st, d.n_never, d.never,
                           (const int*)(d.tot + 1), (const ptam_map_pair*)d.new_never, d.never_out);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

// mark, scan the points, compact every table and queue through the remap, gather the columns
int mt_handle_bad_points_core(hipStream_t st, const MtBadDev& d) {
    HIP_TRY(hipMemsetAsync(d.tot, 0, MT_T_COUNT * sizeof(int), st));
    if (d.n_points > 0)
        hipLaunchKernelGGL(mt_mark_kernel, dim3((unsigned)(((long long)d.n_points + 255) / 256)), dim3(256), 0, st, d.n_points, d.bad,
                           d.outlier_count, d.inlier_count, d.removed, d.tot + MT_T_MARKED);
    const int32_t* ni = d.new_index;
    mt_compact(st, MtPoints{d.removed, d.new_index, d.kept}, d.n_points, d.tiles, d.tot + MT_T_KEPT);
    mt_compact(st, MtRemapRows<ptam_map_meas>{ni, d.meas, d.meas_out}, d.n_meas, d.tiles, d.tot + MT_T_MEAS);
    mt_compact(st, MtRemapRows<ptam_map_pair>{ni, d.never, d.never_out}, d.n_never, d.tiles, d.tot + MT_T_NEVER);
    mt_compact(st, MtRemapQueue{ni, d.new_queue, d.new_out}, d.n_new, d.tiles, d.tot + MT_T_NEW);
    mt_compact(st, MtRemapRows<ptam_map_pair>{ni, d.failure, d.failure_out}, d.n_failure, d.tiles, d.tot + MT_T_FAIL);
    for (int k = 0; k < d.n_columns && d.n_points > 0; k++) {
        const long long blocks = ((long long)d.n_points * d.col_dwords[k] + 255) / 256;
        hipLaunchKernelGGL(mt_gather_kernel, dim3((unsigned)std::min(blocks, 1ll << 20)), dim3(256), 0, st, (const int*)(d.tot + MT_T_KEPT),
                           (const int32_t*)d.kept, d.col_dwords[k], (const uint32_t*)d.col_in[k], (uint32_t*)d.col_out[k]);
    }
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

int mt_add_points_core(hipStream_t st, const MtAdd& p) {
    hipLaunchKernelGGL(mt_add_rows_kernel, dim3((unsigned)(((long long)p.n_meas + 2ll * p.n_made + 255) / 256)), dim3(256), 0, st, p);
    if (p.points || p.sources || p.points3 || p.bad || p.outlier_count || p.inlier_count || p.new_queue)
        hipLaunchKernelGGL(mt_add_points_kernel, dim3((p.n_made + 255) / 256), dim3(256), 0, st, p);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

// tot: {made, then the four per-status counts}
int mt_made_records_core(hipStream_t st, int n, const int32_t* status, const ptam_new_map_point* in, ptam_new_map_point* out, int* tiles, int* tot) {
    HIP_TRY(hipMemsetAsync(tot, 0, MT_MADE_WORDS * sizeof(int), st));
    if (n > 0) hipLaunchKernelGGL(mt_status_count_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, st, n, status, tot + 1);
    mt_compact(st, MtMadeRecords{status, in, out}, n, tiles, tot);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

extern "C" int ptam_map_apply_outliers(ptam_ctx* ctx, int n_kf, int n_points, int n_meas, const ptam_map_meas* meas, int n_never,
                                       const ptam_map_pair* never, int n_failure, const ptam_map_pair* failure, int n_outliers,
                                       const ptam_map_outlier* outliers, uint8_t* bad, ptam_map_outliers_result* res,
                                       ptam_map_meas* meas_out, ptam_map_pair* never_out, ptam_map_pair* failure_out) {
    // ---- refusals: nothing is written and nothing enqueued before all of them have passed
    ARG_TRY(ctx && res);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_failure >= 0 && n_outliers >= 0);
    ARG_TRY((long long)n_never + n_outliers < (1ll << 31) && (long long)n_failure + n_outliers < (1ll << 31));
    ARG_TRY((n_meas == 0 || (meas && meas_out)) && (n_never == 0 || never) && (n_failure == 0 || failure) && (n_outliers == 0 || outliers) &&
            (n_points == 0 || bad));
    ARG_TRY((n_never + n_outliers == 0 || never_out) && (n_failure + n_outliers == 0 || failure_out));
    ARG_TRY(mc_meas_valid(n_meas, meas, n_kf, n_points));
    ARG_TRY(mc_sorted_in_range(n_never, never, n_kf, n_points));
    ARG_TRY(mc_pairs_in_range(n_failure, failure, n_kf, n_points));
    ptam_map_outliers_result r;
    ARG_TRY(mc_outliers_tally(n_outliers, outliers, n_meas, meas, n_never, never, n_failure, &r) < 0);
    HIP_TRY(hipSetDevice(ctx->device));

    // ---- device memory
    const size_t Mz = (size_t)n_meas, Vz = (size_t)n_never, Oz = (size_t)n_outliers, Nz = (size_t)n_points;
    MtOutliersDev d = {};
    d.n_meas = n_meas;
    d.n_never = n_never;
    d.n_outliers = n_outliers;
    d.n_never_out = r.n_never_out;
    ptam_map_meas* d_meas;
    ptam_map_pair* d_never;
    ptam_map_outlier* d_outl;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver&) {
        d.meas = d_meas = c.room<ptam_map_meas>(Mz);
        d.never = d_never = c.room<ptam_map_pair>(Vz);
        d.outliers = d_outl = c.room<ptam_map_outlier>(Oz);
        d.bad = c.room<uint8_t>(Nz);
        d.flag = c.room<uint8_t>(Mz);
        d.tot = c.piece<int>(3);
        d.tiles = c.room<int>((size_t)mt_tiles(std::max(n_meas, n_outliers)));
        d.meas_out = c.room<ptam_map_meas>(Mz);
        d.new_never = c.room<ptam_map_pair>(Oz);
        d.never_out = c.room<ptam_map_pair>(Vz + Oz);
        d.failure_new = c.room<ptam_map_pair>(Oz);
    }));
    STAGE_TRY(s.up(d_meas, meas, Mz * sizeof(ptam_map_meas)));
    STAGE_TRY(s.up(d_never, never, Vz * sizeof(ptam_map_pair)));
    STAGE_TRY(s.up(d_outl, outliers, Oz * sizeof(ptam_map_outlier)));
    STAGE_TRY(s.up(d.bad, bad, Nz));
    STAGE_TRY(mt_apply_outliers_core(s.st, d));

    // ---- down: every size is known from the outlier list
    STAGE_TRY(s.down(meas_out, d.meas_out, (size_t)r.n_meas_out * sizeof(ptam_map_meas)));
    STAGE_TRY(s.down(never_out, d.never_out, (size_t)r.n_never_out * sizeof(ptam_map_pair)));
    STAGE_TRY(s.down(failure_out + n_failure, d.failure_new, (size_t)r.n_failure_added * sizeof(ptam_map_pair)));
    STAGE_TRY(s.down(bad, d.bad, Nz));
    HIP_TRY(ptam_stream_wait(s.st));
    if (n_failure > 0) std::memcpy(failure_out, failure, (size_t)n_failure * sizeof(ptam_map_pair));   // the old queue never left the host
    *res = r;
    return PTAM_OK;
}

extern "C" int ptam_map_handle_bad_points(ptam_ctx* ctx, int n_kf, int n_points, const uint8_t* bad, const int32_t* outlier_count,
                                          const int32_t* inlier_count, int n_meas, const ptam_map_meas* meas, int n_never,
                                          const ptam_map_pair* never, int n_new, const int32_t* new_queue, int n_failure,
                                          const ptam_map_pair* failure, int n_columns, const ptam_map_column* columns,
                                          ptam_map_bad_points_result* res, int32_t* new_index, int32_t* kept, ptam_map_meas* meas_out,
                                          ptam_map_pair* never_out, int32_t* new_queue_out, ptam_map_pair* failure_out) {
    // ---- refusals
    ARG_TRY(ctx && res);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_new >= 0 && n_failure >= 0);
    ARG_TRY(n_columns >= 0 && n_columns <= PTAM_MAP_MAX_COLUMNS && (n_columns == 0 || columns));
    ARG_TRY((outlier_count != nullptr) == (inlier_count != nullptr));
    ARG_TRY((n_points == 0 || (new_index && kept)) && (n_meas == 0 || (meas && meas_out)) && (n_never == 0 || (never && never_out)) &&
            (n_new == 0 || (new_queue && new_queue_out)) && (n_failure == 0 || (failure && failure_out)));
    for (int k = 0; k < n_columns; k++)
        ARG_TRY(columns[k].row_bytes > 0 && columns[k].row_bytes % 4 == 0 && (n_points == 0 || columns[k].data));
    ARG_TRY(mc_meas_valid(n_meas, meas, n_kf, n_points));
    ARG_TRY(mc_sorted_in_range(n_never, never, n_kf, n_points));
    ARG_TRY(mc_pairs_in_range(n_failure, failure, n_kf, n_points));
    ARG_TRY(mc_queue_unique(n_new, new_queue, n_points));
    HIP_TRY(hipSetDevice(ctx->device));

    // ---- device memory
    const size_t Nz = (size_t)n_points, Mz = (size_t)n_meas, Vz = (size_t)n_never, Qz = (size_t)n_new, Fz = (size_t)n_failure;
    const int longest = std::max(std::max(n_points, n_meas), std::max(std::max(n_never, n_new), n_failure));
    MtBadDev d = {};
    d.n_points = n_points;
    d.n_meas = n_meas;
    d.n_never = n_never;
    d.n_new = n_new;
    d.n_failure = n_failure;
    d.n_columns = n_columns;
    uint8_t* d_bad;
    int32_t *d_cnt_o, *d_cnt_i, *d_new;
    ptam_map_meas* d_meas;
    ptam_map_pair *d_never, *d_fail;
    int* h_counts;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_bad = c.room<uint8_t>(bad ? Nz : 0);
        d_cnt_o = c.room<int32_t>(outlier_count ? Nz : 0);
        d_cnt_i = c.room<int32_t>(outlier_count ? Nz : 0);
        d.meas = d_meas = c.room<ptam_map_meas>(Mz);
        d.never = d_never = c.room<ptam_map_pair>(Vz);
        d.new_queue = d_new = c.room<int32_t>(Qz);
        d.failure = d_fail = c.room<ptam_map_pair>(Fz);
        d.removed = c.room<uint8_t>(Nz);
        d.tot = c.piece<int>(MT_T_COUNT);
        d.tiles = c.room<int>((size_t)mt_tiles(longest));
        d.new_index = c.room<int32_t>(Nz);
        d.kept = c.room<int32_t>(Nz);
        d.meas_out = c.room<ptam_map_meas>(Mz);
        d.never_out = c.room<ptam_map_pair>(Vz);
        d.new_out = c.room<int32_t>(Qz);
        d.failure_out = c.room<ptam_map_pair>(Fz);
        for (int k = 0; k < n_columns; k++) {
            d.col_in[k] = c.room<char>(Nz * (size_t)columns[k].row_bytes);
            d.col_out[k] = c.room<char>(Nz * (size_t)columns[k].row_bytes);
            d.col_dwords[k] = columns[k].row_bytes / 4;
        }
        h_counts = pin.piece<int>(MT_T_COUNT);
    }));
    d.bad = bad ? d_bad : nullptr;
    d.outlier_count = outlier_count ? d_cnt_o : nullptr;
    d.inlier_count = outlier_count ? d_cnt_i : nullptr;
    if (bad) STAGE_TRY(s.up(d_bad, bad, Nz));
    if (outlier_count) {
        STAGE_TRY(s.up(d_cnt_o, outlier_count, Nz * 4));
        STAGE_TRY(s.up(d_cnt_i, inlier_count, Nz * 4));
    }
    STAGE_TRY(s.up(d_meas, meas, Mz * sizeof(ptam_map_meas)));
    STAGE_TRY(s.up(d_never, never, Vz * sizeof(ptam_map_pair)));
    STAGE_TRY(s.up(d_new, new_queue, Qz * 4));
    STAGE_TRY(s.up(d_fail, failure, Fz * sizeof(ptam_map_pair)));
    for (int k = 0; k < n_columns; k++) STAGE_TRY(s.up(const_cast<void*>(d.col_in[k]), columns[k].data, Nz * (size_t)columns[k].row_bytes));
    STAGE_TRY(mt_handle_bad_points_core(s.st, d));
    STAGE_TRY(s.down(h_counts, d.tot, MT_T_COUNT * sizeof(int)));
    HIP_TRY(ptam_stream_wait(s.st));   // the counts say how much of each table to fetch
    const ptam_map_bad_points_result r = mt_bad_result(h_counts, n_points, n_new);
    STAGE_TRY(s.down(new_index, d.new_index, Nz * 4));
    STAGE_TRY(s.down(kept, d.kept, (size_t)r.n_kept * 4));
    STAGE_TRY(s.down(meas_out, d.meas_out, (size_t)r.n_meas_out * sizeof(ptam_map_meas)));
    STAGE_TRY(s.down(never_out, d.never_out, (size_t)r.n_never_out * sizeof(ptam_map_pair)));
    STAGE_TRY(s.down(new_queue_out, d.new_out, (size_t)r.n_new_out * 4));
    STAGE_TRY(s.down(failure_out, d.failure_out, (size_t)r.n_failure_out * sizeof(ptam_map_pair)));
    for (int k = 0; k < n_columns; k++) STAGE_TRY(s.down(columns[k].data, d.col_out[k], (size_t)r.n_kept * (size_t)columns[k].row_bytes));
    HIP_TRY(ptam_stream_wait(s.st));
    *res = r;
    return PTAM_OK;
}

extern "C" int ptam_map_add_points(ptam_ctx* ctx, int n_kf, int n_points, int n_meas, const ptam_map_meas* meas, int src_kf, int target_kf,
                                   int target_source, int n_made, const ptam_new_map_point* made, ptam_map_meas* meas_out,
                                   ptam_map_refind_point* points_out, ptam_map_point_source* sources_out) {
    // ---- refusals
    ARG_TRY(ctx);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_made >= 0);
    ARG_TRY((long long)n_points + n_made < (1ll << 31) && (long long)n_meas + 2ll * n_made < (1ll << 31));
    ARG_TRY((n_meas == 0 || meas) && (n_made == 0 || made) && (n_meas + n_made == 0 || meas_out));
    ARG_TRY(src_kf >= 0 && src_kf < n_kf && target_kf >= 0 && target_kf < n_kf && src_kf != target_kf);
    ARG_TRY(target_source >= PTAM_MAP_SRC_TRACKER && target_source <= PTAM_MAP_SRC_EPIPOLAR);
    ARG_TRY(mc_meas_valid(n_meas, meas, n_kf, n_points));
    for (int i = 0; i < n_made; i++) ARG_TRY(made[i].level >= 0 && made[i].level < PTAM_LEVELS);
    if (n_made == 0) {   // nothing to insert: the table is a copy
        if (n_meas > 0) std::memcpy(meas_out, meas, (size_t)n_meas * sizeof(ptam_map_meas));
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    MtAdd p = mt_add_head(src_kf, target_kf, target_source, n_meas, n_made, n_points);
    const auto run_end = [&](int kf) {   // the new indices exceed all old ones: the end of the keyframe's run
        return (int)(std::upper_bound(meas, meas + n_meas, kf, [](int k, const ptam_map_meas& m) { return k < m.kf; }) - meas);
    };
    p.a = run_end(p.kf_lo);
    p.b = run_end(p.kf_hi);

    const size_t Mz = (size_t)n_meas, Az = (size_t)n_made;
    ptam_map_meas* d_meas;
    ptam_new_map_point* d_made;
    ptam_map_refind_point* d_pts;
    ptam_map_point_source* d_src;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver&) {
        p.meas = d_meas = c.room<ptam_map_meas>(Mz);
        p.made = d_made = c.piece<ptam_new_map_point>(Az);
        p.out = c.piece<ptam_map_meas>(Mz + 2 * Az);
        d_pts = c.room<ptam_map_refind_point>(points_out ? Az : 0);
        d_src = c.room<ptam_map_point_source>(sources_out ? Az : 0);
    }));
    p.points = points_out ? d_pts : nullptr;
    p.sources = sources_out ? d_src : nullptr;
    STAGE_TRY(s.up(d_meas, meas, Mz * sizeof(ptam_map_meas)));
    STAGE_TRY(s.up(d_made, made, Az * sizeof(ptam_new_map_point)));
    STAGE_TRY(mt_add_points_core(s.st, p));
    STAGE_TRY(s.down(meas_out, p.out, (Mz + 2 * Az) * sizeof(ptam_map_meas)));
    if (points_out) STAGE_TRY(s.down(points_out, d_pts, Az * sizeof(ptam_map_refind_point)));
    if (sources_out) STAGE_TRY(s.down(sources_out, d_src, Az * sizeof(ptam_map_point_source)));
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

void maptables_preload_kernels() {
    ptam_preload((const void*)mt_scan_kernel);
    ptam_preload((const void*)mt_count_kernel<MtUnflaggedRows>);
    ptam_preload((const void*)mt_scatter_kernel<MtUnflaggedRows>);
    ptam_preload((const void*)mt_count_kernel<MtNeverRows>);
    ptam_preload((const void*)mt_scatter_kernel<MtNeverRows>);
    ptam_preload((const void*)mt_count_kernel<MtFailureOutliers>);
    ptam_preload((const void*)mt_scatter_kernel<MtFailureOutliers>);
    ptam_preload((const void*)mt_count_kernel<MtPoints>);
    ptam_preload((const void*)mt_scatter_kernel<MtPoints>);
    ptam_preload((const void*)mt_count_kernel<MtRemapRows<ptam_map_meas>>);
    ptam_preload((const void*)mt_scatter_kernel<MtRemapRows<ptam_map_meas>>);
    ptam_preload((const void*)mt_count_kernel<MtRemapRows<ptam_map_pair>>);
    ptam_preload((const void*)mt_scatter_kernel<MtRemapRows<ptam_map_pair>>);
    ptam_preload((const void*)mt_count_kernel<MtRemapQueue>);
    ptam_preload((const void*)mt_scatter_kernel<MtRemapQueue>);
    ptam_preload((const void*)mt_count_kernel<MtMadeRecords>);
    ptam_preload((const void*)mt_scatter_kernel<MtMadeRecords>);
    ptam_preload((const void*)mt_count_kernel<MtGoodQueue>);
    ptam_preload((const void*)mt_scatter_kernel<MtGoodQueue>);
    ptam_preload((const void*)mt_sort_tile_kernel);
    ptam_preload((const void*)mt_sort_merge_kernel);
    ptam_preload((const void*)mt_point_keys_kernel);
    ptam_preload((const void*)mt_point_ranks_kernel);
    ptam_preload((const void*)mt_pair_keys_kernel);
    ptam_preload((const void*)mt_key_pairs_kernel);
    ptam_preload((const void*)mt_status_count_kernel);
    ptam_preload((const void*)mt_outliers_kernel);
    ptam_preload((const void*)mt_merge_kernel);
    ptam_preload((const void*)mt_mark_kernel);
    ptam_preload((const void*)mt_gather_kernel);
    ptam_preload((const void*)mt_add_rows_kernel);
    ptam_preload((const void*)mt_add_points_kernel);
}
