// maprefind.hip — MapMaker::ReFindInSingleKeyFrame / ReFindNewlyMade / ReFindFromFailureQueue (src/MapMaker.cc:1028-1081) as one
// call on the map tables (ptam_map_refind).  The tables go up once; per pass of at most max_pairs_per_pass pairs:
//   mr_pairs_kernel     one thread per pair: which (keyframe, point) it is, the set tests of :947-948 by binary search in the two
//                       sorted tables, and the pair record of refind.hip's chain (pose, point, template source, id, slot)
//   rp_* (refind.hip)   the finder chain, unchanged, with the finder's state carried from pass to pass
//   mr_collect_kernel   one workgroup: the found rows and the new never pairs appended to the call's lists in visiting order,
//                       the counts
// and after the last pass the merged tables: mr_order_kernel (NEW_POINTS only, where visiting order is point-major: the rows'
// places in (kf, point) order by one ordered compaction over the transposed pair grid) and mr_merge_kernel (two sorted lists
// into one, each row placed by a binary search in the other list).  Every order is fixed: the same input gives the same bits.
#include <algorithm>

#include "maptables_internal.h"
#include "refind_internal.h"

enum { MR_FOUND = 0, MR_NEVER = 1, MR_SKIPPED = 2, MR_KEPT = 3, MR_COUNTS = 4 };
enum { MR_DEFAULT_PASS = 4096 };
static_assert(sizeof(KfLevels) <= PTAM_RMAP_KF_RECORD_BYTES, "the per-keyframe record ptam_hip.h promises ptam_rmap_refind's callers");

struct MrArgs {
    int mode, n_kf;
    int kf0;                           // KEYFRAME: the keyframe
    int n_wp;                          // NEW_POINTS: points that make pairs
    const int* wpts;                   // NEW_POINTS: those points, in queue order
    const int* wrank;                  // NEW_POINTS: each one's place among them in index order
    const ptam_map_pair* wq;           // FAILURE_QUEUE: the sorted queue
    const double* poses;
    const KfLevels* Ls;                // one entry per keyframe of the table
    const ptam_map_refind_point* pts;
    int n_meas, n_never;
    const ptam_map_meas* meas;
    const ptam_map_pair* never;
    int first, n;                      // the pass: pairs [first, first + n) of the visiting order
    RpPair* pairs;
    const ptam_refind_result* out;
    const int* kept;
    int* cnt;                          // MR_COUNTS running counts
    ptam_map_meas* found;
    int32_t* subpix;
    ptam_map_pair* nev;
    int* slot;                         // NEW_POINTS with a merged table: [kf][rank of the point] -> +(found row + 1) / -(never row + 1) / 0
};

__device__ __forceinline__ unsigned long long mr_key(int kf, int point) {   // (indices are >= 0: one unsigned compare orders (kf, point))
    return ((unsigned long long)(unsigned)kf << 32) | (unsigned)point;
}
template <class Row>
__device__ __forceinline__ bool mr_contains(const Row* t, int n, unsigned long long key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (mr_key(t[mid].kf, t[mid].point) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && mr_key(t[lo].kf, t[lo].point) == key;
}
__device__ __forceinline__ void mr_pair_of(const MrArgs& a, int g, int& k, int& p, int& dup) {
    dup = 0;
    if (a.mode == PTAM_MAP_REFIND_KEYFRAME) {
        k = a.kf0;
        p = g;
    } else if (a.mode == PTAM_MAP_REFIND_NEW_POINTS) {
        k = g % a.n_kf;
        p = a.wpts[g / a.n_kf];
    } else {
        k = a.wq[g].kf;
        p = a.wq[g].point;
        dup = g > 0 && a.wq[g - 1].kf == k && a.wq[g - 1].point == p;
    }
}

__global__ void __launch_bounds__(256) mr_pairs_kernel(MrArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int k, p, dup;
    mr_pair_of(a, a.first + i, k, p, dup);
    const unsigned long long key = mr_key(k, p);
    const ptam_map_refind_point pt = a.pts[p];
    const KfLevels& S = a.Ls[pt.src_kf];
    RpPair r;
    r.pt = pt.pv;
    r.src.im = S.im[pt.src_level];
    r.src.w = S.w[pt.src_level];
    r.src.h = S.h[pt.src_level];
    r.src.cx = pt.center_x;
    r.src.cy = pt.center_y;
#pragma unroll
    for (int j = 0; j < 12; j++) r.pose[j] = a.poses[(size_t)12 * k + j];
    r.id = p;
    r.skip = dup || mr_contains(a.meas, a.n_meas, key) || mr_contains(a.never, a.n_never, key);   // :947-948
    r.kf = k;
    a.pairs[i] = r;
}

// exclusive offsets of two flags over the workgroup's 1024 threads, in thread order, and the totals
__device__ __forceinline__ void mr_scan2(int fa, int fb, int tid, int (*ws)[16], int& offa, int& offb, int& tota, int& totb) {
    const int lane = tid & 63, wid = tid >> 6;
    const int ia = wave_incl_scan_i32(fa), ib = wave_incl_scan_i32(fb);
    __syncthreads();   // (the previous round's sums have been read)
    if (lane == 63) {
        ws[0][wid] = ia;
        ws[1][wid] = ib;
    }
    __syncthreads();
    offa = ia - fa;
    offb = ib - fb;
    tota = totb = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wid) {
            offa += ws[0][w];
            offb += ws[1][w];
        }
        tota += ws[0][w];
        totb += ws[1][w];
    }
}

__global__ void __launch_bounds__(1024) mr_collect_kernel(MrArgs a) {
    __shared__ int ws[2][16];
    const int tid = threadIdx.x;
    int nf = a.cnt[MR_FOUND], nn = a.cnt[MR_NEVER], nsk = a.cnt[MR_SKIPPED], nkp = a.cnt[MR_KEPT];
    for (int b0 = 0; b0 < a.n; b0 += 1024) {
        const int i = b0 + tid;
        int f = 0, nv = 0, sk = 0, kp = 0;
        ptam_refind_result o;
        if (i < a.n) {
            o = a.out[i];
            f = o.found != 0;
            nv = !f && o.never_retry != 0;
            sk = !f && !nv;
            kp = a.kept[i] != 0;
        }
        int of, on, tf, tn;
        mr_scan2(f, nv, tid, ws, of, on, tf, tn);
        int s = 0;
        if (f) {
            ptam_map_meas m;
            m.kf = a.pairs[i].kf;
            m.point = (int)a.pairs[i].id;
            m.level = o.level;
            m.source = PTAM_MAP_SRC_REFIND;
            m.root_pos[0] = o.root_pos[0];
            m.root_pos[1] = o.root_pos[1];
            a.found[nf + of] = m;
            a.subpix[nf + of] = o.sub_pix;
            s = nf + of + 1;
        } else if (nv) {
            ptam_map_pair q;
            q.kf = a.pairs[i].kf;
            q.point = (int)a.pairs[i].id;
            a.nev[nn + on] = q;
            s = -(nn + on + 1);
        }
        if (a.slot && i < a.n) {
            const int g = a.first + i;
            a.slot[(size_t)(g % a.n_kf) * a.n_wp + a.wrank[g / a.n_kf]] = s;
        }
        nf += tf;
        nn += tn;
        int osk, okp, tsk, tkp;
        mr_scan2(sk, kp, tid, ws, osk, okp, tsk, tkp);
        nsk += tsk;
        nkp += tkp;
    }
    if (tid == 0) {
        a.cnt[MR_FOUND] = nf;
        a.cnt[MR_NEVER] = nn;
        a.cnt[MR_SKIPPED] = nsk;
        a.cnt[MR_KEPT] = nkp;
    }
}

// NEW_POINTS: slot[] is the pair grid in (kf, point) order; the rows met while walking it are the lists in sorted order
__global__ void __launch_bounds__(1024) mr_order_kernel(int total, const int* __restrict__ slot, int* __restrict__ order_f, int* __restrict__ order_n) {
    __shared__ int ws[2][16];
    const int tid = threadIdx.x;
    int nf = 0, nn = 0;
    for (int b0 = 0; b0 < total; b0 += 1024) {
        const int t = b0 + tid;
        const int s = t < total ? slot[t] : 0;
        int of, on, tf, tn;
        mr_scan2(s > 0, s < 0, tid, ws, of, on, tf, tn);
        if (s > 0) order_f[nf + of] = s - 1;
        if (s < 0) order_n[nn + on] = -s - 1;
        nf += tf;
        nn += tn;
    }
}

// out = A (sorted) merged with B taken in `order` (sorted that way; null: as it stands); no key is in both
template <class Row>
__global__ void __launch_bounds__(256) mr_merge_kernel(int nA, const Row* __restrict__ A, const int* __restrict__ nB_ptr, const Row* __restrict__ B,
                                                        const int* __restrict__ order, Row* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x, nB = *nB_ptr;
    if (t >= nA + nB) return;
    if (t < nA) {
        const Row r = A[t];
        const unsigned long long key = mr_key(r.kf, r.point);
        int lo = 0, hi = nB;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            const Row& b = B[order ? order[mid] : mid];
            if (mr_key(b.kf, b.point) < key) lo = mid + 1;
            else hi = mid;
        }
        out[t + lo] = r;
    } else {
        const int j = t - nA;
        const Row r = B[order ? order[j] : j];
        const unsigned long long key = mr_key(r.kf, r.point);
        int lo = 0, hi = nA;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (mr_key(A[mid].kf, A[mid].point) < key) lo = mid + 1;
            else hi = mid;
        }
        out[j + lo] = r;
    }
}

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
template <class Row>
static bool table_sorted_in_range(int n, const Row* t, int n_kf, int n_points) {
    for (int i = 0; i < n; i++) {
        if (t[i].kf < 0 || t[i].kf >= n_kf || t[i].point < 0 || t[i].point >= n_points) return false;
        if (i > 0 && !(t[i - 1].kf < t[i].kf || (t[i - 1].kf == t[i].kf && t[i - 1].point < t[i].point))) return false;
    }
    return true;
}

// ptam_map_refind on host tables or on a resident map's (maptables_internal.h)
int mr_run(ptam_ctx* ctx, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, const MrTables& t, int n_work, const void* work,
           const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix,
           ptam_map_pair* never_out, int out_cap, ptam_map_meas* meas_merged, ptam_map_pair* never_merged, int* merged_written,
           unsigned long long traffic[2]) {
    const int n_kf = t.n_kf, n_points = t.n_points, n_meas = t.n_meas, n_never = t.n_never;
    const ptam_kf* const* kfs = t.kfs;
    const double* kf_poses12 = t.h_poses;
    const ptam_map_refind_point* points = t.h_points;
    const ptam_map_meas* meas = t.h_meas;
    const ptam_map_pair* never = t.h_never;
    const bool resident = t.d_poses != nullptr;
    unsigned long long up = 0, down = 0;
    if (merged_written) *merged_written = 0;
    // ---- refusals: nothing is written and nothing enqueued before all of them have passed
    ARG_TRY(ctx && finder && finder->ctx->device == ctx->device && res);
    ARG_TRY(mode == PTAM_MAP_REFIND_KEYFRAME || mode == PTAM_MAP_REFIND_NEW_POINTS || mode == PTAM_MAP_REFIND_FAILURE_QUEUE);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_work >= 0 && out_cap >= 0);
    ARG_TRY((n_kf == 0 || kfs) && (n_work == 0 || work));
    ARG_TRY(resident || ((n_kf == 0 || kf_poses12) && (n_points == 0 || points) && (n_meas == 0 || meas) && (n_never == 0 || never)));
    ARG_TRY(!opts || opts->max_pairs_per_pass >= 0);
    for (int k = 0; k < n_kf; k++) {
        ARG_TRY(kfs[k] && kfs[k]->device == ctx->device);
        ARG_TRY(kfs[k]->L.w[0] == ctx->params.width && kfs[k]->L.h[0] == ctx->params.height);
    }
    if (!resident) {   // (a resident map's tables have been checked on the device when they went up, and every call keeps the rules)
        for (int p = 0; p < n_points; p++)
            ARG_TRY(points[p].src_kf >= 0 && points[p].src_kf < n_kf && points[p].src_level >= 0 && points[p].src_level < PTAM_LEVELS);
        ARG_TRY(table_sorted_in_range(n_meas, meas, n_kf, n_points));
        for (int i = 0; i < n_meas; i++)
            ARG_TRY(meas[i].level >= 0 && meas[i].level < PTAM_LEVELS && meas[i].source >= PTAM_MAP_SRC_TRACKER && meas[i].source <= PTAM_MAP_SRC_EPIPOLAR);
        ARG_TRY(table_sorted_in_range(n_never, never, n_kf, n_points));
    }
    std::vector<int> wpts, wrank, wentry;   // NEW_POINTS: the points that make pairs, their index-order places, their queue entries
    std::vector<ptam_map_pair> wq;          // FAILURE_QUEUE: sorted (:1074)
    int kf0 = 0;
    long long total = 0;                    // the call's pair count
    if (mode == PTAM_MAP_REFIND_KEYFRAME) {
        ARG_TRY(n_work <= 1);
        if (n_work == 1) {
            kf0 = *(const int32_t*)work;
            ARG_TRY(kf0 >= 0 && kf0 < n_kf);
            total = n_points;
        }
    } else if (mode == PTAM_MAP_REFIND_NEW_POINTS) {
        const int32_t* w = (const int32_t*)work;
        std::vector<uint8_t> seen((size_t)n_points, 0);
        for (int e = 0; e < n_work; e++) {
            ARG_TRY(w[e] >= 0 && w[e] < n_points && !seen[(size_t)w[e]]);
            seen[(size_t)w[e]] = 1;
            if (t.work_bad ? t.work_bad[e] != 0 : points[w[e]].bad != 0) continue;   // :1056-1059
            wpts.push_back(w[e]);
            wentry.push_back(e);
        }
        total = (long long)n_kf * n_work;   // (what the capacities are held against: bBad is the table's, not the count's, business)
    } else {
        const ptam_map_pair* w = (const ptam_map_pair*)work;
        for (int e = 0; e < n_work; e++) ARG_TRY(w[e].kf >= 0 && w[e].kf < n_kf && w[e].point >= 0 && w[e].point < n_points);
        total = n_work;
    }
    ARG_TRY(total + n_meas < (1ll << 31) && total + n_never < (1ll << 31));
    if (!resident || found_out || found_subpix || never_out) {
        ARG_TRY(total <= (long long)out_cap);
        ARG_TRY(total == 0 || (found_out && found_subpix && never_out));
    }
    if (mode == PTAM_MAP_REFIND_NEW_POINTS) {
        total = (long long)n_kf * (long long)wpts.size();
        std::vector<int> by_index(wpts.size());
        for (size_t i = 0; i < wpts.size(); i++) by_index[i] = (int)i;
        std::sort(by_index.begin(), by_index.end(), [&](int x, int y) { return wpts[(size_t)x] < wpts[(size_t)y]; });
        wrank.resize(wpts.size());
        for (size_t r = 0; r < by_index.size(); r++) wrank[(size_t)by_index[r]] = (int)r;
    } else if (mode == PTAM_MAP_REFIND_FAILURE_QUEUE) {
        const ptam_map_pair* w = (const ptam_map_pair*)work;
        wq.assign(w, w + n_work);
        std::sort(wq.begin(), wq.end(), [](const ptam_map_pair& x, const ptam_map_pair& y) { return x.kf < y.kf || (x.kf == y.kf && x.point < y.point); });
    }
    ptam_map_refind_result r = {};
    const int P = (int)total;
    if (P == 0) {   // nothing to visit: the merged tables are copies
        if (mode == PTAM_MAP_REFIND_NEW_POINTS && !(stop_flag && *stop_flag)) {
            r.points_consumed = n_work;
            r.n_bad_points = n_work - (int)wpts.size();
        } else if (mode == PTAM_MAP_REFIND_NEW_POINTS)
            r.stopped = n_work > 0;
        if (!resident && meas_merged && n_meas > 0) std::memcpy(meas_merged, meas, (size_t)n_meas * sizeof(ptam_map_meas));
        if (!resident && never_merged && n_never > 0) std::memcpy(never_merged, never, (size_t)n_never * sizeof(ptam_map_pair));
        *res = r;
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));

    // ---- device memory: the tables and the call's lists (sized by the call), the pass's work arrays (sized by the pass)
    int per_pass = opts && opts->max_pairs_per_pass > 0 ? opts->max_pairs_per_pass : MR_DEFAULT_PASS;
    if (mode == PTAM_MAP_REFIND_NEW_POINTS) per_pass = n_kf * (per_pass / n_kf > 0 ? per_pass / n_kf : 1);   // whole points, at least one
    if (per_pass > P) per_pass = P;
    ptam_map_meas* const d_mm_res = resident ? t.d_meas_merged : nullptr;
    ptam_map_pair* const d_nm_res = resident ? t.d_never_merged : nullptr;
    const bool want_mm = resident ? d_mm_res != nullptr : meas_merged != nullptr, want_nm = resident ? d_nm_res != nullptr : never_merged != nullptr;
    const bool merged = want_mm || want_nm, ordered = merged && mode == PTAM_MAP_REFIND_NEW_POINTS;
    const size_t Pz = (size_t)P, Kz = (size_t)n_kf, Wz = wpts.size() > wq.size() * 2 ? wpts.size() : wq.size() * 2;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += up256(bytes > 0 ? bytes : 1);
        return at;
    };
    const size_t o_pose = take(resident ? 0 : Kz * 96), o_ls = take(Kz * sizeof(KfLevels)),
                 o_pts = take(resident ? 0 : (size_t)n_points * sizeof(ptam_map_refind_point)),
                 o_meas = take(resident ? 0 : (size_t)n_meas * sizeof(ptam_map_meas)),
                 o_never = take(resident ? 0 : (size_t)n_never * sizeof(ptam_map_pair)),
                 o_w0 = take(Wz * 4), o_w1 = take(Wz * 4), o_cnt = take(MR_COUNTS * 4), o_found = take(Pz * sizeof(ptam_map_meas)),
                 o_sub = take(Pz * 4), o_nev = take(Pz * sizeof(ptam_map_pair)), o_slot = take(ordered ? Pz * 4 : 0),
                 o_ordf = take(ordered ? Pz * 4 : 0), o_ordn = take(ordered ? Pz * 4 : 0),
                 o_mm = take(want_mm && !resident ? (Pz + (size_t)n_meas) * sizeof(ptam_map_meas) : 0),
                 o_nm = take(want_nm && !resident ? (Pz + (size_t)n_never) * sizeof(ptam_map_pair) : 0), o_pairs = take((size_t)per_pass * sizeof(RpPair));
    RpDev d;
    void *sc, *hp;
    if (int rc = ctx_scratch(ctx, rp_carve(d, nullptr, off, per_pass), &sc)) return rc;
    if (int rc = ctx_pinned(ctx, 256, &hp)) return rc;
    char* b = (char*)sc;
    rp_carve(d, b, off, per_pass);
    hipStream_t st = ctx->stream;
    std::vector<KfLevels> hl(Kz);
    for (int k = 0; k < n_kf; k++) hl[(size_t)k] = kfs[k]->L;
    HIP_TRY(hipMemcpyAsync(b + o_ls, hl.data(), Kz * sizeof(KfLevels), hipMemcpyHostToDevice, st));
    up += Kz * sizeof(KfLevels) + wpts.size() * 8 + wq.size() * sizeof(ptam_map_pair);
    if (!resident) {
        HIP_TRY(hipMemcpyAsync(b + o_pose, kf_poses12, Kz * 96, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + o_pts, points, (size_t)n_points * sizeof(ptam_map_refind_point), hipMemcpyHostToDevice, st));
        if (n_meas > 0) HIP_TRY(hipMemcpyAsync(b + o_meas, meas, (size_t)n_meas * sizeof(ptam_map_meas), hipMemcpyHostToDevice, st));
        if (n_never > 0) HIP_TRY(hipMemcpyAsync(b + o_never, never, (size_t)n_never * sizeof(ptam_map_pair), hipMemcpyHostToDevice, st));
    }
    if (!wpts.empty()) {
        HIP_TRY(hipMemcpyAsync(b + o_w0, wpts.data(), wpts.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b + o_w1, wrank.data(), wrank.size() * 4, hipMemcpyHostToDevice, st));
    }
    if (!wq.empty()) HIP_TRY(hipMemcpyAsync(b + o_w0, wq.data(), wq.size() * sizeof(ptam_map_pair), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(b + o_cnt, 0, MR_COUNTS * 4, st));
    if (ordered) HIP_TRY(hipMemsetAsync(b + o_slot, 0, Pz * 4, st));   // (a stopped call leaves pairs unvisited)
    MrArgs a;
    a.mode = mode;
    a.n_kf = n_kf;
    a.kf0 = kf0;
    a.n_wp = (int)wpts.size();
    a.wpts = (const int*)(b + o_w0);
    a.wrank = (const int*)(b + o_w1);
    a.wq = (const ptam_map_pair*)(b + o_w0);
    a.poses = resident ? t.d_poses : (const double*)(b + o_pose);
    a.Ls = (const KfLevels*)(b + o_ls);
    a.pts = resident ? t.d_points : (const ptam_map_refind_point*)(b + o_pts);
    a.n_meas = n_meas;
    a.n_never = n_never;
    a.meas = resident ? t.d_meas : (const ptam_map_meas*)(b + o_meas);
    a.never = resident ? t.d_never : (const ptam_map_pair*)(b + o_never);
    a.pairs = (RpPair*)(b + o_pairs);
    a.out = d.out;
    a.kept = d.kept;
    a.cnt = (int*)(b + o_cnt);
    a.found = (ptam_map_meas*)(b + o_found);
    a.subpix = (int32_t*)(b + o_sub);
    a.nev = (ptam_map_pair*)(b + o_nev);
    a.slot = ordered ? (int*)(b + o_slot) : nullptr;
    d.pairs = a.pairs;
    d.Ls = a.Ls;
    d.st = finder->st;

    // ---- the passes: the stop flag is looked at before each one, nothing is waited for between them
    int visited = 0;
    while (visited < P) {
        if (stop_flag && *stop_flag) {
            r.stopped = 1;
            break;
        }
        a.first = visited;
        a.n = d.n = P - visited < per_pass ? P - visited : per_pass;
        hipLaunchKernelGGL(mr_pairs_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
        rp_launch_chain(st, ctx->cam, d);
        hipLaunchKernelGGL(mr_collect_kernel, dim3(1), dim3(1024), 0, st, a);
        visited += a.n;
    }
    r.n_pairs = visited;
    if (mode == PTAM_MAP_REFIND_NEW_POINTS) {   // queue entries behind the last visited point are popped while the flag is down (:1053-1059)
        const size_t wp = (size_t)(visited / n_kf);
        r.points_consumed = r.stopped ? (wp > 0 ? wentry[wp - 1] + 1 : 0) : n_work;
        r.n_bad_points = r.points_consumed - (int)wp;
    }
    const int* order_f = nullptr;
    const int* order_n = nullptr;
    if (ordered) {
        order_f = (const int*)(b + o_ordf);
        order_n = (const int*)(b + o_ordn);
        hipLaunchKernelGGL(mr_order_kernel, dim3(1), dim3(1024), 0, st, P, (const int*)a.slot, (int*)(b + o_ordf), (int*)(b + o_ordn));
    }
    if (want_mm)
        hipLaunchKernelGGL(mr_merge_kernel<ptam_map_meas>, dim3((n_meas + visited + 255) / 256 + 1), dim3(256), 0, st, n_meas, a.meas,
                           (const int*)(a.cnt + MR_FOUND), (const ptam_map_meas*)a.found, order_f, resident ? d_mm_res : (ptam_map_meas*)(b + o_mm));
    if (want_nm)
        hipLaunchKernelGGL(mr_merge_kernel<ptam_map_pair>, dim3((n_never + visited + 255) / 256 + 1), dim3(256), 0, st, n_never, a.never,
                           (const int*)(a.cnt + MR_NEVER), (const ptam_map_pair*)a.nev, order_n, resident ? d_nm_res : (ptam_map_pair*)(b + o_nm));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp, a.cnt, MR_COUNTS * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));   // the counts say how much of the lists to fetch
    const int* hc = (const int*)hp;
    r.n_found = hc[MR_FOUND];
    r.n_never = hc[MR_NEVER];
    r.n_skipped = hc[MR_SKIPPED];
    r.n_template_kept = hc[MR_KEPT];
    const size_t nf = (size_t)r.n_found, nn = (size_t)r.n_never;
    down += MR_COUNTS * 4;
    if (merged_written) *merged_written = 1;
    if (found_out) down += nf * (sizeof(ptam_map_meas) + 4) + nn * sizeof(ptam_map_pair);
    if (nf > 0 && found_out) {
        HIP_TRY(hipMemcpyAsync(found_out, a.found, nf * sizeof(ptam_map_meas), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(found_subpix, a.subpix, nf * 4, hipMemcpyDeviceToHost, st));
    }
    if (nn > 0 && never_out) HIP_TRY(hipMemcpyAsync(never_out, a.nev, nn * sizeof(ptam_map_pair), hipMemcpyDeviceToHost, st));
    if (!resident && meas_merged && nf + (size_t)n_meas > 0)
        HIP_TRY(hipMemcpyAsync(meas_merged, b + o_mm, (nf + (size_t)n_meas) * sizeof(ptam_map_meas), hipMemcpyDeviceToHost, st));
    if (!resident && never_merged && nn + (size_t)n_never > 0)
        HIP_TRY(hipMemcpyAsync(never_merged, b + o_nm, (nn + (size_t)n_never) * sizeof(ptam_map_pair), hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));   // (also keeps the staging vectors alive until their pageable copies have been staged)
    if (traffic) {
        traffic[0] = up;
        traffic[1] = down;
    }
    *res = r;
    return PTAM_OK;
}

extern "C" int ptam_map_refind(ptam_ctx* ctx, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_kf,
                               const ptam_kf* const* kfs, const double* kf_poses12, int n_points, const ptam_map_refind_point* points, int n_meas,
                               const ptam_map_meas* meas, int n_never, const ptam_map_pair* never, int n_work, const void* work,
                               const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out,
                               int32_t* found_subpix, ptam_map_pair* never_out, int out_cap, ptam_map_meas* meas_merged,
                               ptam_map_pair* never_merged) {
    MrTables t = {};
    t.n_kf = n_kf;
    t.n_points = n_points;
    t.n_meas = n_meas;
    t.n_never = n_never;
    t.kfs = kfs;
    t.h_poses = kf_poses12;
    t.h_points = points;
    t.h_meas = meas;
    t.h_never = never;
    return mr_run(ctx, finder, opts, mode, t, n_work, work, stop_flag, res, found_out, found_subpix, never_out, out_cap, meas_merged,
                  never_merged, nullptr, nullptr);
}

void maprefind_preload_kernels() {
    ptam_preload((const void*)mr_pairs_kernel);
    ptam_preload((const void*)mr_collect_kernel);
    ptam_preload((const void*)mr_order_kernel);
    ptam_preload((const void*)mr_merge_kernel<ptam_map_meas>);
    ptam_preload((const void*)mr_merge_kernel<ptam_map_pair>);
}
