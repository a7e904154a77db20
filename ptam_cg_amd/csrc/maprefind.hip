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
// mr_core uploads the work lists of a host plan (maprefind_plan.h) and calls mr_run, which is everything behind the lists;
// ptam_rmap_refind_queue (maprmap.hip) has kernels build the lists from the resident queue and calls mr_run itself.
#include <algorithm>

#include "maptables_internal.h"
#include "refind_internal.h"

enum { MR_FOUND = 0, MR_NEVER = 1, MR_SKIPPED = 2, MR_KEPT = 3, MR_COUNTS = 4 };
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

int mr_check_call(ptam_ctx* ctx, const ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_kf, const ptam_kf* const* kfs) {
    ARG_TRY(ctx && finder && finder->ctx->device == ctx->device);
    ARG_TRY(mode == PTAM_MAP_REFIND_KEYFRAME || mode == PTAM_MAP_REFIND_NEW_POINTS || mode == PTAM_MAP_REFIND_FAILURE_QUEUE);
    ARG_TRY(n_kf >= 0 && (n_kf == 0 || kfs));
    ARG_TRY(!opts || opts->max_pairs_per_pass >= 0);
    for (int k = 0; k < n_kf; k++) {
        ARG_TRY(kfs[k] && kfs[k]->device == ctx->device);
        ARG_TRY(kfs[k]->L.w[0] == ctx->params.width && kfs[k]->L.h[0] == ctx->params.height);
    }
    return PTAM_OK;
}

// what the layout and the passes need of a host plan
MrShape mr_shape(const MrPlan& plan) {
    MrShape sh;
    sh.mode = plan.mode;
    sh.kf0 = plan.kf0;
    sh.n_wp = (int)plan.wpts.size();
    sh.n_wq = (int)plan.wq.size();
    sh.pairs = plan.pairs;
    sh.per_pass = plan.per_pass;
    return sh;
}
void mr_layout(Carver& c, Carver& pin, int n_kf, const MrPlan& plan, bool merged, MrWork& w) { mr_layout_shape(c, pin, n_kf, mr_shape(plan), merged, w); }
// the call's lists (sized by the call), then the pass's work arrays (sized by the pass)
void mr_layout_shape(Carver& c, Carver& pin, int n_kf, const MrShape& plan, bool merged, MrWork& w) {
    const bool ordered = merged && plan.mode == PTAM_MAP_REFIND_NEW_POINTS;   // (visiting order is point-major there: mr_order_kernel)
    const size_t Pz = (size_t)plan.pairs, Wz = std::max((size_t)plan.n_wp, (size_t)plan.n_wq * 2);
    w.Ls = c.room<KfLevels>((size_t)n_kf);
    w.w0 = c.room<int>(Wz);
    w.w1 = c.room<int>(Wz);
    w.cnt = c.piece<int>(MR_COUNTS);
    w.found = c.room<ptam_map_meas>(Pz);
    w.subpix = c.room<int32_t>(Pz);
    w.nev = c.room<ptam_map_pair>(Pz);
    w.slot = c.room<int>(ordered ? Pz : 0);
    w.ord_f = c.room<int>(ordered ? Pz : 0);
    w.ord_n = c.room<int>(ordered ? Pz : 0);
    w.pairs = c.room<RpPair>((size_t)plan.per_pass);
    c.off = rp_carve(w.chain, c.base, c.off, plan.per_pass);
    w.h_cnt = pin.piece<int>(MR_COUNTS);
}

// the work lists of a host plan up, then mr_run; what the stop leaves of the queue is the plan's to say
int mr_core(MapStage& s, ptam_refinder* finder, const MrTables& t, const MrPlan& plan, const MrWork& w, const volatile unsigned char* stop_flag,
            ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix, ptam_map_pair* never_out) {
    STAGE_TRY(s.up(w.w0, plan.wpts.data(), plan.wpts.size() * 4));
    STAGE_TRY(s.up(w.w1, plan.wrank.data(), plan.wrank.size() * 4));
    STAGE_TRY(s.up(w.w0, plan.wq.data(), plan.wq.size() * sizeof(ptam_map_pair)));
    STAGE_TRY(mr_run(s, finder, t, mr_shape(plan), w, stop_flag, res, found_out, found_subpix, never_out));
    mr_plan_consumed(plan, res->n_pairs, res->stopped != 0, &res->points_consumed, &res->n_bad_points);
    return PTAM_OK;
}

int mr_run(MapStage& s, ptam_refinder* finder, const MrTables& t, const MrShape& plan, const MrWork& w, const volatile unsigned char* stop_flag,
           ptam_map_refind_result* res, ptam_map_meas* found_out, int32_t* found_subpix, ptam_map_pair* never_out) {
    const int P = plan.pairs, n_kf = t.n_kf;
    const bool merged = t.d_meas_merged || t.d_never_merged, ordered = merged && plan.mode == PTAM_MAP_REFIND_NEW_POINTS;
    hipStream_t st = s.st;
    // ---- up: the level records
    std::vector<KfLevels> hl((size_t)n_kf);
    for (int k = 0; k < n_kf; k++) hl[(size_t)k] = t.kfs[k]->L;
    STAGE_TRY(s.up(w.Ls, hl.data(), hl.size() * sizeof(KfLevels)));
    HIP_TRY(hipMemsetAsync(w.cnt, 0, MR_COUNTS * 4, st));
    if (ordered) HIP_TRY(hipMemsetAsync(w.slot, 0, (size_t)P * 4, st));   // (a stopped call leaves pairs unvisited)
    MrArgs a;
    a.mode = plan.mode;
    a.n_kf = n_kf;
    a.kf0 = plan.kf0;
    a.n_wp = plan.n_wp;
    a.wpts = w.w0;
    a.wrank = w.w1;
    a.wq = (const ptam_map_pair*)w.w0;
    a.poses = t.d_poses;
    a.Ls = w.Ls;
    a.pts = t.d_points;
    a.n_meas = t.n_meas;
    a.n_never = t.n_never;
    a.meas = t.d_meas;
    a.never = t.d_never;
    a.pairs = w.pairs;
    a.out = w.chain.out;
    a.kept = w.chain.kept;
    a.cnt = w.cnt;
    a.found = w.found;
    a.subpix = w.subpix;
    a.nev = w.nev;
    a.slot = ordered ? w.slot : nullptr;
    RpDev d = w.chain;
    d.pairs = a.pairs;
    d.Ls = a.Ls;
    d.st = finder->st;

    // ---- the passes: the stop flag is looked at before each one, nothing is waited for between them
    ptam_map_refind_result r = {};
    int visited = 0;
    while (visited < P) {
        if (stop_flag && *stop_flag) {
            r.stopped = 1;
            break;
        }
        a.first = visited;
        a.n = d.n = std::min(P - visited, plan.per_pass);
        hipLaunchKernelGGL(mr_pairs_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
        rp_launch_chain(st, s.ctx->cam, d);
        hipLaunchKernelGGL(mr_collect_kernel, dim3(1), dim3(1024), 0, st, a);
        visited += a.n;
    }
    r.n_pairs = visited;
    // ---- the merged tables: the rows' places in (kf, point) order where the visiting order is point-major, then the two merges
    const int *order_f = nullptr, *order_n = nullptr;
    if (ordered) {
        order_f = w.ord_f;
        order_n = w.ord_n;
        hipLaunchKernelGGL(mr_order_kernel, dim3(1), dim3(1024), 0, st, P, (const int*)a.slot, w.ord_f, w.ord_n);
    }
    if (t.d_meas_merged)
        hipLaunchKernelGGL(mr_merge_kernel<ptam_map_meas>, dim3((t.n_meas + visited + 255) / 256 + 1), dim3(256), 0, st, t.n_meas, a.meas,
                           (const int*)(a.cnt + MR_FOUND), (const ptam_map_meas*)a.found, order_f, t.d_meas_merged);
    if (t.d_never_merged)
        hipLaunchKernelGGL(mr_merge_kernel<ptam_map_pair>, dim3((t.n_never + visited + 255) / 256 + 1), dim3(256), 0, st, t.n_never, a.never,
                           (const int*)(a.cnt + MR_NEVER), (const ptam_map_pair*)a.nev, order_n, t.d_never_merged);
    HIP_TRY(hipGetLastError());
    STAGE_TRY(s.down(w.h_cnt, a.cnt, MR_COUNTS * 4));
    HIP_TRY(ptam_stream_wait(st));   // the counts say how much of the lists to fetch
    r.n_found = w.h_cnt[MR_FOUND];
    r.n_never = w.h_cnt[MR_NEVER];
    r.n_skipped = w.h_cnt[MR_SKIPPED];
    r.n_template_kept = w.h_cnt[MR_KEPT];
    if (found_out) {
        STAGE_TRY(s.down(found_out, a.found, (size_t)r.n_found * sizeof(ptam_map_meas)));
        STAGE_TRY(s.down(found_subpix, a.subpix, (size_t)r.n_found * 4));
        STAGE_TRY(s.down(never_out, a.nev, (size_t)r.n_never * sizeof(ptam_map_pair)));
    }
    *res = r;
    return PTAM_OK;
}

// the host-table form: check, stage up, core, stage down
extern "C" int ptam_map_refind(ptam_ctx* ctx, ptam_refinder* finder, const ptam_map_refind_opts* opts, int mode, int n_kf,
                               const ptam_kf* const* kfs, const double* kf_poses12, int n_points, const ptam_map_refind_point* points, int n_meas,
                               const ptam_map_meas* meas, int n_never, const ptam_map_pair* never, int n_work, const void* work,
                               const volatile unsigned char* stop_flag, ptam_map_refind_result* res, ptam_map_meas* found_out,
                               int32_t* found_subpix, ptam_map_pair* never_out, int out_cap, ptam_map_meas* meas_merged,
                               ptam_map_pair* never_merged) {
    // ---- refusals: nothing is written and nothing enqueued before all of them have passed
    ARG_TRY(res && n_points >= 0 && n_meas >= 0 && n_never >= 0 && n_work >= 0 && out_cap >= 0);
    if (int rc = mr_check_call(ctx, finder, opts, mode, n_kf, kfs)) return rc;
    ARG_TRY((n_work == 0 || work) && (n_kf == 0 || kf_poses12) && (n_points == 0 || points) && (n_meas == 0 || meas) && (n_never == 0 || never));
    ARG_TRY(mc_points_source_range(n_points, points, n_kf));
    ARG_TRY(mc_meas_valid(n_meas, meas, n_kf, n_points));
    ARG_TRY(mc_sorted_in_range(n_never, never, n_kf, n_points));
    MrPlan plan;
    ARG_TRY(mr_plan(mode, n_kf, n_points, n_work, work, [&](int, int p) { return points[p].bad != 0; }, opts ? opts->max_pairs_per_pass : 0, &plan));
    ARG_TRY(plan.bound + n_meas < (1ll << 31) && plan.bound + n_never < (1ll << 31));
    ARG_TRY(plan.bound <= (long long)out_cap);
    ARG_TRY(plan.bound == 0 || (found_out && found_subpix && never_out));
    if (plan.pairs == 0) {   // nothing to visit: the merged tables are copies
        if (meas_merged && n_meas > 0) std::memcpy(meas_merged, meas, (size_t)n_meas * sizeof(ptam_map_meas));
        if (never_merged && n_never > 0) std::memcpy(never_merged, never, (size_t)n_never * sizeof(ptam_map_pair));
        *res = mr_plan_nothing(plan, stop_flag && *stop_flag);
        return PTAM_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));

    // ---- the tables up, beside the core's work in the call's one block
    const size_t Pz = (size_t)plan.pairs, Mz = (size_t)n_meas, Vz = (size_t)n_never;
    double* d_poses;
    ptam_map_refind_point* d_points;
    ptam_map_meas* d_meas;
    ptam_map_pair* d_never;
    MrTables t = {};
    t.n_kf = n_kf;
    t.n_points = n_points;
    t.n_meas = n_meas;
    t.n_never = n_never;
    t.kfs = kfs;
    MrWork w;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        t.d_poses = d_poses = c.piece<double>((size_t)n_kf * 12);
        t.d_points = d_points = c.room<ptam_map_refind_point>((size_t)n_points);
        t.d_meas = d_meas = c.room<ptam_map_meas>(Mz);
        t.d_never = d_never = c.room<ptam_map_pair>(Vz);
        t.d_meas_merged = c.room<ptam_map_meas>(meas_merged ? Pz + Mz : 0);
        t.d_never_merged = c.room<ptam_map_pair>(never_merged ? Pz + Vz : 0);
        mr_layout(c, pin, n_kf, plan, meas_merged || never_merged, w);
    }));
    if (!meas_merged) t.d_meas_merged = nullptr;
    if (!never_merged) t.d_never_merged = nullptr;
    STAGE_TRY(s.up(d_poses, kf_poses12, (size_t)n_kf * 96));
    STAGE_TRY(s.up(d_points, points, (size_t)n_points * sizeof(ptam_map_refind_point)));
    STAGE_TRY(s.up(d_meas, meas, Mz * sizeof(ptam_map_meas)));
    STAGE_TRY(s.up(d_never, never, Vz * sizeof(ptam_map_pair)));
    ptam_map_refind_result r;
    STAGE_TRY(mr_core(s, finder, t, plan, w, stop_flag, &r, found_out, found_subpix, never_out));
    // ---- down: the merged tables, behind the lists
    if (meas_merged) STAGE_TRY(s.down(meas_merged, t.d_meas_merged, ((size_t)r.n_found + Mz) * sizeof(ptam_map_meas)));
    if (never_merged) STAGE_TRY(s.down(never_merged, t.d_never_merged, ((size_t)r.n_never + Vz) * sizeof(ptam_map_pair)));
    HIP_TRY(ptam_stream_wait(s.st));
    *res = r;
    return PTAM_OK;
}

void maprefind_preload_kernels() {
    ptam_preload((const void*)mr_pairs_kernel);
    ptam_preload((const void*)mr_collect_kernel);
    ptam_preload((const void*)mr_order_kernel);
    ptam_preload((const void*)mr_merge_kernel<ptam_map_meas>);
    ptam_preload((const void*)mr_merge_kernel<ptam_map_pair>);
}
