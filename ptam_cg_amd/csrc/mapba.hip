// mapba.hip — MapMaker::BundleAdjustRecent / BundleAdjustAll / BundleAdjust (src/MapMaker.cc:768-933) as ONE device call on flat
// map tables (ptam_map_bundle_adjust): the set choice, the bundle ids and the Add* marshalling on the device, the adjustment by the
// bundle's own Compute() (bundle.hip, inputs taken device to device: ba_dev_ingest), then the write-back through the id maps and
// the outlier routing.  M = table rows, K = keyframes, N = points.
//
//   mba_select_kernel   ONE WORKGROUP.  RECENT: camera centres of se3CfromW^-1 in uncontracted fp64, the 4 nearest other
//                       keyframes by (distance, index) in four block-wide arg-min passes (partial_sort, :711-730), the adjust set.
//                       ALL: adjust / fixed from bFixed
//   mba_mark_kernel     per row: the table checks (ranges, strictly ascending (kf, point)), rows per point (GoodMeasCount at the
//                       start), points measured by an adjust keyframe (:806-811)
//   mba_fixed_kernel    per row: a keyframe outside the adjust set that measures a chosen point joins the fixed set (:814-826);
//                       per 256-row block the number of rows the bundle takes
//   mba_ids_kernel      ONE WORKGROUP: exclusive scans -> camera ids (adjust ascending, then fixed ascending), point ids (ascending)
//                       with the points gathered (Bundle::AddPoint's NaN rule), block offsets of the rows
//   mba_compact_kernel  per row: ordered, stable compaction into the bundle's MeasStore chunks (cam, point, v2RootPos, 4^level)
//   -- one host wait: error flag, sizes, camera list (O(K)) --
//   Compute()
//   mba_scatter_*       accepted > 0: the bundle's points and poses back into the tables through the id maps
//   mba_order_kernel    the purged measurements per LM step in insertion order (GetOutlierMeasurements, src/Bundle.cc:540, :623)
//   mba_route_kernel    one lane per point with outliers walks them in list order: GoodMeasCount / SRC_ROOT rules (:916-932)
// mba_core is all of the above on tables in device memory.  ptam_map_bundle_adjust stages the caller's host arrays up into the
// call's scratch and the adjusted poses and points down; ptam_rmap_bundle_adjust (maprmap.hip) hands it a resident map's buffers:
// adjusted in place, mba_sync_world_kernel copies the points into the point rows' pv.world, the poses come down into the host mirror.
#include "common.h"
#include <climits>
#include <vector>

#include "bundle.h"
#include "maptables_internal.h"   // MbaTables, MbaWork, mba_core
#include "kf_dist_device.h"   // mba_centre, mba_linear_dist, mba_pair_less, mba_block_least

namespace {

enum { ROLE_NONE = 0, ROLE_ADJUST = 1, ROLE_FIXED = 2 };
#define MBA_BLOCK 256

struct MbaHdr {   // device counters, read back once after the selection
    int err;      // a row failed the table checks
    int err_row;  // the first such row
    int n_adjust, n_fixed, n_points, n_meas;
    int pad_[2];
};

struct MbaDev {
    int mode, K, N, M, nb;
    const double* pose;          // [K][12] the caller's se3CfromW
    const uint8_t* fixed;        // [K]
    double* pts;                 // [N][3] the caller's points (the write-back goes here first)
    const ptam_map_meas* meas;   // [M]
    int* role;                   // [K] ROLE_*
    int* cam_id;                 // [K] bundle camera id or -1
    int* cam_kf;                 // [K] bundle camera id -> keyframe
    int* pt_mark;                // [N] the point is in the bundle (RECENT)
    int* pt_rows;                // [N] table rows of the point
    int* pt_id;                  // [N] bundle point id or -1
    int* pt_of;                  // [N] bundle point id -> point
    double* pts_sel;             // [N][3] the bundle's points in bundle order
    int* blk;                    // [nb + 1] rows the bundle takes per block -> offsets
    int* sel_row;                // [M] bundle measurement -> table row
    char* ms;                    // the bundle's measurement chunks
    MbaHdr* hdr;
};

}   // namespace

__device__ __forceinline__ bool mba_row_ok(const MbaDev& a, const ptam_map_meas& m) {
    return (unsigned)m.kf < (unsigned)a.K && (unsigned)m.point < (unsigned)a.N && (unsigned)m.level < 4u && (unsigned)m.source < 5u;
}

// ---- set choice: BundleAdjustRecent's adjust set (:797-803) / BundleAdjustAll's roles (:770-776) ----------------------------------
__global__ void __launch_bounds__(1024) mba_select_kernel(MbaDev a) {
    const int tid = threadIdx.x;
    if (tid == 0) a.hdr->err_row = INT_MAX;
    if (a.mode == PTAM_MAP_BA_ALL) {
        for (int k = tid; k < a.K; k += 1024) a.role[k] = a.fixed[k] ? ROLE_FIXED : ROLE_ADJUST;
        return;
    }
    __shared__ double s_d[16];
    __shared__ int s_k[16];
    __shared__ int chosen[4];
    const int newest = a.K - 1;
    double c0[3];
    mba_centre(a.pose + (size_t)12 * newest, c0);
    const int n_pick = min(4, newest);
    for (int r = 0; r < n_pick; r++) {
        double bd = 0.0;
        int bk = -1;
        for (int k = tid; k < newest; k += 1024) {
            bool taken = false;
            for (int q = 0; q < r; q++) taken |= chosen[q] == k;
            if (taken) continue;
            const double d = mba_linear_dist(c0, a.pose + (size_t)12 * k);   // KeyFrameLinearDist(k1 = newest, k2 = k) (:700-701)
            if (bk < 0 || mba_pair_less(d, k, bd, bk)) bd = d, bk = k;
        }
        mba_block_least(bd, bk, s_d, s_k);
        if (tid == 0) chosen[r] = bk;
        __syncthreads();
    }
    if (tid == 0) {
        a.role[newest] = ROLE_ADJUST;   // with its own bFixed (:798-799, :853)
        for (int r = 0; r < n_pick; r++)
            if (chosen[r] >= 0 && !a.fixed[chosen[r]]) a.role[chosen[r]] = ROLE_ADJUST;
    }
}

// ---- table checks, rows per point, the adjust set's points (:806-811) -------------------------------------------------------------
__global__ void __launch_bounds__(MBA_BLOCK) mba_mark_kernel(MbaDev a) {
    const int i = blockIdx.x * MBA_BLOCK + threadIdx.x;
    if (i >= a.M) return;
    const ptam_map_meas m = a.meas[i];
    bool ok = mba_row_ok(a, m);
    if (ok && i > 0) {
        const int pk = a.meas[i - 1].kf, pp = a.meas[i - 1].point;
        ok = pk < m.kf || (pk == m.kf && pp < m.point);
    }
    if (!ok) {
        atomicOr(&a.hdr->err, 1);
        atomicMin(&a.hdr->err_row, i);
        return;
    }
    atomicAdd(&a.pt_rows[m.point], 1);
    if (a.mode == PTAM_MAP_BA_RECENT && a.role[m.kf] == ROLE_ADJUST) a.pt_mark[m.point] = 1;
}

__device__ __forceinline__ bool mba_take(const MbaDev& a, const ptam_map_meas& m) {
    return mba_row_ok(a, m) && (a.mode == PTAM_MAP_BA_ALL || a.pt_mark[m.point]);
}

// ---- the fixed set (:814-826), rows per block ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MBA_BLOCK) mba_fixed_kernel(MbaDev a) {
    const int i = blockIdx.x * MBA_BLOCK + threadIdx.x;
    bool take = false;
    if (i < a.M) {
        const ptam_map_meas m = a.meas[i];
        take = mba_take(a, m);
        if (take && a.role[m.kf] == ROLE_NONE) a.role[m.kf] = ROLE_FIXED;   // (only NONE -> FIXED happens here)
    }
    const int n = __syncthreads_count(take);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = n;
}

// exclusive scan of one value per thread over a 1024-thread workgroup
__device__ __forceinline__ int mba_block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
    for (int j = 0; j < 16; j++) {
        const int c = s_w[j];
        base += j < w ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// ---- bundle ids (:851-868) and the rows' block offsets: each thread owns a contiguous slice of every list -------------------------
__global__ void __launch_bounds__(1024) mba_ids_kernel(MbaDev a) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x;
    int tot_a = 0, tot_f = 0, tot_p = 0, tot_m = 0;
    {   // cameras: the adjust set ascending, then the fixed set ascending
        const int ch = (a.K + 1023) / 1024, k0 = min(a.K, tid * ch), k1 = min(a.K, k0 + ch);
        int na = 0, nf = 0;
        for (int k = k0; k < k1; k++) na += a.role[k] == ROLE_ADJUST, nf += a.role[k] == ROLE_FIXED;
        int ia = mba_block_scan(na, s_w, &tot_a);
        int jf = mba_block_scan(nf, s_w, &tot_f);
        for (int k = k0; k < k1; k++) {
            const int r = a.role[k];
            const int id = r == ROLE_ADJUST ? ia++ : r == ROLE_FIXED ? tot_a + jf++ : -1;
            a.cam_id[k] = id;
            if (id >= 0) a.cam_kf[id] = k;
        }
    }
    {   // points ascending (Bundle::AddPoint: a NaN position becomes zeros, src/Bundle.cc:70-74)
        const int ch = (a.N + 1023) / 1024, p0 = min(a.N, tid * ch), p1 = min(a.N, p0 + ch);
        int np = 0;
        for (int p = p0; p < p1; p++) np += a.mode == PTAM_MAP_BA_ALL || a.pt_mark[p];
        int ip = mba_block_scan(np, s_w, &tot_p);
        for (int p = p0; p < p1; p++) {
            if (a.mode == PTAM_MAP_BA_ALL || a.pt_mark[p]) {
                double v[3] = {a.pts[(size_t)3 * p], a.pts[(size_t)3 * p + 1], a.pts[(size_t)3 * p + 2]};
                if (isnan(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) v[0] = v[1] = v[2] = 0.0;
                for (int c = 0; c < 3; c++) a.pts_sel[(size_t)3 * ip + c] = v[c];
                a.pt_of[ip] = p;
                a.pt_id[p] = ip++;
            } else
                a.pt_id[p] = -1;
        }
    }
    {   // rows: block offsets
        const int ch = (a.nb + 1023) / 1024, b0 = min(a.nb, tid * ch), b1 = min(a.nb, b0 + ch);
        int nm = 0;
        for (int b = b0; b < b1; b++) nm += a.blk[b];
        int im = mba_block_scan(nm, s_w, &tot_m);
        for (int b = b0; b < b1; b++) {
            const int c = a.blk[b];
            a.blk[b] = im;
            im += c;
        }
    }
    if (tid == 0) {
        a.blk[a.nb] = tot_m;
        a.hdr->n_adjust = tot_a;
        a.hdr->n_fixed = tot_f;
        a.hdr->n_points = tot_p;
        a.hdr->n_meas = tot_m;
    }
}

// ---- the AddMeas calls of :871-882 in table order: ordered compaction into the MeasStore chunks -----------------------------------
__global__ void __launch_bounds__(MBA_BLOCK) mba_compact_kernel(MbaDev a) {
    __shared__ int s_w[MBA_BLOCK / 64];
    const int i = blockIdx.x * MBA_BLOCK + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    ptam_map_meas m;
    bool take = false;
    if (i < a.M) {
        m = a.meas[i];
        take = mba_take(a, m);
    }
    const unsigned long long bal = __ballot(take);
    if (lane == 0) s_w[w] = __popcll(bal);
    __syncthreads();
    if (!take) return;
    int j = a.blk[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int q = 0; q < w; q++) j += s_w[q];
    const int ls = 1 << m.level;   // Level::LevelScale (:880)
    const_cast<int&>(ms_cam(a.ms, (size_t)j)) = a.cam_id[m.kf];
    const_cast<int&>(ms_pt(a.ms, (size_t)j)) = a.pt_id[m.point];
    const_cast<double2&>(ms_found(a.ms, (size_t)j)) = make_double2(m.root_pos[0], m.root_pos[1]);
    const_cast<double&>(ms_sig(a.ms, (size_t)j)) = (double)(ls * ls);
    a.sel_row[j] = i;
}

// ---- write-back (:895-900): every bundle point (unobserved ones keep AddPoint's value), then the adjusted ones and the poses ------
__global__ void __launch_bounds__(256) mba_scatter_points_kernel(MbaDev a, int n_sel) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_sel) return;
    const int p = a.pt_of[q];
    for (int c = 0; c < 3; c++) a.pts[(size_t)3 * p + c] = a.pts_sel[(size_t)3 * q + c];
}
__global__ void __launch_bounds__(256) mba_scatter_live_kernel(MbaDev a, BaDevResult r, double* poses) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < r.P_live) {
        const int p = a.pt_of[r.pt_orig[q]];
        for (int c = 0; c < 3; c++) a.pts[(size_t)3 * p + c] = r.pt[(size_t)3 * q + c];
    }
    if (q < r.C) {
        const int k = a.cam_kf[q];
        for (int c = 0; c < 12; c++) poses[(size_t)12 * k + c] = r.pose[(size_t)12 * q + c];
    }
}

// ---- GetOutlierMeasurements: per LM step, the purged measurements in insertion order (indices are unique) -------------------------
__global__ void __launch_bounds__(256) mba_order_kernel(const int* __restrict__ raw, int n_out, const int* __restrict__ step_end,
                                                        int n_steps, int* __restrict__ ord) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    int b = 0, e = n_out;
    for (int s = 0; s < n_steps; s++) {
        if (i < step_end[s]) {
            e = min(step_end[s], n_out);
            break;
        }
        b = step_end[s];
    }
    const int v = raw[i];
    int rank = 0;
    for (int j = b; j < e; j++) rank += raw[j] < v;
    ord[b + rank] = v;
}
// each outlier: its table row and point; the first outlier of every point in list order
__global__ void __launch_bounds__(256) mba_route_prep_kernel(MbaDev a, const int* __restrict__ ord, int n_out, int n_sel,
                                                             int* __restrict__ o_row, int* __restrict__ o_pt, int* __restrict__ first) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_out) return;
    const int j = ord[k];
    const int row = (unsigned)j < (unsigned)n_sel ? a.sel_row[j] : 0;
    const int p = a.meas[row].point;
    o_row[k] = row;
    o_pt[k] = p;
    atomicMin(&first[p], k);
}
// :916-932 — one lane per point with outliers takes them in list order
__global__ void __launch_bounds__(256) mba_route_kernel(MbaDev a, int n_out, const int* __restrict__ o_row, const int* __restrict__ o_pt,
                                                        const int* __restrict__ first, ptam_map_outlier* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_out) return;
    const int p = o_pt[k];
    if (first[p] != k) return;
    int good = a.pt_rows[p];   // pMMData->GoodMeasCount() = sMeasurementKFs.size()
    for (int q = k; q < n_out; q++) {
        if (o_pt[q] != p) continue;
        const ptam_map_meas m = a.meas[o_row[q]];
        int action;
        if (good <= 2 || m.source == PTAM_MAP_SRC_ROOT)
            action = PTAM_MAP_OUT_POINT_BAD;
        else {
            action = (m.source == PTAM_MAP_SRC_TRACKER || m.source == PTAM_MAP_SRC_EPIPOLAR) ? PTAM_MAP_OUT_FAILURE_QUEUE : PTAM_MAP_OUT_NEVER_RETRY;
            good--;   // sMeasurementKFs.erase(pk)
        }
        ptam_map_outlier o;
        o.point = p;
        o.kf = m.kf;
        o.action = action;
        o.meas = o_row[q];
        out[q] = o;
    }
}

namespace {
struct BaGuard {   // the call's own bundle, destroyed on every return path
    ptam_ba* ba = nullptr;
    ~BaGuard() {
        if (ba) ptam_ba_destroy(ba);
    }
};
}   // namespace

// the resident map's second copy of the world positions (ptam_map_refind_point::pv) follows points3 after an accepted bundle
__global__ void __launch_bounds__(256) mba_sync_world_kernel(int n, const double* __restrict__ pts, ptam_map_refind_point* __restrict__ rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 3; c++) rows[i].pv.world[c] = pts[(size_t)3 * i + c];
}

// device scratch (the bundle keeps its own memory): [cleared: header | role | point marks | rows per point] then the rest
void mba_layout(Carver& c, Carver& pin, int K, int N, int M, MbaWork& w) {
    const size_t Kz = std::max(K, 1), Nz = std::max(N, 1), Mz = std::max(M, 1), nb = ((size_t)M + MBA_BLOCK - 1) / MBA_BLOCK;
    const size_t clear_from = c.off;
    w.cleared = (char*)c.piece<MbaHdr>(1);
    w.role = c.piece<int>(Kz);
    w.pt_mark = c.piece<int>(Nz);
    w.pt_rows = c.piece<int>(Nz);
    w.clear_bytes = c.off - clear_from;
    w.cam_id = c.piece<int>(Kz);
    w.cam_kf = c.piece<int>(Kz);
    w.pt_id = c.piece<int>(Nz);
    w.pt_of = c.piece<int>(Nz);
    w.pts_sel = c.piece<double>(Nz * 3);
    w.blk = c.piece<int>(nb + 1);
    w.sel_row = c.piece<int>(Mz);
    // outlier routing (outliers <= bundle measurements <= M)
    w.ord = c.piece<int>(Mz);
    w.orow = c.piece<int>(Mz);
    w.opt = c.piece<int>(Mz);
    w.first = c.piece<int>(Nz);
    w.out = c.piece<ptam_map_outlier>(Mz);
    w.h_sel = pin.piece<char>(sizeof(MbaHdr) + Kz * 4);
}

int mba_core(MapStage& s, const ptam_ba_opts* opts, int mode, const MbaTables& t, const MbaWork& w, const volatile unsigned char* abort_flag,
             ptam_map_ba_result* res, ptam_map_outlier* outliers, int32_t* cam_kf, int32_t* point_ids, int* n_routed) {
    ptam_ctx* ctx = s.ctx;
    const int K = t.K, N = t.N, M = t.M, nb = (M + MBA_BLOCK - 1) / MBA_BLOCK;
    BaGuard g;
    if (int rc = ptam_ba_create(ctx, opts, &g.ba)) return rc;
    char* d_ms = nullptr;
    if (int rc = ba_dev_meas_chunks(g.ba, (size_t)M, &d_ms)) return rc;
    MbaDev a;
    a.mode = mode, a.K = K, a.N = N, a.M = M, a.nb = nb;
    a.pose = t.d_poses;
    a.fixed = t.d_fixed;
    a.pts = t.d_points3;
    a.meas = t.d_meas;
    a.role = w.role;
    a.cam_id = w.cam_id;
    a.cam_kf = w.cam_kf;
    a.pt_mark = w.pt_mark;
    a.pt_rows = w.pt_rows;
    a.pt_id = w.pt_id;
    a.pt_of = w.pt_of;
    a.pts_sel = w.pts_sel;
    a.blk = w.blk;
    a.sel_row = w.sel_row;
    a.ms = d_ms;
    a.hdr = (MbaHdr*)w.cleared;
    // ---- the selection and its one wait: error flag, sizes, camera list
    hipStream_t st = s.st;
    HIP_TRY(hipMemsetAsync(w.cleared, 0, w.clear_bytes, st));
    hipLaunchKernelGGL(mba_select_kernel, dim3(1), dim3(1024), 0, st, a);
    if (M > 0) {
        hipLaunchKernelGGL(mba_mark_kernel, dim3(nb), dim3(MBA_BLOCK), 0, st, a);
        hipLaunchKernelGGL(mba_fixed_kernel, dim3(nb), dim3(MBA_BLOCK), 0, st, a);
    }
    hipLaunchKernelGGL(mba_ids_kernel, dim3(1), dim3(1024), 0, st, a);
    if (M > 0) hipLaunchKernelGGL(mba_compact_kernel, dim3(nb), dim3(MBA_BLOCK), 0, st, a);
    HIP_TRY(hipGetLastError());
    STAGE_TRY(s.down(w.h_sel, a.hdr, sizeof(MbaHdr)));
    STAGE_TRY(s.down(w.h_sel + sizeof(MbaHdr), a.cam_kf, (size_t)K * 4));
    HIP_TRY(ptam_stream_wait(st));
    const MbaHdr h = *(const MbaHdr*)w.h_sel;
    if (h.err) {
        ptam_set_error("map_bundle_adjust: table row %d is out of range or out of (kf, point) order", h.err_row);
        return PTAM_E_ARG;
    }
    const int C = h.n_adjust + h.n_fixed;
    if (C > K || h.n_points > N || h.n_meas > M) {
        ptam_set_error("map_bundle_adjust: inconsistent sizes (cameras %d / %d, points %d / %d, measurements %d / %d)", C, K, h.n_points, N,
                       h.n_meas, M);
        return PTAM_E_STATE;
    }
    // ---- the bundle's cameras: O(K) host work (:852-861), then ingest and Compute()
    std::vector<int> ckf((const int*)(w.h_sel + sizeof(MbaHdr)), (const int*)(w.h_sel + sizeof(MbaHdr)) + C);
    std::vector<double> cpose((size_t)12 * C);
    std::vector<uint8_t> cfix((size_t)C);
    for (int c = 0; c < C; c++) {
        const int k = ckf[(size_t)c];
        std::memcpy(&cpose[(size_t)12 * c], t.h_poses + (size_t)12 * k, 96);
        cfix[(size_t)c] = c < h.n_adjust ? (t.h_fixed[k] ? 1 : 0) : 1;
    }
    if (int rc = ba_dev_ingest(g.ba, C, cpose.data(), cfix.data(), h.n_points, a.pts_sel, h.n_meas)) return rc;
    int accepted = 0;
    if (int rc = ptam_ba_compute(g.ba, abort_flag, &accepted)) return rc;
    BaDevResult r;
    if (int rc = ba_dev_result(g.ba, &r)) return rc;
    // ---- the write-back through the id maps (:895-904)
    if (accepted > 0) {
        if (h.n_points > 0) hipLaunchKernelGGL(mba_scatter_points_kernel, dim3((h.n_points + 255) / 256), dim3(256), 0, st, a, h.n_points);
        const int nl = std::max(r.P_live, r.C);
        if (nl > 0) hipLaunchKernelGGL(mba_scatter_live_kernel, dim3((nl + 255) / 256), dim3(256), 0, st, a, r, t.d_poses);
        if (t.d_points && N > 0) hipLaunchKernelGGL(mba_sync_world_kernel, dim3((N + 255) / 256), dim3(256), 0, st, N, (const double*)a.pts, t.d_points);
        HIP_TRY(hipGetLastError());
    }
    // ---- the outlier routing (:916-932)
    const int n_out = std::min(r.n_out, h.n_meas);
    if ((outliers || n_routed) && n_out > 0) {
        void* hs = nullptr;   // the step ends, read by the ordering kernel through host-mapped memory; their number is known only now,
                              // and the selection's words in the pinned block have been read: a request of its own
        if (int rc = ctx_pinned(ctx, (size_t)std::max(r.n_steps, 1) * 4, &hs)) return rc;
        if (r.n_steps > 0) std::memcpy(hs, r.step_end, (size_t)r.n_steps * 4);
        HIP_TRY(hipMemsetAsync(w.first, 0x7f, (size_t)std::max(N, 1) * 4, st));
        const dim3 grid((n_out + 255) / 256);
        hipLaunchKernelGGL(mba_order_kernel, grid, dim3(256), 0, st, r.outliers, n_out, (const int*)ctx->d_pinned, r.n_steps, w.ord);
        hipLaunchKernelGGL(mba_route_prep_kernel, grid, dim3(256), 0, st, a, (const int*)w.ord, n_out, h.n_meas, w.orow, w.opt, w.first);
        hipLaunchKernelGGL(mba_route_kernel, grid, dim3(256), 0, st, a, n_out, (const int*)w.orow, (const int*)w.opt, (const int*)w.first, w.out);
        HIP_TRY(hipGetLastError());
        if (outliers) STAGE_TRY(s.down(outliers, w.out, (size_t)n_out * sizeof(ptam_map_outlier)));
    }
    if (n_routed) *n_routed = n_out;
    if (point_ids) STAGE_TRY(s.down(point_ids, a.pt_of, (size_t)h.n_points * 4));
    if (cam_kf && C > 0) std::memcpy(cam_kf, ckf.data(), (size_t)C * 4);
    res->ran = 1;
    res->accepted = accepted;
    res->converged = ptam_ba_converged(g.ba);
    res->n_adjust = h.n_adjust;
    res->n_fixed = h.n_fixed;
    res->n_points = h.n_points;
    res->n_meas = h.n_meas;
    res->n_outliers = r.n_out;
    return PTAM_OK;
}

extern "C" {

// the host-table form: check, stage up, core, stage down (the table rows themselves are checked by mba_mark_kernel)
int ptam_map_bundle_adjust(ptam_ctx* ctx, const ptam_ba_opts* opts, int mode, int n_kf, double* kf_poses12, const uint8_t* kf_fixed,
                           int n_points, double* points3, int n_meas, const ptam_map_meas* meas, const volatile unsigned char* abort_flag,
                           ptam_map_ba_result* res, ptam_map_outlier* outliers, int outlier_cap, int32_t* cam_kf, int32_t* point_ids) {
    ARG_TRY(ctx && res);
    ARG_TRY(mode == PTAM_MAP_BA_ALL || mode == PTAM_MAP_BA_RECENT);
    ARG_TRY(n_kf >= 0 && n_points >= 0 && n_meas >= 0);
    ARG_TRY(n_kf == 0 || (kf_poses12 && kf_fixed));
    ARG_TRY(n_points == 0 || points3);
    ARG_TRY(n_meas == 0 || meas);
    ARG_TRY(!outliers || outlier_cap >= n_meas);
    std::memset(res, 0, sizeof *res);
    if (mode == PTAM_MAP_BA_RECENT && n_kf < 8) return PTAM_OK;   // :790-793
    HIP_TRY(hipSetDevice(ctx->device));
    MbaTables t = {};
    t.K = n_kf;
    t.N = n_points;
    t.M = n_meas;
    t.h_poses = kf_poses12;
    t.h_fixed = kf_fixed;
    uint8_t* d_fixed;
    ptam_map_meas* d_meas;
    MbaWork w;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        mba_layout(c, pin, n_kf, n_points, n_meas, w);
        t.d_poses = c.piece<double>((size_t)std::max(n_kf, 1) * 12);
        t.d_fixed = d_fixed = c.piece<uint8_t>((size_t)std::max(n_kf, 1));
        t.d_points3 = c.piece<double>((size_t)std::max(n_points, 1) * 3);
        t.d_meas = d_meas = c.piece<ptam_map_meas>((size_t)std::max(n_meas, 1));
    }));
    STAGE_TRY(s.up(t.d_poses, kf_poses12, (size_t)n_kf * 96));
    STAGE_TRY(s.up(d_fixed, kf_fixed, (size_t)n_kf));
    STAGE_TRY(s.up(t.d_points3, points3, (size_t)n_points * 24));
    STAGE_TRY(s.up(d_meas, meas, (size_t)n_meas * sizeof(ptam_map_meas)));
    STAGE_TRY(mba_core(s, opts, mode, t, w, abort_flag, res, outliers, cam_kf, point_ids));
    if (res->accepted > 0) {
        STAGE_TRY(s.down(points3, t.d_points3, (size_t)n_points * 24));
        STAGE_TRY(s.down(kf_poses12, t.d_poses, (size_t)n_kf * 96));
    }
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

}   // extern "C"

void mapba_preload_kernels() {
    ptam_preload((const void*)mba_select_kernel);
    ptam_preload((const void*)mba_mark_kernel);
    ptam_preload((const void*)mba_fixed_kernel);
    ptam_preload((const void*)mba_ids_kernel);
    ptam_preload((const void*)mba_compact_kernel);
    ptam_preload((const void*)mba_scatter_points_kernel);
    ptam_preload((const void*)mba_scatter_live_kernel);
    ptam_preload((const void*)mba_order_kernel);
    ptam_preload((const void*)mba_route_prep_kernel);
    ptam_preload((const void*)mba_route_kernel);
    ptam_preload((const void*)mba_sync_world_kernel);
}
