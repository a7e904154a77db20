// maprmap_keyframe.hip — a keyframe into the resident map (rmap_internal.h):
//   ptam_rmap_add_keyframe          the table side of AddKeyFrameFromTopOfQueue (src/MapMaker.cc:501-506)
//   ptam_rmap_closest_keyframes     ClosestKeyFrame / NClosestKeyFrames (:711-752): rm_closest_kernel on the resident pose table
//   ptam_rmap_insert_keyframe       AddKeyFrameFromTopOfQueue (:493-518) after MakeKeyFrame_Rest as one call: the keyframe's rows, its
//                                   re-find (ptam_rmap_refind), the closest keyframe, the busy list from the resident measurement table
//                                   (rm_busy_kernel), the epipolar chain of mapmaker.hip, and mt_add_points_core on the chain's output
//   ptam_rmap_insert_keyframe_report   the same with the rows taken from a tracker's frame report where it lies (rm_report_rows_kernel:
//                                   records resolved by serial)
//   rm_epipolar_points              steps (d)-(g) of an insertion — busy list, epipolar chain, its count, the new points' rows — for
//                                   ptam_rmap_init_from_stereo's AddSomeMapPoints as well (maprmap_init.hip)
// Each step of an insertion that ends in a wait of its own stages for itself; nothing of one step's scratch is read after its wait.
#include <algorithm>

#include "rmap_internal.h"
#include "kf_dist_device.h"       // mba_centre, mba_linear_dist, mba_pair_less, mba_block_least
#include "mapmaker_internal.h"    // EpiBusy, EpiRun, the epipolar chain

namespace {

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

// ---- host side -----------------------------------------------------------------------------------------------------------------
// :501-506, what both forms begin with: room for the pose, the flag and up to n_rows rows; the pose and the flag behind the keyframe
// tables' counts
int rm_add_keyframe_head(MapStage& s, ptam_rmap* m, const double pose12[12], const uint8_t* fx, long long n_rows) {
    const int K = m->n[RM_N_KF];
    if (int rc = rm_room(m, PTAM_RMAP_KF_POSES, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_KF_FIXED, (long long)K + 1)) return rc;
    if (int rc = rm_room(m, PTAM_RMAP_MEAS, (long long)m->n[RM_N_MEAS] + n_rows)) return rc;
    STAGE_TRY(s.up(rm_poses(m) + (size_t)12 * K, pose12, 96));
    return s.up(rm_fixed(m) + K, fx, 1);
}
// ... and the rows behind the measurement table's, from the host's list
int rm_add_keyframe_enqueue(ptam_rmap* m, const double pose12[12], const uint8_t* fx, int n_rows, const ptam_map_kf_row* rows) {
    MapStage s = rm_stage(m);
    if (int rc = rm_add_keyframe_head(s, m, pose12, fx, n_rows)) return rc;
    ptam_map_kf_row* d_rows;
    STAGE_TRY(s.carve([&](Carver& c, Carver&) { d_rows = c.piece<ptam_map_kf_row>((size_t)n_rows); }));
    if (n_rows > 0) {
        STAGE_TRY(s.up(d_rows, rows, (size_t)n_rows * sizeof(ptam_map_kf_row)));
        hipLaunchKernelGGL(rm_add_keyframe_kernel, dim3(s.blocks(n_rows)), dim3(256), 0, s.st, n_rows, d_rows, m->n[RM_N_KF], rm_meas(m) + m->n[RM_N_MEAS]);
        HIP_TRY(hipGetLastError());
    }
    return PTAM_OK;
}
// ... or from a frame report: room for every record, the live ones appended by the device; their count comes down in a wait
int rm_add_keyframe_enqueue_report(ptam_rmap* m, const double pose12[12], const uint8_t* fx, const ptam_frame_report* rep, int* n_rows) {
    const int R = rep->info.n_records;
    MapStage s = rm_stage(m);
    if (int rc = rm_add_keyframe_head(s, m, pose12, fx, R)) return rc;
    int* hw;
    STAGE_TRY(s.carve([&](Carver&, Carver& pin) { hw = pin.piece<int>(RM_WORDS); }));
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_report_rows_kernel, dim3(1), dim3(1024), 0, s.st, R, rep->rec, m->n[RM_N_POINTS], rm_serials(m), m->n[RM_N_KF],
                       rm_meas(m) + m->n[RM_N_MEAS], m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    if (int rc = rm_words_wait(s, m, hw)) return rc;
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
    char *b, *hp;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        b = c.piece<char>(bytes);
        hp = pin.piece<char>(bytes);
    }));
    hipLaunchKernelGGL(rm_closest_kernel, dim3(1), dim3(1024), 0, s.st, K, rm_poses(m), self, only, n_pick, (int*)b, (double*)(b + 8),
                       (int32_t*)(b + 8 + (size_t)8 * n_pick));
    HIP_TRY(hipGetLastError());
    STAGE_TRY(s.down(hp, b, bytes));
    HIP_TRY(ptam_stream_wait(s.st));
    *hdr = (const int*)hp;
    *dist = (const double*)(hp + 8);
    *idx = (const int32_t*)(hp + 8 + (size_t)8 * n_pick);
    return PTAM_OK;
}

}   // namespace

// Steps (d)-(g) of a keyframe's insertion, as AddSomeMapPoints runs them for kSrc = keyframe `src_kf` of the map (handle `src`, pose
// src_pose) against keyframe target_kf: rows [busy_first, busy_first + n_busy) of the resident measurement table are kSrc's run.
// run: sized by epi_sizes.  The made points become points [n_points, n_points + *n_made); levels: run.nl entries.
int rm_epipolar_points(ptam_rmap* m, int src_kf, const ptam_kf* src, const double src_pose[12], int target_kf, const ptam_epipolar_opts* epi,
                       EpiRun& run, int busy_first, int n_busy, int32_t* n_made, ptam_epipolar_level_stats* levels) {
    ptam_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    // ---- (d) the busy list
    ptam_kf* target = const_cast<ptam_kf*>(m->kfs[(size_t)target_kf]);   // (its implane tables are cached on the handle)
    if (int rc = epi_carve(ctx, target, epi, n_busy, run)) return rc;
    HIP_TRY(hipMemsetAsync(run.d_hdr, 0, EPI_HDR_BYTES, st));
    hipLaunchKernelGGL(rm_busy_kernel, dim3(std::max(MapStage::blocks(n_busy), 1u)), dim3(256), 0, st, n_busy, rm_meas(m) + busy_first, run.d_busy,
                       run.d_hdr);
    HIP_TRY(hipGetLastError());
    // ---- (e) the epipolar chain, (f) its count and stats
    if (int rc = epi_launch_chain(ctx, src, src_pose, target, m->h_poses.data() + (size_t)12 * target_kf, epi, run)) return rc;
    char* hp;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver&, Carver& pin) { hp = pin.piece<char>(EPI_HDR_BYTES); }));
    STAGE_TRY(s.down(hp, run.d_hdr, EPI_HDR_BYTES));
    HIP_TRY(ptam_stream_wait(st));
    const int made = ((const int*)hp)[1];
    if (made < 0 || made > run.sum) {
        ptam_set_error("ptam_rmap: %d epipolar points made, room for %d", made, run.sum);
        return PTAM_E_STATE;
    }
    std::memcpy(levels, hp + 16, sizeof(ptam_epipolar_level_stats) * (size_t)run.nl);
    *n_made = made;
    // ---- (g) the made points into the tables, straight from the chain's output
    if (made > 0)
        if (int rc = rm_add_points_device(m, src_kf, target_kf, PTAM_MAP_SRC_EPIPOLAR, made, run.d_out)) return rc;
    return PTAM_OK;
}

extern "C" {

int ptam_rmap_add_keyframe(ptam_rmap* m, const ptam_kf* kf, const double pose12[12], int fixed, int n_rows, const ptam_map_kf_row* rows) {
    ARG_TRY(m && pose12 && n_rows >= 0 && (n_rows == 0 || rows));
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS], M = m->n[RM_N_MEAS];
    ARG_TRY((long long)K + 1 < (1ll << 31) && (long long)M + n_rows < (1ll << 31));
    ARG_TRY(mc_kf_rows(N, n_rows, rows));   // the small list is checked where it is
    HIP_TRY(hipSetDevice(m->ctx->device));
    const uint8_t fx = fixed ? 1 : 0;
    if (int rc = rm_add_keyframe_enqueue(m, pose12, &fx, n_rows, rows)) return rc;
    HIP_TRY(ptam_stream_wait(m->ctx->stream));
    rm_add_keyframe_commit(m, kf, pose12, fx, n_rows);
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
        ARG_TRY(mc_kf_rows(N, n_rows, rows));
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
    // ---- (d)-(g): the busy list from the new keyframe's run (the tail of the table as (b) left it), the chain, the made points
    if (int rc = rm_epipolar_points(m, K, kf, pose12, r.target_kf, &opts->epipolar, run, M, m->n[RM_N_MEAS] - M, &r.n_made, r.levels)) return rc;
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

}   // extern "C"

void maprmap_keyframe_preload_kernels() {
    ptam_preload((const void*)rm_add_keyframe_kernel);
    ptam_preload((const void*)rm_closest_kernel);
    ptam_preload((const void*)rm_busy_kernel);
    ptam_preload((const void*)rm_report_rows_kernel);
}
