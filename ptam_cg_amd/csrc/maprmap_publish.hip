// maprmap_publish.hip — what the resident map (rmap_internal.h) gives to and takes from the tracker:
//   ptam_rmap_point_serials / resolve_serials   the serial column (one int64 per point, strictly increasing, given by rm_serials_kernel)
//                                   and a binary search in it (rm_resolve_kernel)
//   ptam_rmap_note_reports          the tracker's frame reports (framereport.hip) into the counts (rm_note_reports_kernel): records
//                                   resolved by serial where they lie
//   ptam_rmap_publish               the map as the tracker wants it into a ptam_map_snapshot's free slot (rm_publish_kernel): rows, patch
//                                   sources resolved through a per-keyframe level record, serials; the hand-over is snapshot_slots.h;
//                                   with a keyframe section in the snapshot also the pose table and the missing keyframe SBIs (sbi.hip)
#include <algorithm>

#include "rmap_internal.h"
#include "snapshot_internal.h"    // ptam_map_snapshot: ptam_rmap_publish fills its free slot
#include "sbi.h"                  // the snapshot's keyframe section: ptam_rmap_publish fills it too

namespace {

// the next serials of the handle, one thread per new point
__global__ void __launch_bounds__(256) rm_serials_kernel(int n, long long first, long long* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = first + i;
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

}   // namespace

void rm_give_serials(hipStream_t st, int n, long long first, long long* out) {
    if (n > 0) hipLaunchKernelGGL(rm_serials_kernel, dim3(MapStage::blocks(n)), dim3(256), 0, st, n, first, out);
}

extern "C" {

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
    RmReportRef* d_refs;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_refs = c.piece<RmReportRef>((size_t)n);
        hw = pin.piece<int>(RM_WORDS);
    }));
    STAGE_TRY(s.up(d_refs, refs.data(), (size_t)n * sizeof(RmReportRef)));
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_note_reports_kernel, dim3(s.blocks(most), (unsigned)n), dim3(256), 0, s.st, d_refs, m->n[RM_N_POINTS], rm_serials(m),
                       rm_outlier_count(m), rm_inlier_count(m), m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    res->n_records = (int32_t)all;
    res->n_gone = hw[RM_W_TOT];
    return PTAM_OK;
}

int ptam_rmap_point_serials(ptam_rmap* m, int first, int count, int64_t* out) {
    ARG_TRY(m && first >= 0 && count >= 0 && (long long)first + count <= m->n[RM_N_POINTS]);
    ARG_TRY(count == 0 || out);
    if (count == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    MapStage s = rm_stage(m);
    STAGE_TRY(s.down(out, rm_serials(m) + first, (size_t)count * sizeof(long long)));
    HIP_TRY(ptam_stream_wait(s.st));
    return PTAM_OK;
}

int ptam_rmap_resolve_serials(ptam_rmap* m, int n, const int64_t* serials, int32_t* index_out, int32_t* n_gone) {
    ARG_TRY(m && n >= 0 && (n == 0 || (serials && index_out)));
    if (n_gone) *n_gone = 0;
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(m->ctx->device));
    long long* d_keys;
    int32_t* d_index;
    int* hw;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_keys = c.piece<long long>((size_t)n);
        d_index = c.piece<int32_t>((size_t)n);
        hw = pin.piece<int>(RM_WORDS);
    }));
    STAGE_TRY(s.up(d_keys, serials, (size_t)n * sizeof(long long)));
    if (int rc = rm_words_reset(m)) return rc;
    hipLaunchKernelGGL(rm_resolve_kernel, dim3(s.blocks(n)), dim3(256), 0, s.st, n, d_keys, m->n[RM_N_POINTS], rm_serials(m), d_index,
                       m->d_words + RM_W_TOT);
    HIP_TRY(hipGetLastError());
    STAGE_TRY(s.down(index_out, d_index, (size_t)n * 4));
    if (int rc = rm_words_wait(s, m, hw)) return rc;
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
    RmKfRecord* d_recs;
    const uint8_t** d_l3;
    MapStage st = rm_stage(m);
    STAGE_TRY(st.carve([&](Carver& c, Carver&) {
        d_recs = c.piece<RmKfRecord>((size_t)K);
        d_l3 = c.piece<const uint8_t*>((size_t)K);
    }));
    const int s = snap->slots.begin_write();
    if (s < 0) {
        ptam_set_error("ptam_rmap_publish: a publish into this snapshot is under way");
        return PTAM_E_STATE;
    }
    // ---- the free slot is this call's until the commit
    ptam_map_publish_result r = {};
    int grew = 0;
    int rc = snap_slot_room(snap, s, (size_t)std::max(N, 1), &grew);
    if (!rc) rc = st.up(d_recs, recs.data(), (size_t)K * sizeof(RmKfRecord));
    const int kf_first = with_kfs ? sbi_snapshot_kf_first_missing(snap, s, m->map_id, m->kf_epoch, K) : K;
    std::vector<const uint8_t*> l3((size_t)(K - kf_first));   // (lives until the wait below)
    if (!rc && with_kfs) {
        for (int k = kf_first; k < K; k++) l3[(size_t)(k - kf_first)] = m->kfs[(size_t)k]->L.im[3];
        rc = st.up(d_l3, l3.data(), l3.size() * sizeof(l3[0]));
        if (!rc) rc = sbi_snapshot_kf_enqueue(m->ctx, snap, s, K, rm_poses(m), kf_first, d_l3);
    }
    if (!rc && N > 0) {
        SnapSlot& sl = snap->slot[s];
        hipLaunchKernelGGL(rm_publish_kernel, dim3(st.blocks(N)), dim3(256), 0, st.st, N, rm_points(m), rm_serials(m), d_recs, sl.pts, sl.src, sl.serials);
        if (hipGetLastError() != hipSuccess) rc = PTAM_E_HIP;
    }
    if (!rc && ptam_stream_wait(st.st) != hipSuccess) rc = PTAM_E_HIP;   // the call's one wait: the slot is whole
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

void maprmap_publish_preload_kernels() {
    ptam_preload((const void*)rm_serials_kernel);
    ptam_preload((const void*)rm_resolve_kernel);
    ptam_preload((const void*)rm_note_reports_kernel);
    ptam_preload((const void*)rm_publish_kernel);
}
