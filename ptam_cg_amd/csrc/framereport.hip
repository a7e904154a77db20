// framereport.hip — ptam_frame_report (ptam_hip.h): the found entries of one tracked frame's iteration set as 32-byte records in
// device memory, sorted by point serial, filled on the tracker's side and consumed by the resident map (maprmap.hip) without a
// record crossing the host link.  What the reference does with pointers — CalcPoseUpdate's counts (src/Tracker.cc:989-997),
// mCurrentKF.mMeasurements (:667-676), AddKeyFrameFromTopOfQueue's stamps (src/MapMaker.cc:501-506).
//   fr_fill_kernel   ONE launch for a batch of frames, one 1024-thread workgroup per frame (blockIdx.y, as the batch chains' kernels):
//                      1. mark[p] = -1 over the frame's n points;
//                      2. one thread per slot: atomicMax(mark[list[s]], s) for found slots — the reference's sets are disjoint, so a
//                         point is named once; the max only defines what a repeat would do (the later slot wins, as
//                         mMeasurements[&p] = m would);
//                      3. an ordered compaction over the points in tiles of 1024 (the ballot / popcount offsets of maptables.hip's
//                         mt_tile_offset, the running count carried from tile to tile by the workgroup itself): point p with
//                         mark[p] >= 0 writes its record at the count of marked points in front of it.
//                    The serial column increases strictly with the point index, so index order is serial order: no sort.  No atomic
//                    decides where a record lands: the same frame gives the same bytes.  The workgroup's barriers order the three
//                    steps (a barrier makes the workgroup's global writes visible to itself); nothing is handed between workgroups.
//                    mt_compact's three launches would spread the tiles over the device; a tracker's map is a few tiles long and
//                    the call's cost is its launches, so the tiles run in sequence in one launch instead.
// Sizes at which the kernel changes path (tests/test_gpu_frame_report.py runs n - 1, n, n + 1 of each): 64 points (a second
// wave), 1024 (a second tile: the carried count), 2048.
#include <algorithm>

#include "framereport_internal.h"

namespace {

enum { FR_TILE = 1024 };
static_assert(sizeof(ptam_frame_record) == 32, "the record ptam_hip.h describes");

// slot s of a job: the point it names, or -1 where it is not found
__device__ __forceinline__ int fr_found_point(const FrJob& j, int s) {
    if (j.entries) return j.entries[s].found ? j.entries[s].point : -1;
    return j.slot_found[s] ? j.list[s] : -1;
}

__device__ __forceinline__ ptam_frame_record fr_record(const FrJob& j, int p, int s, int n_meas, int by_slot) {
    ptam_frame_record r;
    r.serial = j.serials[p];
    r.pad_[0] = r.pad_[1] = 0;
    if (j.entries) {
        const ptam_trackmap_meas e = j.entries[s];
        r.level = e.level;
        r.outlier = e.outlier != 0;
        r.did_subpix = e.did_subpix != 0;
        r.root_pos[0] = e.v2_found[0];
        r.root_pos[1] = e.v2_found[1];
        return r;
    }
    r.level = j.tres[s].bad ? -1 : j.q[s].level;   // (as ptam_tracker_read_iteration_set)
    r.did_subpix = j.slot_subpix[s] != 0;
    const double2 v = j.slot_v2[s];
    r.root_pos[0] = v.x;
    r.root_pos[1] = v.y;
    int out = 0;
    if (by_slot) out = j.outlier[s];
    else {   // the flags sit at the measurements; the gather compacts in slot order, so mslot ascends
        int lo = 0, hi = n_meas;
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (j.mslot[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n_meas && j.mslot[lo] == s) out = j.outlier[lo];
    }
    r.outlier = out != 0;
    return r;
}

// one workgroup fills job jobs[at]; heads + at * FR_HEAD_WORDS: the job's head words, written by thread 0 as the workgroup's last act
__device__ __forceinline__ void fr_fill_body(const FrJob* __restrict__ jobs, int* __restrict__ heads, unsigned at) {
    __shared__ int ws[2][FR_TILE / 64];
    const FrJob j = jobs[at];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = j.n_points;
    const int ns = j.entries ? j.n_entries : min(max(*j.n_slots, 0), j.cap);
    const int n_meas = j.entries ? 0 : min(max(*j.n_meas, 0), j.cap);
    const int by_slot = j.entries ? 0 : *j.outlier_by_slot;
    for (int p = tid; p < n; p += FR_TILE) j.mark[p] = -1;
    __syncthreads();
    for (int s = tid; s < ns; s += FR_TILE) {
        const int p = fr_found_point(j, s);
        if (p >= 0 && p < n) atomicMax(j.mark + p, s);
    }
    __syncthreads();
    int run = 0, n_out = 0;
    for (int base = 0; base < n; base += FR_TILE) {
        const int p = base + tid;
        const int s = p < n ? j.mark[p] : -1;
        const bool keep = s >= 0;
        ptam_frame_record r;
        if (keep) r = fr_record(j, p, s, n_meas, by_slot);
        const bool outl = keep && r.outlier;
        const unsigned long long m = __ballot(keep), mo = __ballot(outl);
        if (lane == 0) {
            ws[0][wid] = __popcll(m);
            ws[1][wid] = __popcll(mo);
        }
        __syncthreads();
        int off = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < FR_TILE / 64; w++) {
            const int c = ws[0][w];
            if (w < wid) off += c;
            total += c;
            n_out += ws[1][w];
        }
        const int at = run + off;
        if (keep && at < j.max_records) j.rec[at] = r;
        run += total;
        __syncthreads();   // (the wave counts are rewritten by the next tile)
    }
    if (tid == 0) {
        int* h = heads + (size_t)at * FR_HEAD_WORDS;
        h[FR_H_RECORDS] = run;
        h[FR_H_OUTLIERS] = n_out;
        h[FR_H_ENTRIES] = ns;
        h[FR_H_PAD] = 0;
    }
}

__global__ void __launch_bounds__(FR_TILE) fr_fill_kernel(const FrJob* __restrict__ jobs, int* __restrict__ heads) {
    fr_fill_body(jobs, heads, blockIdx.y);
}

// The fill at the end of a batch chain (ptam_track_frames_report_batch): the head words go to the frame's host-mapped block and the
// frame's sequence number behind them — what the host waits for.  A frame whose recovery failed (the gate, read as the TrackMap
// kernels read it) has tracked nothing: its head is zero and the tracker's control block, which still holds the frame before, is
// not looked at.  A frame whose fine pose loop asked for the long path (its sequence word says so) is not finished yet: nothing is
// filled or published, the host fills it behind the passes it enqueues.
__global__ void __launch_bounds__(FR_TILE) fr_fill_chain_kernel(const FrChainJob* __restrict__ jobs) {
    const FrChainJob& c = jobs[blockIdx.y];
    if (*(volatile const unsigned long long*)c.frame_word & FR_FRAME_LONG) return;
    if (c.gate && !*c.gate) {
        if (threadIdx.x < FR_HEAD_WORDS) c.head[threadIdx.x] = 0;
    } else {
        fr_fill_body(&c.job, c.head, 0);
    }
    __threadfence();   // (the records: whoever the host hands the report to may read them on another queue)
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        *(volatile unsigned long long*)c.head_seq = c.seq;
    }
}


}   // namespace

int fr_fill_core(hipStream_t st, int nb, const FrJob* d_jobs, int* d_heads) {
    hipLaunchKernelGGL(fr_fill_kernel, dim3(1, (unsigned)nb), dim3(FR_TILE), 0, st, d_jobs, d_heads);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

int fr_fill_chain_core(hipStream_t st, int nb, const FrChainJob* d_jobs) {
    hipLaunchKernelGGL(fr_fill_chain_kernel, dim3(1, (unsigned)nb), dim3(FR_TILE), 0, st, d_jobs);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

int fr_mark_room(ptam_frame_report* r, int n_points) {
    if ((size_t)n_points <= r->mark_cap) return PTAM_OK;
    const size_t cap = std::max((size_t)n_points, 2 * r->mark_cap);
    int* nm = nullptr;
    if (hipMalloc((void**)&nm, cap * sizeof(int)) != hipSuccess) {
        ptam_set_error("ptam_frame_report: no device memory for %zu marks", cap);
        return PTAM_E_HIP;
    }
    if (r->mark) {
        HIP_TRY(ptam_stream_wait(r->ctx->stream));
        HIP_TRY(hipFree(r->mark));
    }
    r->mark = nm;
    r->mark_cap = cap;
    return PTAM_OK;
}

extern "C" {

int ptam_frame_report_create(ptam_ctx* ctx, int max_records, ptam_frame_report** out) {
    ARG_TRY(ctx && out && max_records >= 1);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_frame_report* r = new ptam_frame_report();
    r->ctx = ctx;
    r->max_records = max_records;
    r->rec = nullptr;
    r->mark = nullptr;
    r->mark_cap = 0;
    r->info = ptam_frame_report_info_t{};
    if (hipMalloc((void**)&r->rec, (size_t)max_records * sizeof(ptam_frame_record)) != hipSuccess) {
        delete r;
        ptam_set_error("ptam_frame_report_create: no device memory for %d records", max_records);
        return PTAM_E_HIP;
    }
    *out = r;
    return PTAM_OK;
}

int ptam_frame_report_destroy(ptam_frame_report* r) {
    if (!r) return PTAM_OK;
    (void)hipSetDevice(r->ctx->device);
    (void)ptam_stream_wait(r->ctx->stream);
    if (r->rec) (void)hipFree(r->rec);
    if (r->mark) (void)hipFree(r->mark);
    delete r;
    return PTAM_OK;
}

int ptam_frame_report_info(const ptam_frame_report* r, ptam_frame_report_info_t* out) {
    ARG_TRY(r && out);
    *out = r->info;
    return PTAM_OK;
}

int ptam_frame_report_read(ptam_frame_report* r, int first, int count, ptam_frame_record* out) {
    ARG_TRY(r && first >= 0 && count >= 0 && (long long)first + count <= r->info.n_records);
    ARG_TRY(count == 0 || out);
    if (count == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(r->ctx->device));
    HIP_TRY(hipMemcpy(out, r->rec + first, (size_t)count * sizeof(ptam_frame_record), hipMemcpyDeviceToHost));
    return PTAM_OK;
}

int ptam_frame_report_from_host(ptam_frame_report* r, int64_t map_id, int n_points, const int64_t* point_serials, int n_entries,
                                const ptam_trackmap_meas* entries) {
    ARG_TRY(r && n_points >= 0 && n_entries >= 0 && (n_points == 0 || point_serials) && (n_entries == 0 || entries));
    ARG_TRY(map_id != 0);
    for (int i = 1; i < n_points; i++) ARG_TRY(point_serials[i - 1] < point_serials[i]);
    for (int s = 0; s < n_entries; s++)
        if (entries[s].found) ARG_TRY(entries[s].point >= 0 && entries[s].point < n_points && entries[s].level >= 0 && entries[s].level < PTAM_LEVELS);
    ptam_ctx* ctx = r->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = fr_mark_room(r, n_points)) return rc;
    long long* d_serials;
    ptam_trackmap_meas* d_entries;
    FrJob* d_job;
    int *d_head, *h;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_serials = c.piece<long long>((size_t)n_points);
        d_entries = c.piece<ptam_trackmap_meas>((size_t)n_entries);   // (non-null also for an empty set: the host's form)
        d_job = c.piece<FrJob>(1);
        d_head = c.piece<int>(FR_HEAD_WORDS);
        h = pin.piece<int>(FR_HEAD_WORDS);
    }));
    FrJob j = {};
    j.n_points = n_points;
    j.serials = d_serials;
    j.entries = d_entries;
    j.n_entries = n_entries;
    j.mark = r->mark;
    j.rec = r->rec;
    j.max_records = r->max_records;
    STAGE_TRY(s.up(d_serials, point_serials, (size_t)n_points * sizeof(long long)));
    STAGE_TRY(s.up(d_entries, entries, (size_t)n_entries * sizeof(ptam_trackmap_meas)));
    STAGE_TRY(s.up(d_job, &j, sizeof j));
    STAGE_TRY(fr_fill_core(s.st, 1, d_job, d_head));
    STAGE_TRY(s.down(h, d_head, FR_HEAD_WORDS * sizeof(int)));
    HIP_TRY(ptam_stream_wait(s.st));
    r->info = ptam_frame_report_info_t{};
    if (h[FR_H_RECORDS] > r->max_records) {
        ptam_set_error("bad argument: ptam_frame_report_from_host: %d found points, the report holds %d records", h[FR_H_RECORDS], r->max_records);
        return PTAM_E_ARG;
    }
    r->info.map_id = map_id;
    r->info.tag = 0;
    r->info.n_records = h[FR_H_RECORDS];
    r->info.n_entries = h[FR_H_ENTRIES];
    r->info.n_outliers = h[FR_H_OUTLIERS];
    return PTAM_OK;
}

}   // extern "C"

void framereport_preload_kernels() {
    ptam_preload((const void*)fr_fill_kernel);
    ptam_preload((const void*)fr_fill_chain_kernel);
}
