// trails.hip — the frames before a map exists, on gfx950: Tracker::TrailTracking_Start / TrailTracking_Advance
// (src/Tracker.cc:352-432) with MiniPatch::FindPatch / SSDAtPoint (src/ImageProcess.cc:57-80, 204-252), the match table of
// MapMaker::InitFromStereo (src/MapMaker.cc:272-279) and its point loop (:310-367).
//
// Start, once:
//   trails_start_kernel    lane = maximal corner of level 0: a candidate's rank in std::sort's order of pair<-score, ImageRef> is
//                          the number of candidates ordered before it (every key is distinct: positions are); the first
//                          min(max_initial, max_trails) ranks become trails and sample their 9x9 patch.
//   trails_keep_kernel     the frame's level-0 image, corners and row LUT copied into the object (mPreviousFrameKF).
// Advance, per frame — two launches, nothing crosses to the host between them:
//   trails_search_kernel   ONE WAVE PER TRAIL: the patch in LDS (9 rows of 3 words), lane = corner of rows y-10 .. y+10 from the row
//                          LUT, 64 at a time; a lane inside the box scores its corner (v_dot4: SSD = sum I^2 - 2 sum I T + sum T^2,
//                          integers); the wave minimum of (SSD << 6 | lane), earlier batches winning ties, is the first strictly
//                          smaller SSD in raster order.  Found: the backwards patch is read from the current frame into LDS and the
//                          same search runs in the kept previous frame (the married-matches check, :402-407).
//   trails_compact_kernel  workgroup 0: the survivors, in order, into the other trail buffer (ballot + per-wave counts, 1024 trails
//                          per pass), nGoodTrails and the live count; the other workgroups copy the current frame into the object
//                          (:430) — the searches of this frame have all ended, the launch is behind them on the queue.
// A trail's patch never moves: the trail record carries its slot in the patch table.
// Advance for nb cameras, each with its own object in its own context (ptam_trails_advance_batch) — ONE chain on the lead's queue:
//   MakeKeyFrame_Lite per camera, then
//   trails_search_batch_kernel   the search above with the camera as the grid's second dimension and a job table (TrailJob) in
//                                device memory; a row past its camera's live count returns.
//   trails_compact_batch_kernel  per camera the compaction and the kept frame as above; the counts also go to the object's
//                                host-mapped block, and the call's sequence number behind them is what the host waits for.
#include "common.h"

#include <algorithm>

#include "keyframe.h"
#include "track_internal.h"
#include "patch_device.h"
#include "mapmaker_device.h"
#include "homography.h"
#include "trails_internal.h"
#include "wait_mapped.h"

#define TRAIL_MAX_SSD 100000   // MiniPatch::FindPatch's default nMaxSSD (include/ImageProcess.h)
#define TRAIL_RANGE 10         // src/Tracker.cc:400
#define TRAIL_PATCH 9          // MiniPatch::mirPatchSize
#define TRAIL_PATCH_BYTES (TRAIL_PATCH * TRAIL_PATCH)
#define TRAIL_PATCH_WORDS 28   // 9 rows of 3 words (bytes 9 .. 11 of a row are zero), one spare
#define KEEP_BLOCKS 64

namespace {

struct PrevFrame {   // mPreviousFrameKF.aLevels[0]: im, vCorners, vCornerRowLUT
    uint8_t* im;
    ptam_int2* corners;
    int* rowlut;
    int* ncorners;
    int corner_cap;
};
enum { TRAIL_UNFOUND = 0, TRAIL_UNMARRIED = 1, TRAIL_KEPT = 2 };
enum { HDR_GOOD = 0, HDR_LIVE = 1, HDR_ARRIVED = 4 };   // (HDR_ARRIVED: workgroups of a batch's compaction that have ended; words 8.. are the kept frame's)

struct TrailDone {   // host-mapped, one per object: what a batch's compaction leaves for the host
    int good, live;
    unsigned long long seq;
};
struct TrailJob {    // one camera of ptam_trails_advance_batch: the arguments of the two per-camera kernels
    KfLevels C;
    PrevFrame P;
    int n, pad_;
    const ptam_trail* tin;
    const int* sin;
    const uint8_t* patches;
    int* status;
    ptam_int2* newpos;
    ptam_trail* tout;
    int* sout;
    int* hdr;
    TrailDone* done;
    unsigned long long seq;
};

}   // namespace

struct ptam_trails {
    ptam_ctx* ctx;
    int max_trails, w, h;
    int started, n_live, cur;   // cur: which of the two trail buffers holds the list
    void* base;
    PrevFrame prev;
    ptam_trail* trails[2];
    int* slot[2];
    uint8_t* patches;           // max_trails x 81 bytes, by slot
    int* status;
    ptam_int2* newpos;
    int* hdr;
    void* out;                  // read-back staging on the device: the match table / the patches in list order
    // ptam_trails_advance_batch
    TrailDone* done;            // host-mapped and coherent; done_dev: the same block as the device sees it
    TrailDone* done_dev;
    unsigned long long seq;     // the last batch call's sequence number
    void* batch_dev;            // the job table of the batches this object leads: grown on demand
    size_t batch_cap;
    int in_flight;              // a batch was enqueued for this object and has not been committed: it died on the way (see the batch)
};

__device__ __forceinline__ void keep_frame(const KfLevels& C, const PrevFrame& P, int w, int h, int part, int nparts) {
    const int tid = part * blockDim.x + threadIdx.x, nth = nparts * blockDim.x;
    const size_t n16 = ((((size_t)w * h) + 255) & ~(size_t)255) / 16;   // (a level's pixels are padded to 256 bytes on both sides)
    const uint4* __restrict__ s = (const uint4*)C.im[0];
    uint4* __restrict__ d = (uint4*)P.im;
    for (size_t i = tid; i < n16; i += nth) d[i] = s[i];
    const int nc = min(C.ncorners[0], P.corner_cap);
    for (int i = tid; i < nc; i += nth) P.corners[i] = C.corners[0][i];
    for (int i = tid; i < h; i += nth) P.rowlut[i] = C.rowlut[0][i];
    if (tid == 0) *P.ncorners = nc;
}

__global__ void __launch_bounds__(256) trails_keep_kernel(KfLevels C, PrevFrame P, int w, int h) { keep_frame(C, P, w, h, blockIdx.x, gridDim.x); }

// ---- TrailTracking_Start (src/Tracker.cc:352-370) ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) trails_start_kernel(KfLevels F, int w, int h, double thr, int ntake, ptam_trail* __restrict__ trails,
                                                           int* __restrict__ slot, uint8_t* __restrict__ patches, int* __restrict__ hdr) {
    const int n = F.nmax[0];
    const ptam_int2* __restrict__ mc = F.mcorners[0];
    const double* __restrict__ st = F.st[0];
    // Level::vCandidates (src/KeyFrame.cc:66-76): inside the 10-pixel border, Shi-Tomasi score above the threshold
    auto candidate = [&](ptam_int2 c, double s) { return c.x >= 10 && c.y >= 10 && c.x < w - 10 && c.y < h - 10 && s > thr; };
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const ptam_int2 c = mc[i];
        const double s = st[i];
        if (!candidate(c, s)) continue;
        int rank = 0;   // candidates before this one: higher score, then ImageRef::operator< (y, then x)
        for (int j = 0; j < n; j++) {
            const ptam_int2 cj = mc[j];
            const double sj = st[j];
            if (candidate(cj, sj) && (sj > s || (sj == s && (cj.y < c.y || (cj.y == c.y && cj.x < c.x))))) rank++;
        }
        atomicMax(&hdr[HDR_LIVE], min(rank + 1, ntake));
        if (rank >= ntake) continue;
        ptam_trail t;
        t.initial_x = t.current_x = c.x;
        t.initial_y = t.current_y = c.y;
        trails[rank] = t;
        slot[rank] = rank;
        uint8_t* p = patches + (size_t)rank * TRAIL_PATCH_BYTES;   // MiniPatch::SampleFromImage
        for (int r = 0; r < TRAIL_PATCH; r++)
            for (int k = 0; k < TRAIL_PATCH; k++) p[r * TRAIL_PATCH + k] = F.im[0][(size_t)(c.y - 4 + r) * w + (c.x - 4 + k)];
    }
}

// ---- MiniPatch::FindPatch (src/ImageProcess.cc:204-252) by one wave: pw = the patch (LDS), stt = its sum of squares ------------
__device__ __forceinline__ bool wave_find_minipatch(const uint8_t* __restrict__ im, int w, int h, const ptam_int2* __restrict__ corners,
                                                    const int* __restrict__ rowlut, int ncorners, const unsigned* pw, unsigned stt, int px,
                                                    int py, int lane, int& bx, int& by) {
    typedef unsigned u32_unaligned __attribute__((aligned(1)));
    const int left = px - TRAIL_RANGE, right = px + TRAIL_RANGE, top = py - TRAIL_RANGE, bottom = py + TRAIL_RANGE;
    const int i0 = rowlut[min(max(top, 0), h - 1)];
    const int i1 = bottom + 1 >= h ? ncorners : min(rowlut[max(bottom + 1, 0)], ncorners);
    int best = TRAIL_MAX_SSD + 1;
    bx = by = 0;
    for (int base = i0; base < i1; base += 64) {
        const int idx = base + lane;
        ptam_int2 c = {0, 0};
        bool pass = false;
        if (idx < i1) {
            c = corners[idx];
            pass = c.x >= left && c.x <= right && c.y >= top && c.y <= bottom;
        }
        unsigned ssd = TRAIL_MAX_SSD + 1;   // SSDAtPoint outside in_image_with_border(ir, 4)
        if (pass && c.x >= 4 && c.y >= 4 && c.x < w - 4 && c.y < h - 4) {
            const uint8_t* p = im + (size_t)(c.y - 4) * w + (c.x - 4);
            unsigned sii = 0, sit = 0;
#pragma unroll
            for (int r = 0; r < TRAIL_PATCH; r++) {
                const unsigned a = *(const u32_unaligned*)(p + (size_t)r * w), b = *(const u32_unaligned*)(p + (size_t)r * w + 4);
                const unsigned e = p[(size_t)r * w + 8];
                sii = __builtin_amdgcn_udot4(a, a, sii, false);
                sii = __builtin_amdgcn_udot4(b, b, sii, false);
                sii += e * e;
                sit = __builtin_amdgcn_udot4(a, pw[3 * r], sit, false);
                sit = __builtin_amdgcn_udot4(b, pw[3 * r + 1], sit, false);
                sit += e * pw[3 * r + 2];
            }
            ssd = sii + stt - 2u * sit;   // sum (I - T)^2 <= 81 * 255^2
        }
        const unsigned mk = wave_min_u32(pass ? ((ssd << 6) | (unsigned)lane) : 0xffffffffu);
        if (mk != 0xffffffffu && (int)(mk >> 6) < best) {   // (wave-uniform) nSSD < nBestSSD: the first one in raster order stays
            best = (int)(mk >> 6);
            bx = __builtin_amdgcn_readlane(c.x, (int)(mk & 63u));
            by = __builtin_amdgcn_readlane(c.y, (int)(mk & 63u));
        }
    }
    return best < TRAIL_MAX_SSD;
}

// the 9x9 patch at src (row pitch) into the wave's LDS words; returns its sum of squares
__device__ __forceinline__ unsigned wave_load_minipatch(const uint8_t* __restrict__ src, size_t pitch, unsigned* pw, int lane) {
    unsigned word = 0;
    if (lane < 27) {
        const int r = lane / 3, k = lane % 3;
        const uint8_t* p = src + (size_t)r * pitch + 4 * k;
        word = p[0];
        if (k < 2) word |= ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        pw[lane] = word;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (the words are read by every lane of the wave)
    __builtin_amdgcn_wave_barrier();
    return (unsigned)wave_sum_i32((int)__builtin_amdgcn_udot4(word, word, 0u, false));
}

// ---- TrailTracking_Advance (src/Tracker.cc:393-426), one wave per trail --------------------------------------------------------
__global__ void __launch_bounds__(256) trails_search_kernel(KfLevels C, PrevFrame P, int w, int h, int n, const ptam_trail* __restrict__ trails,
                                                            const int* __restrict__ slot, const uint8_t* __restrict__ patches,
                                                            int* __restrict__ status, ptam_int2* __restrict__ newpos) {
    __shared__ unsigned lds[4][2][TRAIL_PATCH_WORDS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wv;
    if (t >= n) return;
    const ptam_trail tr = trails[t];
    unsigned stt = wave_load_minipatch(patches + (size_t)slot[t] * TRAIL_PATCH_BYTES, TRAIL_PATCH, lds[wv][0], lane);
    int ex, ey, st = TRAIL_UNFOUND;
    const bool found = wave_find_minipatch(C.im[0], w, h, C.corners[0], C.rowlut[0], C.ncorners[0], lds[wv][0], stt, tr.current_x, tr.current_y,
                                           lane, ex, ey);
    if (found) {   // (a found corner passed SSDAtPoint's border: its 9x9 window is inside the image)
        st = TRAIL_UNMARRIED;
        stt = wave_load_minipatch(C.im[0] + (size_t)(ey - 4) * w + (ex - 4), (size_t)w, lds[wv][1], lane);   // BackwardsPatch.SampleFromImage
        int bx, by;
        const bool back = wave_find_minipatch(P.im, w, h, P.corners, P.rowlut, *P.ncorners, lds[wv][1], stt, ex, ey, lane, bx, by);
        const int dx = bx - tr.current_x, dy = by - tr.current_y;
        if (back && dx * dx + dy * dy <= 2) st = TRAIL_KEPT;   // (irBackWardsFound - irStart).mag_squared() > 2 -> erased
    }
    if (lane == 0) {
        status[t] = st;
        ptam_int2 e;
        e.x = found ? ex : tr.current_x;
        e.y = found ? ey : tr.current_y;
        newpos[t] = e;
    }
}

__global__ void __launch_bounds__(1024) trails_compact_kernel(KfLevels C, PrevFrame P, int w, int h, int n, const ptam_trail* __restrict__ tin,
                                                              const int* __restrict__ sin, const int* __restrict__ status,
                                                              const ptam_int2* __restrict__ newpos, ptam_trail* __restrict__ tout,
                                                              int* __restrict__ sout, int* __restrict__ hdr) {
    if (blockIdx.x > 0) {   // mPreviousFrameKF = mCurrentKF (:430)
        keep_frame(C, P, w, h, blockIdx.x - 1, gridDim.x - 1);
        return;
    }
    __shared__ int wk[16], wg[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int base = 0, good = 0;
    for (int start = 0; start < n; start += 1024) {
        const int i = start + tid;
        const int st = i < n ? status[i] : TRAIL_UNFOUND;
        const bool keep = st == TRAIL_KEPT;
        const unsigned long long mk = __ballot(keep), mg = __ballot(st != TRAIL_UNFOUND);
        if (lane == 0) {
            wk[wid] = __popcll(mk);
            wg[wid] = __popcll(mg);
        }
        __syncthreads();
        int pk = 0, tk = 0;
        for (int v = 0; v < 16; v++) {
            if (v < wid) pk += wk[v];
            tk += wk[v];
            good += wg[v];
        }
        if (keep) {
            ptam_trail t = tin[i];
            const ptam_int2 e = newpos[i];
            t.current_x = e.x;
            t.current_y = e.y;
            const int o = base + pk + __popcll(mk & lt);
            tout[o] = t;
            sout[o] = sin[i];
        }
        base += tk;
        __syncthreads();   // (wk / wg are rewritten by the next pass)
    }
    if (tid == 0) {
        hdr[HDR_GOOD] = good;
        hdr[HDR_LIVE] = base;
    }
}

// ---- the two launches for the cameras of a batch (ptam_trails_advance_batch): blockIdx.y = camera, its arguments in jobs[] ------
__global__ void __launch_bounds__(256) trails_search_batch_kernel(const TrailJob* __restrict__ jobs, int w, int h) {
    __shared__ unsigned lds[4][2][TRAIL_PATCH_WORDS];
    const TrailJob& j = jobs[blockIdx.y];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wv;
    if (t >= j.n) return;   // (the grid is shaped by the batch's longest list)
    const KfLevels& C = j.C;
    const PrevFrame& P = j.P;
    const ptam_trail tr = j.tin[t];
    unsigned stt = wave_load_minipatch(j.patches + (size_t)j.sin[t] * TRAIL_PATCH_BYTES, TRAIL_PATCH, lds[wv][0], lane);
    int ex, ey, st = TRAIL_UNFOUND;
    const bool found = wave_find_minipatch(C.im[0], w, h, C.corners[0], C.rowlut[0], C.ncorners[0], lds[wv][0], stt, tr.current_x, tr.current_y,
                                           lane, ex, ey);
    if (found) {
        st = TRAIL_UNMARRIED;
        stt = wave_load_minipatch(C.im[0] + (size_t)(ey - 4) * w + (ex - 4), (size_t)w, lds[wv][1], lane);
        int bx, by;
        const bool back = wave_find_minipatch(P.im, w, h, P.corners, P.rowlut, *P.ncorners, lds[wv][1], stt, ex, ey, lane, bx, by);
        const int dx = bx - tr.current_x, dy = by - tr.current_y;
        if (back && dx * dx + dy * dy <= 2) st = TRAIL_KEPT;
    }
    if (lane == 0) {
        j.status[t] = st;
        ptam_int2 e;
        e.x = found ? ex : tr.current_x;
        e.y = found ? ey : tr.current_y;
        j.newpos[t] = e;
    }
}

// Workgroup 0 of a camera compacts and leaves the counts in the device header and in the object's host-mapped block; the others keep
// the frame.  The sequence word goes out in fr_fill_chain_kernel's order — fence, barrier, system fence, the word — by the camera's
// LAST workgroup to end (a count in the header), so that a host which has seen the word may use the kept frame on another queue.
__global__ void __launch_bounds__(1024) trails_compact_batch_kernel(const TrailJob* __restrict__ jobs, int w, int h) {
    const TrailJob& j = jobs[blockIdx.y];
    const int tid = threadIdx.x;
    if (blockIdx.x > 0) {
        keep_frame(j.C, j.P, w, h, blockIdx.x - 1, gridDim.x - 1);
    } else {
        __shared__ int wk[16], wg[16];
        const int lane = tid & 63, wid = tid >> 6, n = j.n;
        const unsigned long long lt = (1ull << lane) - 1ull;
        int base = 0, good = 0;
        for (int start = 0; start < n; start += 1024) {
            const int i = start + tid;
            const int st = i < n ? j.status[i] : TRAIL_UNFOUND;
            const bool keep = st == TRAIL_KEPT;
            const unsigned long long mk = __ballot(keep), mg = __ballot(st != TRAIL_UNFOUND);
            if (lane == 0) {
                wk[wid] = __popcll(mk);
                wg[wid] = __popcll(mg);
            }
            __syncthreads();
            int pk = 0, tk = 0;
            for (int v = 0; v < 16; v++) {
                if (v < wid) pk += wk[v];
                tk += wk[v];
                good += wg[v];
            }
            if (keep) {
                ptam_trail t = j.tin[i];
                const ptam_int2 e = j.newpos[i];
                t.current_x = e.x;
                t.current_y = e.y;
                const int o = base + pk + __popcll(mk & lt);
                j.tout[o] = t;
                j.sout[o] = j.sin[i];
            }
            base += tk;
            __syncthreads();   // (wk / wg are rewritten by the next pass)
        }
        if (tid == 0) {
            j.hdr[HDR_GOOD] = good;
            j.hdr[HDR_LIVE] = base;
            j.done->good = good;
            j.done->live = base;
        }
    }
    __threadfence();   // (the list and the kept frame: the object's next call may read them on its own queue)
    __syncthreads();
    if (tid == 0) {
        __threadfence_system();
        if (atomicAdd(&j.hdr[HDR_ARRIVED], 1) == (int)gridDim.x - 1) {
            j.hdr[HDR_ARRIVED] = 0;   // (for the next batch; nobody else of this launch looks at it any more)
            __threadfence_system();
            *(volatile unsigned long long*)&j.done->seq = j.seq;
        }
    }
}

// ---- the match table of InitFromStereo (src/MapMaker.cc:272-279) --------------------------------------------------------------
// ATANCamera::UnProject (src/ATANCamera.cc:125-140) with what it leaves in the camera's cache: mvLastCam (x, y), mdLastR, mdLastFactor
__device__ __forceinline__ void cam_unproject_cached(const DevCam& c, double u, double v, double& x, double& y, double& r, double& f) {
#pragma clang fp contract(off)
    const double dx = (u - c.cx) * c.inv_fx, dy = (v - c.cy) * c.inv_fy;
    const double dr = sqrt(dx * dx + dy * dy);
    r = (c.w == 0.0) ? dr : tan(dr * c.w) * c.one_over_two_tan;   // invrtrans include/ATANCamera.h:152-157
    const double fac = dr > 0.01 ? r / dr : 1.0;
    f = 1.0 / fac;
    x = fac * dx;
    y = fac * dy;
}
__global__ void __launch_bounds__(256) trails_matches_kernel(DevCam cam, int n, const ptam_trail* __restrict__ trails,
                                                             ptam_homography_match* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ptam_trail t = trails[i];
    ptam_homography_match m;
    double r, f;
    cam_unproject_cached(cam, (double)t.initial_x, (double)t.initial_y, m.first[0], m.first[1], r, f);
    cam_unproject_cached(cam, (double)t.current_x, (double)t.current_y, m.second[0], m.second[1], r, f);
    cam_derivs(cam, m.second[0], m.second[1], r, f, m.jac);   // GetProjectionDerivs() on the cache of the SECOND UnProject
    out[i] = m;
}
__global__ void __launch_bounds__(256) trails_gather_patches_kernel(int n, const int* __restrict__ slot, const uint8_t* __restrict__ patches,
                                                                    uint8_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * TRAIL_PATCH_BYTES) return;
    out[i] = patches[(size_t)slot[i / TRAIL_PATCH_BYTES] * TRAIL_PATCH_BYTES + i % TRAIL_PATCH_BYTES];
}

// ---- the point loop of InitFromStereo (src/MapMaker.cc:310-367), one wave per match -----------------------------------------
namespace {
struct InitArgs {
    DevCam cam;
    double R[9], t[3];   // se3 (second from first)
    int its, n;
};
}   // namespace
__global__ void __launch_bounds__(256) init_points_kernel(InitArgs a, KfLevels F, KfLevels S, const ptam_trail* __restrict__ matches,
                                                          int* __restrict__ status, ptam_new_map_point* __restrict__ pts) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const ptam_trail m = matches[i];
    int code = PTAM_INIT_MADE;
    ptam_new_map_point P;
    const int fw = F.w[0], fh = F.h[0];
    // MakeTemplateCoarseNoWarp(first, 0, irCenter): in_image_with_border(irCenter, mnPatchSize / 2 + 1)
    if (!(m.initial_x >= 5 && m.initial_y >= 5 && m.initial_x < fw - 5 && m.initial_y < fh - 5)) code = PTAM_INIT_TEMPLATE_BAD;
    const double root_x = (double)m.initial_x, root_y = (double)m.initial_y;   // vec(irCenter)
    if (code == PTAM_INIT_MADE) {
        const int T = F.im[0][(size_t)(m.initial_y - 4 + (lane >> 3)) * fw + (m.initial_x - 4 + (lane & 7))];
        ptam_subpix_query sq;
        sq.level = 0;
        sq.max_its = a.its;
        sq.coarse_pos[0] = (double)m.current_x;   // SetSubPixPos(vec(vTrailMatches[i].second))
        sq.coarse_pos[1] = (double)m.current_y;
        ptam_subpix_result sr;
        wave_subpix(S, sq, T, lane, sr);
        if (!sr.converged) code = PTAM_INIT_SUBPIX_FAILED;
        P.target_pos[0] = sr.pos[0];
        P.target_pos[1] = sr.pos[1];
    }
    if (code == PTAM_INIT_MADE) {
        double uax, uay, ubx, uby;
        cam_unproject(a.cam, P.target_pos[0], P.target_pos[1], uax, uay);   // v2A = v2CamPlaneSecond
        cam_unproject(a.cam, root_x, root_y, ubx, uby);                     // v2B = v2CamPlaneFirst
        double A[16] = {-1.0, 0.0, ubx, 0.0, 0.0, -1.0, uby, 0.0};          // Triangulate(se3, v2A, v2B) (:171-189)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double p0 = j < 3 ? a.R[j] : a.t[0], p1 = j < 3 ? a.R[3 + j] : a.t[1], p2 = j < 3 ? a.R[6 + j] : a.t[2];
            A[8 + j] = nc_sub(nc_mul(uax, p2), p0);
            A[12 + j] = nc_sub(nc_mul(uay, p2), p1);
        }
        double v4[4];
        smallest_right_singular_vector(A, v4);
        if (v4[3] == 0.0) v4[3] = 0.00001;
        const double world[3] = {v4[0] / v4[3], v4[1] / v4[3], v4[2] / v4[3]};   // pkFirst->se3CfromW is the identity
        if (world[2] < 0.0) code = PTAM_INIT_BEHIND_CAMERA;
        double center[3], right[3], down[3];
        unit_ray(a.cam, root_x, root_y, center);
        unit_ray(a.cam, nc_add(root_x, 1.0), root_y, right);
        unit_ray(a.cam, root_x, nc_add(root_y, 1.0), down);
        // MapPoint::RefreshPixelVectors (src/Map.cc:40-65) in the first keyframe, whose pose is the identity: the plane point
        // in camera coordinates is the world position, the world frame the camera's; v3Normal_NC = (0, 0, -1)
        const double cam_h = fabs(world[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double cen = nc_mul(center[k], cam_h) / fabs(center[2]);
            P.point.pixel_right_w[k] = nc_sub(nc_mul(right[k], cam_h) / fabs(right[2]), cen);
            P.point.pixel_down_w[k] = nc_sub(nc_mul(down[k], cam_h) / fabs(down[2]), cen);
            P.point.world[k] = world[k];
            P.center_nc[k] = center[k];
            P.one_right_nc[k] = right[k];
            P.one_down_nc[k] = down[k];
        }
        P.src_root_pos[0] = root_x;
        P.src_root_pos[1] = root_y;
        P.level = 0;
        P.center_x = m.initial_x;
        P.center_y = m.initial_y;
        P.candidate = i;
        P.target_corner = -1;
        P.best_zmssd = 0;
    }
    if (lane == 0) {
        status[i] = code;
        if (code == PTAM_INIT_MADE) pts[i] = P;
    }
}

// ---- the same launches for ptam_rmap_init_from_stereo (trails_internal.h) ----------------------------------------------------------
void trails_view(const ptam_trails* t, TrailsView* out) {
    out->ctx = t->ctx;
    out->w = t->w;
    out->h = t->h;
    out->started = t->started;
    out->n_live = t->n_live;
    out->d_trails = t->trails[t->cur];
    out->d_out = (ptam_homography_match*)t->out;
}
int trails_matches_enqueue(ptam_ctx* ctx, int n, const ptam_trail* d_trails, ptam_homography_match* d_out) {
    hipLaunchKernelGGL(trails_matches_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->cam, n, d_trails, d_out);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
int init_points_enqueue(ptam_ctx* ctx, const ptam_kf* first, const ptam_kf* second, const double se3_second_from_first[12], int subpix_max_its,
                        int n, const ptam_trail* d_matches, int* d_status, ptam_new_map_point* d_pts) {
    InitArgs a;
    a.cam = ctx->cam;
    for (int i = 0; i < 9; i++) a.R[i] = se3_second_from_first[i];
    for (int i = 0; i < 3; i++) a.t[i] = se3_second_from_first[9 + i];
    a.its = subpix_max_its;
    a.n = n;
    hipLaunchKernelGGL(init_points_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, a, first->L, second->L, d_matches, d_status, d_pts);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

extern "C" {

int ptam_trails_create(ptam_ctx* ctx, int max_trails, ptam_trails** out) {
    ARG_TRY(ctx && out && max_trails >= 1);
    HIP_TRY(hipSetDevice(ctx->device));
    const int w = ctx->params.width, h = ctx->params.height;
    ARG_TRY(w >= 8 && h >= 8);
    ptam_trails* t = new ptam_trails();
    std::memset(t, 0, sizeof *t);
    t->ctx = ctx;
    t->max_trails = max_trails;
    t->w = w;
    t->h = h;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t px = up((size_t)w * h), n = (size_t)max_trails;
    const size_t b_im = px + 256, b_corn = px * sizeof(ptam_int2), b_lut = up((size_t)h * 4), b_hdr = 256, b_tr = up(n * sizeof(ptam_trail)),
                 b_slot = up(n * 4), b_patch = up(n * TRAIL_PATCH_BYTES) + 256, b_pos = up(n * sizeof(ptam_int2)),
                 b_out = up(n * (sizeof(ptam_homography_match) > (size_t)TRAIL_PATCH_BYTES ? sizeof(ptam_homography_match) : (size_t)TRAIL_PATCH_BYTES));
    const size_t total = b_im + b_corn + b_lut + b_hdr + 2 * b_tr + 3 * b_slot + b_patch + b_pos + b_out;
    hipError_t e = hipMalloc(&t->base, total);
    if (e != hipSuccess) {
        ptam_set_error("hipMalloc(%zu) failed: %s", total, hipGetErrorString(e));
        delete t;
        return PTAM_E_HIP;
    }
    char* p = (char*)t->base;
    t->prev.im = (uint8_t*)p;
    t->prev.corners = (ptam_int2*)(p += b_im);
    t->prev.corner_cap = (int)px;
    t->prev.rowlut = (int*)(p += b_corn);
    t->hdr = (int*)(p += b_lut);
    t->prev.ncorners = t->hdr + 8;
    t->trails[0] = (ptam_trail*)(p += b_hdr);
    t->trails[1] = (ptam_trail*)(p += b_tr);
    t->slot[0] = (int*)(p += b_tr);
    t->slot[1] = (int*)(p += b_slot);
    t->status = (int*)(p += b_slot);
    t->patches = (uint8_t*)(p += b_slot);
    t->newpos = (ptam_int2*)(p += b_patch);
    t->out = (void*)(p += b_pos);
    void *hp, *hs;   // the staging and the scratch every later call needs, so that none of them allocates
    size_t homog_scratch, homog_pinned;   // (ptam_trails_homography on max_trails matches with the reference's 300 trials)
    homog_sizes(max_trails, 300, &homog_scratch, &homog_pinned);
    int rc = ctx_pinned(ctx, std::max(256 + b_out + n * sizeof(ptam_trail), homog_pinned), &hp);
    if (!rc) rc = ctx_scratch(ctx, homog_scratch, &hs);
    // the block a batch's compaction reports into, and the header's arrival count at zero
    void *hd = nullptr, *dd = nullptr;
    if (!rc && (hipHostMalloc(&hd, sizeof(TrailDone), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                hipHostGetDevicePointer(&dd, hd, 0) != hipSuccess || hipMemsetAsync(t->hdr, 0, b_hdr, ctx->stream) != hipSuccess ||
                ptam_stream_wait(ctx->stream) != hipSuccess)) {   // (on the object's own queue, and done before anyone uses the object)
        ptam_set_error("ptam_trails_create: no host-mapped block: %s", hipGetErrorString(hipGetLastError()));
        rc = PTAM_E_HIP;
    }
    if (rc) {
        if (hd) hipHostFree(hd);
        hipFree(t->base);
        delete t;
        return rc;
    }
    std::memset(hd, 0, sizeof(TrailDone));
    t->done = (TrailDone*)hd;
    t->done_dev = (TrailDone*)dd;
    *out = t;
    return PTAM_OK;
}

int ptam_trails_destroy(ptam_trails* t) {
    if (!t) return PTAM_OK;
    hipSetDevice(t->ctx->device);
    hipDeviceSynchronize();
    hipFree(t->base);
    if (t->batch_dev) hipFree(t->batch_dev);
    hipHostFree(t->done);
    delete t;
    return PTAM_OK;
}

static int trails_check_kf(const ptam_trails* t, const ptam_kf* kf) {
    ARG_TRY(kf->device == t->ctx->device);
    ARG_TRY(kf->L.w[0] == t->w && kf->L.h[0] == t->h);
    return PTAM_OK;
}
static int trails_need_start(const ptam_trails* t, const char* what) {
    if (t->started) return PTAM_OK;
    ptam_set_error("%s: no ptam_trails_start yet", what);
    return PTAM_E_STATE;
}

int ptam_trails_start(ptam_trails* t, const ptam_kf* first, double min_shi_tomasi, int max_initial, int* n_trails) {
    ARG_TRY(t && first && n_trails);
    int rc = trails_check_kf(t, first);
    if (rc) return rc;
    if (!first->rest_made) {
        ptam_set_error("trails_start: the keyframe has no MakeKeyFrame_Rest since its MakeKeyFrame_Lite");
        return PTAM_E_STATE;
    }
    ptam_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    void* hp;
    rc = ctx_pinned(ctx, 256, &hp);
    if (rc) return rc;
    const int ntake = max(0, min(max_initial, t->max_trails));
    HIP_TRY(hipMemsetAsync(t->hdr, 0, 16, ctx->stream));
    hipLaunchKernelGGL(trails_start_kernel, dim3(64), dim3(256), 0, ctx->stream, first->L, t->w, t->h, min_shi_tomasi, ntake, t->trails[0],
                       t->slot[0], t->patches, t->hdr);
    hipLaunchKernelGGL(trails_keep_kernel, dim3(KEEP_BLOCKS), dim3(256), 0, ctx->stream, first->L, t->prev, t->w, t->h);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp, t->hdr, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    t->cur = 0;
    t->n_live = ((const int*)hp)[HDR_LIVE];
    t->started = 1;
    *n_trails = t->n_live;
    return PTAM_OK;
}

int ptam_trails_advance(ptam_trails* t, const ptam_kf* current, int* n_good, int* n_alive) {
    ARG_TRY(t && current && n_good && n_alive);
    int rc = trails_check_kf(t, current);
    if (rc) return rc;
    rc = trails_need_start(t, "trails_advance");
    if (rc) return rc;
    ptam_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    void* hp;
    rc = ctx_pinned(ctx, 256, &hp);
    if (rc) return rc;
    const int n = t->n_live, a = t->cur, b = 1 - t->cur;
    if (n > 0)
        hipLaunchKernelGGL(trails_search_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, current->L, t->prev, t->w, t->h, n,
                           (const ptam_trail*)t->trails[a], (const int*)t->slot[a], (const uint8_t*)t->patches, t->status, t->newpos);
    hipLaunchKernelGGL(trails_compact_kernel, dim3(1 + KEEP_BLOCKS), dim3(1024), 0, ctx->stream, current->L, t->prev, t->w, t->h, n,
                       (const ptam_trail*)t->trails[a], (const int*)t->slot[a], (const int*)t->status, (const ptam_int2*)t->newpos,
                       t->trails[b], t->slot[b], t->hdr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hp, t->hdr, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    t->cur = b;
    t->n_live = ((const int*)hp)[HDR_LIVE];
    *n_good = ((const int*)hp)[HDR_GOOD];
    *n_alive = t->n_live;
    return PTAM_OK;
}

// What ptam_trails_advance_batch refuses before it looks further (no HIP call, nothing written): the conditions of the tracker's batch
// calls — one device, one image geometry and halfSample variant, no object, keyframe or context twice — and a start on every object.
static int trails_batch_check(int nb, ptam_trails* const* ts, ptam_kf* const* curs, const int32_t* n_good, const int32_t* n_alive) {
    ARG_TRY(nb >= 1 && nb <= 4096 && ts && curs && n_good && n_alive);
    for (int i = 0; i < nb; i++) ARG_TRY(ts[i] && curs[i]);
    const ptam_ctx* ctx = ts[0]->ctx;
    const KfLevels& L0 = curs[0]->L;
    for (int i = 0; i < nb; i++) {
        ARG_TRY(ts[i]->ctx->device == ctx->device && ts[i]->ctx->halfsample == ctx->halfsample);
        ARG_TRY(ts[i]->w == ts[0]->w && ts[i]->h == ts[0]->h);
        if (int rc = trails_check_kf(ts[i], curs[i])) return rc;
        ARG_TRY(curs[i]->n_blocks == curs[0]->n_blocks);
        for (int l = 0; l < PTAM_LEVELS; l++) ARG_TRY(curs[i]->L.w[l] == L0.w[l] && curs[i]->L.h[l] == L0.h[l]);
        for (int j = 0; j < i; j++) ARG_TRY(ts[j] != ts[i] && curs[j] != curs[i] && ts[j]->ctx != ts[i]->ctx);
    }
    for (int i = 0; i < nb; i++)
        if (int rc = trails_need_start(ts[i], "trails_advance_batch")) return rc;
    return PTAM_OK;
}

int ptam_trails_advance_batch(int nb, ptam_trails* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, int32_t* n_good,
                              int32_t* n_alive) {
    int rc = trails_batch_check(nb, ts, curs, n_good, n_alive);
    if (rc) return rc;
    ptam_trails* lead = ts[0];
    ptam_ctx* ctx = lead->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    // the chain runs on the lead's queue: whatever the other objects' own queues still hold (a start, a keyframe) must be done
    for (int i = 1; i < nb; i++) HIP_TRY(ptam_stream_wait(ts[i]->ctx->stream));
    const size_t bytes = (size_t)nb * sizeof(TrailJob);
    void* pin;
    rc = ctx_pinned(ctx, bytes, &pin);
    if (rc) return rc;
    if (lead->batch_cap < bytes) {
        HIP_TRY(ptam_stream_wait(st));
        if (lead->batch_dev) HIP_TRY(hipFree(lead->batch_dev));
        lead->batch_dev = nullptr;
        lead->batch_cap = 0;
        HIP_TRY(hipMalloc(&lead->batch_dev, bytes * 2));
        lead->batch_cap = bytes * 2;
    }
    TrailJob* hj = (TrailJob*)pin;
    const TrailJob* dj = (const TrailJob*)lead->batch_dev;
    int n_max = 0;
    for (int i = 0; i < nb; i++) {
        ptam_trails* t = ts[i];
        const int a = t->cur, b = 1 - t->cur;
        TrailJob& j = hj[i];
        std::memset(&j, 0, sizeof j);
        j.C = curs[i]->L;
        j.P = t->prev;
        j.n = t->n_live;
        j.tin = t->trails[a];
        j.sin = t->slot[a];
        j.patches = t->patches;
        j.status = t->status;
        j.newpos = t->newpos;
        j.tout = t->trails[b];
        j.sout = t->slot[b];
        j.hdr = t->hdr;
        j.done = t->done_dev;
        j.seq = t->seq + 1;
        n_max = std::max(n_max, t->n_live);
    }
    HIP_TRY(hipMemcpyAsync(lead->batch_dev, hj, bytes, hipMemcpyHostToDevice, st));
    for (int i = 0; i < nb; i++) {
        // an object whose last batch never came back (PTAM_E_HIP below): its arrival count may stand anywhere
        if (ts[i]->in_flight) HIP_TRY(hipMemsetAsync(ts[i]->hdr + HDR_ARRIVED, 0, sizeof(int), st));
        if (d_frames && d_frames[i]) {   // (a failure here leaves the keyframes before it made and every trails object as it was)
            rc = kf_make_lite_on(ts[i]->ctx, curs[i], d_frames[i], st);
            if (rc) return rc;
        }
    }
    for (int i = 0; i < nb; i++) ts[i]->seq++, ts[i]->in_flight = 1;   // (from here on the device may write the word)
    if (n_max > 0) hipLaunchKernelGGL(trails_search_batch_kernel, dim3((n_max + 3) / 4, nb), dim3(256), 0, st, dj, lead->w, lead->h);
    hipLaunchKernelGGL(trails_compact_batch_kernel, dim3(1 + KEEP_BLOCKS, nb), dim3(1024), 0, st, dj, lead->w, lead->h);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < nb; i++) {
        const volatile unsigned long long* word = &ts[i]->done->seq;
        const unsigned long long seq = ts[i]->seq;
        rc = ptam_wait_mapped(st, "a camera's trail counts", [&] { return *word == seq; });
        if (rc) return rc;   // (the queue died: no object is committed, each keeps its list of before; the next batch clears the counts)
    }
    for (int i = 0; i < nb; i++) {   // every camera has arrived: the lists change hands
        ptam_trails* t = ts[i];
        t->cur = 1 - t->cur;
        t->in_flight = 0;
        t->n_live = t->done->live;
        n_good[i] = t->done->good;
        n_alive[i] = t->done->live;
    }
    return PTAM_OK;
}

// a read-back of n_live records of `bytes` each from d (device) through the pinned staging
static int trails_download(ptam_trails* t, const void* d, size_t bytes, void* out) {
    ptam_ctx* ctx = t->ctx;
    if (t->n_live == 0) return PTAM_OK;
    void* hp;
    int rc = ctx_pinned(ctx, bytes * (size_t)t->n_live, &hp);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(hp, d, bytes * (size_t)t->n_live, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    std::memcpy(out, hp, bytes * (size_t)t->n_live);
    return PTAM_OK;
}

int ptam_trails_read(ptam_trails* t, ptam_trail* out, int cap, int* n) {
    ARG_TRY(t && n && (out || cap == 0));
    int rc = trails_need_start(t, "trails_read");
    if (rc) return rc;
    ARG_TRY(cap >= t->n_live);
    HIP_TRY(hipSetDevice(t->ctx->device));
    rc = trails_download(t, t->trails[t->cur], sizeof(ptam_trail), out);
    if (rc) return rc;
    *n = t->n_live;
    return PTAM_OK;
}

int ptam_trails_read_patches(ptam_trails* t, uint8_t* out, int cap, int* n) {
    ARG_TRY(t && n && (out || cap == 0));
    int rc = trails_need_start(t, "trails_read_patches");
    if (rc) return rc;
    ARG_TRY(cap >= t->n_live);
    HIP_TRY(hipSetDevice(t->ctx->device));
    if (t->n_live > 0) {
        const int nb = t->n_live * TRAIL_PATCH_BYTES;
        hipLaunchKernelGGL(trails_gather_patches_kernel, dim3((nb + 255) / 256), dim3(256), 0, t->ctx->stream, t->n_live,
                           (const int*)t->slot[t->cur], (const uint8_t*)t->patches, (uint8_t*)t->out);
        HIP_TRY(hipGetLastError());
    }
    rc = trails_download(t, t->out, TRAIL_PATCH_BYTES, out);
    if (rc) return rc;
    *n = t->n_live;
    return PTAM_OK;
}

int ptam_trails_matches(ptam_trails* t, ptam_homography_match* out, int cap, int* n) {
    ARG_TRY(t && n && (out || cap == 0));
    int rc = trails_need_start(t, "trails_matches");
    if (rc) return rc;
    ARG_TRY(cap >= t->n_live);
    HIP_TRY(hipSetDevice(t->ctx->device));
    if (t->n_live > 0) {
        hipLaunchKernelGGL(trails_matches_kernel, dim3((t->n_live + 255) / 256), dim3(256), 0, t->ctx->stream, t->ctx->cam, t->n_live,
                           (const ptam_trail*)t->trails[t->cur], (ptam_homography_match*)t->out);
        HIP_TRY(hipGetLastError());
    }
    rc = trails_download(t, t->out, sizeof(ptam_homography_match), out);
    if (rc) return rc;
    *n = t->n_live;
    return PTAM_OK;
}

int ptam_trails_homography(ptam_trails* t, const ptam_homography_opts* opts, double se3_second_from_first[12], ptam_homography_info* info,
                           uint8_t* inlier_out) {
    ARG_TRY(t && opts && se3_second_from_first && info);
    int rc = trails_need_start(t, "trails_homography");
    if (rc) return rc;
    rc = homog_check(t->n_live, opts);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(t->ctx->device));
    hipLaunchKernelGGL(trails_matches_kernel, dim3((t->n_live + 255) / 256), dim3(256), 0, t->ctx->stream, t->ctx->cam, t->n_live,
                       (const ptam_trail*)t->trails[t->cur], (ptam_homography_match*)t->out);
    HIP_TRY(hipGetLastError());
    return homog_run(t->ctx, t->n_live, (const ptam_homography_match*)t->out, nullptr, opts, se3_second_from_first, info, inlier_out);
}

int ptam_init_points_from_trails(ptam_ctx* ctx, const ptam_kf* first, ptam_kf* second, const double se3_second_from_first[12], int n,
                                 const ptam_trail* matches, int subpix_max_its, ptam_new_map_point* out, int32_t* status, int32_t* n_out) {
    ARG_TRY(ctx && first && second && se3_second_from_first && n_out && n >= 0);
    ARG_TRY(n == 0 || (matches && out && status));
    ARG_TRY(first->device == ctx->device && second->device == ctx->device);
    ARG_TRY(first->L.w[0] == second->L.w[0] && first->L.h[0] == second->L.h[0]);
    *n_out = 0;
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_m = up(sizeof(ptam_trail) * (size_t)n), b_st = up(sizeof(int) * (size_t)n), b_pts = sizeof(ptam_new_map_point) * (size_t)n;
    void *s, *hp;
    int rc = ctx_scratch(ctx, b_m + b_st + b_pts, &s);
    if (rc) return rc;
    rc = ctx_pinned(ctx, b_st + b_pts, &hp);
    if (rc) return rc;
    ptam_trail* d_m = (ptam_trail*)s;
    int* d_st = (int*)((char*)s + b_m);
    ptam_new_map_point* d_pts = (ptam_new_map_point*)((char*)s + b_m + b_st);
    // (pageable: staged before the call returns, which is after the final wait)
    HIP_TRY(hipMemcpyAsync(d_m, matches, sizeof(ptam_trail) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    rc = init_points_enqueue(ctx, first, second, se3_second_from_first, subpix_max_its, n, d_m, d_st, d_pts);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(hp, d_st, b_st + b_pts, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    const int* h_st = (const int*)hp;
    const ptam_new_map_point* h_pts = (const ptam_new_map_point*)((const char*)hp + b_st);
    int made = 0;
    for (int i = 0; i < n; i++) {   // mMap.vpPoints.push_back(p): match order
        status[i] = h_st[i];
        if (h_st[i] == PTAM_INIT_MADE) out[made++] = h_pts[i];
    }
    *n_out = made;
    return PTAM_OK;
}

}   // extern "C"

void trails_preload_kernels() {
    ptam_preload((const void*)trails_start_kernel);
    ptam_preload((const void*)trails_keep_kernel);
    ptam_preload((const void*)trails_search_kernel);
    ptam_preload((const void*)trails_compact_kernel);
    ptam_preload((const void*)trails_search_batch_kernel);
    ptam_preload((const void*)trails_compact_batch_kernel);
    ptam_preload((const void*)trails_matches_kernel);
    ptam_preload((const void*)trails_gather_patches_kernel);
    ptam_preload((const void*)init_points_kernel);
}
