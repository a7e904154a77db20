// trackmap.hip — Tracker::TrackMap (src/Tracker.cc:442-696) as ONE device-resident chain.
//
// The reference's frame is  PVS loop (:453-478)  ->  choice of the coarse / top-level / fine search sets (:480-611)  ->
// SearchForPoints on the coarse set, range 30, 8 sub-pixel iterations (:549)  ->  ten coarse pose iterations (:554-568)  ->
// SearchForPoints on the remaining top-level points (sub-pixel) and on the fine set (:572-610)  ->  ten fine pose
// iterations (:613-643)  ->  measurement / scene-depth bookkeeping (:660-696).  Which sets are searched, whether the coarse
// stage counts (nFound >= CoarseMin), the fine search range (5 or 10) and every list length are decided from data that only
// exists on the device, so the whole chain is enqueued at once: list lengths, slot ranges and the stage flags live in a
// small control block (TmCtl) that the kernels read; nothing comes back to the host before the final result.
//
// std::random_shuffle (:483-484, :598) is replaced by caller-provided permutations of the map-point ids: level l's
// list is taken in the order its members appear in `shuffle_levels` (the order a uniform permutation induces on a subset is
// itself uniform), the chop of the fine set likewise with `shuffle_fine`.
//
// Per map point the chain keeps the reference's TrackerData (v3Cam, v2Image, m2CamDerivs) in the PVS result table and
// carries it from stage to stage exactly as the reference does: the fine loop's iteration 0 does not re-project
// (:617), so a point found in the coarse stage enters it with the state the coarse loop left, a point of the later sets
// with its re-projection at the post-coarse pose and the camera derivatives of the PVS pass (ProjectAndDerivs only
// refreshes them for found points, include/Tracker.h:89-94).
#include <climits>
#include <memory>

#include "track_internal.h"
#include "sbi.h"                  // ptam_track_frames_batch: the estimators' steps of a batch
#include "snapshot_internal.h"    // ptam_map_snapshot: ptam_tracker_take_map copies its current slot
#include "wait_mapped.h"
#include "../../include/ptam_hip_bench.h"
#include "patch_device.h"
#include "keyframe_device.h"
#include "pvs_device.h"
#include "pose_device.h"
#include "framereport_internal.h"   // ptam_tracker_report_frames: FrJob, fr_fill_core

struct TmCtl {
    int n_lvl[4];           // avPVS[l].size() after the PVS loop
    int nC, nH, nF, n_slots;
    int do_coarse;          // the coarse search runs (:519)
    int did_coarse;         // mbDidCoarse (:551)
    int n_found_coarse;     // nFound of the coarse SearchForPoints
    int n_meas_coarse;      // measurements of the coarse pose loop (0 unless did_coarse)
    int n_meas;             // found entries of vIterationSet
    int fine_range;         // nFineRange (:572)
    int attempted[4], found[4];   // manMeasAttempted / manMeasFound
    int range_all[2], range_c[2], range_hf[2], range_h[2];   // slot ranges {first, end} of the stages
    int n_reused;           // searched patches whose PatchFinder kept its template (src/PatchFinder.cc:103-111)
    int outlier_by_slot;    // d.outlier is indexed by search slot (fused pose kernels) instead of by compacted measurement
    double depth[3];        // sum z, sum z^2, count over the found points (:680-690)
};

// The PatchFinder of a map point (TrackerData::Finder, include/Tracker.h:52), the part of its state that outlives a frame:
// MakeTemplateCoarseCont (src/PatchFinder.cc:98-127) keeps the template — and mbTemplateBad with it — when the finder last
// warped THIS point and neither column of the warp m2 has moved by more than 0.07 since.  (The finder is per point here, so
// "the same map point" is "a template was made at all".)
struct TmFinder {
    double m2[4];           // mm2LastWarpMatrix {m00, m01, m10, m11}
    int valid;              // mpLastTemplateMapPoint == &p
    int bad;                // mbTemplateBad
    int sum, sum_sq;        // MakeTemplateSums
    uint8_t tpl[64];        // mimTemplate
};

// What a search slot hands to the pose loop, written by the search wave when it is done with the slot, FIELD-MAJOR (plane f holds
// field f of every slot): the pose kernel's prologue needs a single round trip — status, point id, position and TrackerData state
// used to be four arrays, two of them behind the point id — and its loads are coalesced (slot-major 120-byte records cost a wave 60
// load instructions of 64 cache lines each: 8.7 k cycles of the fine loop's prologue).
//   planes 0-2 v3WorldPos | 3-4 v2Found | 5-7 v3Cam | 8-9 v2Image | 10-13 m2CamDerivs  (doubles);  tag: {status word, map point}
#define TM_REC_F 14
struct TmDev {
    int n, cap;
    ptam_pvs_point* pts;
    TmSrc* src;
    int* perm_a;
    int* perm_b;
    ptam_pvs_result* pvs;     // proj = the point's TrackerData state
    int* lvl_list;            // [4][cap]
    uint8_t* isfc;            // [cap] member of the fine candidate set
    int* list;                // [cap] search slots: coarse | top level | fine
    ptam_template_result* tres;
    ptam_patch_query* q;
    ptam_patch_result* r;
    ptam_subpix_result* sr;
    int* slot_found;
    int* slot_stat;           // per slot: found | attempted << 1 | level << 2, written by the search kernel
    int* slot_subpix;
    double2* slot_v2;
    double* recf;             // [TM_REC_F][cap] per slot: everything the pose loop wants of it (written by the search wave, state refreshed by the coarse pose loop)
    int2* rect;               // [cap] {slot_stat, map point}
    ptam_pose_meas* meas;
    ptam_projection* entry;
    int* midx;                // measurement -> map point
    int* mslot;               // measurement -> slot
    int* outlier;             // per measurement (fine loop, iteration 9)
    TmCtl* ctl;
    double* pose;
    TmFinder* finder;         // [cap] per-point PatchFinder state
};

// exclusive block scan of four counters at once (1024 threads): returns this thread's four offsets, totals in tot[]
__device__ __forceinline__ void block_scan4(const int v[4], int off[4], int tot[4], int (*wsum)[16]) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int incl[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const int x = wave_incl_scan_i32(v[l]);   // (DPP: a __shfl_up ladder is six LDS round trips per counter)
        incl[l] = x;
        if (lane == 63) wsum[l][wid] = x;
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 4; l++) {
        int base = 0, total = 0;
        for (int w = 0; w < 16; w++) {
            const int s = wsum[l][w];
            if (w < wid) base += s;
            total += s;
        }
        off[l] = base + incl[l] - v[l];
        tot[l] = total;
    }
    __syncthreads();
}

// The choice of the search sets, src/Tracker.cc:480-611.  One workgroup.  The level lists and the fine-candidate flags live
// in LDS when the map has at most TM_SEL_LDS points (global scratch otherwise): a list written to global memory and read
// back by another thread of the workgroup costs two round trips per pass, and this kernel is a chain of such passes.
#ifndef TM_SEL_LDS
#define TM_SEL_LDS 8192   // 4 x 32 KB level lists + 8 KB flags = 136 KB of the CU's 160 KB (2048 until round 2c: a 2 561-point map
                          // cost 18 us more per frame than a 1 998-point one)
#endif
__device__ __forceinline__ void tm_select_body(const TmDev& d, const ptam_trackmap_opts& o) {   // a 1024-thread workgroup
    __shared__ int wsum[4][16];
    __shared__ int ls_list[4][TM_SEL_LDS];
    __shared__ uint8_t ls_isfc[TM_SEL_LDS];
    const int tid = threadIdx.x, n = d.n, cap = d.cap;
    const bool lds = n <= TM_SEL_LDS;
    const int chunk = (n + 1023) / 1024, p0 = min(n, tid * chunk), p1 = min(n, p0 + chunk);
    // both permutations' entries of my run and the levels of the first one's points leave together
    constexpr int RUNMAX = TM_SEL_LDS / 1024;   // (longer runs — maps that do not fit the LDS lists — reload inside the loops)
    int ida[RUNMAX], idb[RUNMAX], lva[RUNMAX];
#pragma unroll
    for (int j = 0; j < RUNMAX; j++) {
        ida[j] = idb[j] = 0;
        lva[j] = -1;
        if (chunk <= RUNMAX && p0 + j < p1) {
            ida[j] = d.perm_a[p0 + j];
            idb[j] = d.perm_b[p0 + j];
        }
    }
#pragma unroll
    for (int j = 0; j < RUNMAX; j++)
        if (chunk <= RUNMAX && p0 + j < p1) lva[j] = d.pvs[ida[j]].level;
    // f(id of the first permutation, its level, id of the second permutation) over my run, in order
    auto for_run = [&](auto&& f) {
        if (chunk <= RUNMAX) {
#pragma unroll
            for (int j = 0; j < RUNMAX; j++)
                if (p0 + j < p1) f(ida[j], lva[j], idb[j]);
        } else
            for (int p = p0; p < p1; p++) {
                const int ia = d.perm_a[p];
                f(ia, (int)d.pvs[ia].level, d.perm_b[p]);
            }
    };
    auto set_fc = [&](int id, int v) { if (lds) ls_isfc[id] = (uint8_t)v; else d.isfc[id] = (uint8_t)v; };
    auto get_fc = [&](int id) { return lds ? (int)ls_isfc[id] : (int)d.isfc[id]; };
    auto LL = [&](int l, int i) -> int { return lds ? ls_list[l][i] : d.lvl_list[l * cap + i]; };
    // level lists in the order the shuffle permutation visits their members
    int cnt[4] = {0, 0, 0, 0};
    for_run([&](int id, int l, int) {
        set_fc(id, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) cnt[q] += (l == q) ? 1 : 0;
    });
    int off[4], tot[4];
    block_scan4(cnt, off, tot, wsum);
    for_run([&](int id, int l, int) {
        if (l >= 0) {
            int at = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (l == q) at = off[q]++;
            if (lds)
                ls_list[l][at] = id;
            else
                d.lvl_list[l * cap + at] = id;
        }
    });
    __syncthreads();
    const int n3 = tot[3], n2 = tot[2], n1 = tot[1], n0 = tot[0];
    const int cmax = (int)o.coarse_max;
    // coarse set (:519-546)
    const int do_coarse = o.try_coarse && ((unsigned)(n3 + n2) > o.coarse_min);
    int t3 = 0, t2 = 0, nC3 = 0, nC2 = 0;
    if (do_coarse) {
        t3 = min(n3, cmax);   // all of level 3, or CoarseMax of it; either way they leave avPVS[3]
        nC3 = t3;
        if (nC3 < cmax) {
            const int need = cmax - nC3;
            if (n2 <= need) {
                // :538 ASSIGNS avPVS[LEVELS-2] to vNextToSearch: the level-3 picks made above are dropped from the frame
                // (they are neither searched nor left in the PVS).  Kept as the reference does it.
                nC3 = 0;
                nC2 = n2;
                t2 = n2;
            } else {
                nC2 = need;
                t2 = need;
            }
        }
    }
    const int nC = nC3 + nC2, nH = n3 - t3;
    const int nFC = (n2 - t2) + n1 + n0;
    const int n_use = max(0, o.max_patches - (nC + nH));   // :594-596
    const bool chop = nFC > n_use;
    const int nF = chop ? n_use : nFC;
    for (int s = tid; s < nC; s += 1024) d.list[s] = s < nC3 ? LL(3, s) : LL(2, s - nC3);
    for (int s = tid; s < nH; s += 1024) d.list[nC + s] = LL(3, t3 + s);
    // fine candidates in the order of :588-590: levels 2, 1, 0
    for (int s = tid; s < nFC; s += 1024) {
        const int a = n2 - t2;
        const int id = s < a ? LL(2, t2 + s) : (s < a + n1 ? LL(1, s - a) : LL(0, s - a - n1));
        if (chop)
            set_fc(id, 1);
        else
            d.list[nC + nH + s] = id;
    }
    if (chop) {
        // random_shuffle + resize (:597-600): the first n_use members in the order of the second permutation
        __syncthreads();
        int c4[4] = {0, 0, 0, 0};
        for_run([&](int, int, int id) { c4[0] += get_fc(id); });
        int o4[4], t4[4];
        block_scan4(c4, o4, t4, wsum);
        int k = o4[0];
        for_run([&](int, int, int id) {
            if (get_fc(id)) {
                if (k < n_use) d.list[nC + nH + k] = id;
                k++;
            }
        });
    }
    if (tid == 0) {
        TmCtl& c = *d.ctl;
        c.n_lvl[0] = n0, c.n_lvl[1] = n1, c.n_lvl[2] = n2, c.n_lvl[3] = n3;
        c.nC = nC, c.nH = nH, c.nF = nF, c.n_slots = nC + nH + nF;
        c.do_coarse = do_coarse;
        c.did_coarse = 0;
        c.n_found_coarse = c.n_meas_coarse = c.n_meas = 0;
        c.n_reused = 0;
        c.fine_range = 10;
        for (int l = 0; l < 4; l++) c.attempted[l] = c.found[l] = 0;
        c.range_all[0] = 0, c.range_all[1] = nC + nH + nF;
        c.range_c[0] = 0, c.range_c[1] = nC;
        c.range_hf[0] = nC, c.range_hf[1] = nC + nH + nF;
        c.range_h[0] = nC, c.range_h[1] = nC + nH;
        c.depth[0] = c.depth[1] = c.depth[2] = 0;
    }
}

__global__ void __launch_bounds__(1024) tm_select_kernel(TmDev d, ptam_trackmap_opts o) { tm_select_body(d, o); }

// ---- horizontal fusion for a frame that arrives with its image (ptam_track_map_frame) ----
// The PVS pass and the set choice do not look at the image, the pyramid and the corner compaction do not look at the map:
// run on separate queues the two cross-queue waits cost more than the overlap (measured, see track_map_impl), but as
// workgroups of ONE launch they overlap for free — every kernel of this chain leaves most of the chip idle.
//   launch 1: pyramid (its 2-D grid linearised) | PVS pass        launch 2: FAST detect
//   launch 3: set choice (workgroup 0) | raster-ordered corner compaction (9 independent workgroups at 640x480)
template <int VARIANT>
__global__ void __launch_bounds__(256) tm_pyr_pvs_kernel(PyrArgs a, int gx, int n_pyr, DevCam cam, int n, const ptam_pvs_point* __restrict__ pts,
                                                         ptam_pvs_result* __restrict__ out, PoseArg pv, double* __restrict__ pose_out,
                                                         int* __restrict__ finder_bad) {
    const int b = blockIdx.x;
    if (b < n_pyr)
        pyramid_body<VARIANT>(a, (b % gx) * 64 + (threadIdx.x & 63), (b / gx) * 4 + (threadIdx.x >> 6));
    else
        track_pvs_body(cam, n, pts, pose_out, out, nullptr, pv, pose_out, b - n_pyr, finder_bad, (int)sizeof(TmFinder));
}
// (round 4) launch 1 of a tracked frame: the keyframe's tiles — pyramid pixels + FAST test per tile (keyframe_device.h:
// kf_fused_tile_body) — beside the PVS pass; launch 2: set choice | corner compaction.  One launch and the pyramid kernel less.
template <int VARIANT>
__global__ void __launch_bounds__(256) tm_kf_pvs_kernel(PyrArgs a, KfLevels L, int n_tiles, DevCam cam, int n, const ptam_pvs_point* __restrict__ pts,
                                                        ptam_pvs_result* __restrict__ out, PoseArg pv, double* __restrict__ pose_out,
                                                        int* __restrict__ finder_bad) {
    // workgroup order = start order: the PVS blocks first, then the tiles from the coarsest level (the longest cascade) down
    const int n_pvs = (int)gridDim.x - n_tiles, b = blockIdx.x;
    if (b < n_pvs)
        track_pvs_body(cam, n, pts, pose_out, out, nullptr, pv, pose_out, b, finder_bad, (int)sizeof(TmFinder));
    else
        kf_fused_tile_body<VARIANT>(a, L, n_tiles - 1 - (b - n_pvs));
}
__global__ void __launch_bounds__(1024) tm_compact_select_kernel(KfLevels L, TmDev d, ptam_trackmap_opts o) {
    if (blockIdx.x == 0)
        tm_select_body(d, o);
    else
        fast_compact_body(L, blockIdx.x - 1, 0);
}


// Tracker::SearchForPoints (src/Tracker.cc:867-912) for the slots of a stage, ONE WAVE PER SLOT, everything a patch needs
// in one pass of that wave: [stage 1: TrackerData::Project at the current pose — :573-574 always for the top-level set,
// :606-608 for the fine set if the coarse stage counted; bFound is false here, so the derivatives stay, include/Tracker.h:89-94]
// -> MakeTemplateCoarseCont (:873; the template never leaves the wave's registers) -> FindPatchCoarse at ir(v2Image) (:881)
// -> MakeSubPixTemplate + IterateSubPixToConvergence where the stage asks for it (:896-906: the coarse set with
// CoarseSubPixIts, the top-level set with 8, the fine set not at all).  Every lane computes the same scalars (wave-uniform
// control flow); lane 0 stores.  stage 0: the coarse set; stage 1: top-level and fine sets.
__device__ __forceinline__ void tm_search_body(const DevCam& cam, const KfLevels& L, const TmDev& d, int stage, unsigned coarse_range,
                                               int coarse_its, int bx) {   // a 256-thread workgroup: four slots
    // (the slot is the workgroup's own — the launch covers the slots from 0 — so that the point id is requested together with
    //  the control block, not behind it: one dependent round trip less at the head of every search wave)
    const int s = bx * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
#ifdef K7_TIMING
    const long long ts0_ = (long long)__builtin_readcyclecounter();
#endif
    const int id = d.list[min(s, d.cap - 1)];
    const TmCtl& c = *d.ctl;
    const int first = stage == 0 ? c.range_c[0] : c.range_hf[0], end = stage == 0 ? c.range_c[1] : c.range_hf[1];
    if (s < first || s >= end) return;
    ptam_pvs_result& pv = d.pvs[id];
    // the point's PatchFinder state, requested with the point's TrackerData (one round trip, not one more behind the decision)
    TmFinder& fs = d.finder[id];
    const double fm0 = fs.m2[0], fm1 = fs.m2[1], fm2 = fs.m2[2], fm3 = fs.m2[3];
    const int f_valid = fs.valid, f_bad = fs.bad, f_sum = fs.sum, f_sum_sq = fs.sum_sq, f_tpl = fs.tpl[lane];
    double u = pv.proj.image[0], v = pv.proj.image[1];
    const ptam_pvs_point& p = d.pts[id];
    const double pw0 = p.world[0], pw1 = p.world[1], pw2 = p.world[2];
    const TmSrc sr = d.src[id];   // (with the point's other records: behind the re-projection it was a round trip of its own)
    const int pv_level = pv.level;
    double pwi[4];
#pragma unroll
    for (int k = 0; k < 4; k++) pwi[k] = pv.warp_inverse[k];
    double pcam0 = pv.proj.cam[0], pcam1 = pv.proj.cam[1], pcam2 = pv.proj.cam[2];
    const double pd0 = pv.proj.derivs[0], pd1 = pv.proj.derivs[1], pd2 = pv.proj.derivs[2], pd3 = pv.proj.derivs[3];
    if (stage == 1 && (s < c.range_h[1] || c.did_coarse)) {
        double X, Y, Z;
        se3_apply(d.pose, pw0, pw1, pw2, X, Y, Z);
        int in_image = 0;
        bool reached = false;
        if (!(Z < 0.001)) {
            const double x = X / Z, y = Y / Z;
            if (!(x * x + y * y > cam.largest_radius * cam.largest_radius)) {
                double rr, f;
                cam_project(cam, x, y, u, v, rr, f);
                reached = true;
                if (!(rr > cam.max_r) && !(u < 0 || v < 0 || u > cam.width || v > cam.height)) in_image = 1;
            }
        }
        if (lane == 0) {
            pv.proj.cam[0] = X, pv.proj.cam[1] = Y, pv.proj.cam[2] = Z;
            if (reached) pv.proj.image[0] = u, pv.proj.image[1] = v;
            pv.proj.in_image = in_image;
        }
        pcam0 = X, pcam1 = Y, pcam2 = Z;   // (u, v: the new position if the projection got that far, the old one otherwise)
    }
    ptam_patch_query q;
    q.x = (int)u;   // ir(): truncation
    q.y = (int)v;
    q.level = pv_level;
    q.range = stage == 0 ? coarse_range : (unsigned)c.fine_range;
    TemplateJob jb;
    jb.im = sr.im;
    jb.w = sr.w;
    jb.h = sr.h;
    jb.search_level = pv_level;
    jb.cx = sr.cx;
    jb.cy = sr.cy;
#pragma unroll
    for (int k = 0; k < 4; k++) jb.wi[k] = pwi[k];
    // MakeTemplateCoarseCont (src/PatchFinder.cc:98-127): re-make the template unless this finder's last one was made with
    // (nearly) this warp — then the template, its sums and mbTemplateBad stay as they are
    ptam_template_result tr;
    int T, kept = 0;
#ifdef K7_TIMING
    const long long ts1_ = (long long)__builtin_readcyclecounter();
#endif
    {
        double m2[4];
        template_m2(jb, m2);
        const double c0x = m2[0] - fm0, c0y = m2[2] - fm2, c1x = m2[1] - fm1, c1y = m2[3] - fm3;   // columns m2.T()[0], m2.T()[1]
        const double lim = 0.07 * 0.07;
        const bool refresh = !f_valid || pv_level < 0 || c0x * c0x + c0y * c0y > lim || c1x * c1x + c1y * c1y > lim;
        if (refresh) {
            T = wave_make_template(jb, lane, tr);
            fs.tpl[lane] = (uint8_t)T;
            if (lane == 0 && pv_level >= 0) {
                fs.m2[0] = tr.m2[0], fs.m2[1] = tr.m2[1], fs.m2[2] = tr.m2[2], fs.m2[3] = tr.m2[3];
                fs.valid = 1;
                fs.bad = tr.bad;
                fs.sum = tr.sum;
                fs.sum_sq = tr.sum_sq;
            }
        } else {
            T = f_tpl;
            tr.bad = f_bad;
            tr.n_outside = 0;
            tr.sum = f_sum;
            tr.sum_sq = f_sum_sq;
            tr.m2[0] = fm0, tr.m2[1] = fm1, tr.m2[2] = fm2, tr.m2[3] = fm3;
            kept = 1;   // (counted by the gather pass from the slot's status word: a thousand atomics on one counter cost 5 us)
        }
    }
    ptam_patch_result res;
#ifdef K7_TIMING
    const long long ts2_ = (long long)__builtin_readcyclecounter();
#endif
    __shared__ __attribute__((aligned(16))) unsigned sw_win[4][SW_BYTES / 4];   // (a wave's own search region: no barrier)
    wave_find_patch_coarse(L, q, !tr.bad, T, lane, res, sw_win[threadIdx.x >> 6]);
#ifdef K7_TIMING
    const long long ts3_ = (long long)__builtin_readcyclecounter();
#endif
    if (lane == 0) {
        d.tres[s] = tr;
        d.q[s] = q;
        d.r[s] = res;
        if (tr.bad) pv.proj.in_image = 0;   // TD.bInImage = false (:877)
    }
    const int its = stage == 0 ? coarse_its : (s < c.range_h[1] ? 8 : 0);
    ptam_subpix_result sres;
    sres.converged = 0;
    sres.iterations = 0;
    sres.pos[0] = sres.pos[1] = 0;
    if (its > 0) {
        ptam_subpix_query sq;
        sq.level = (q.level >= 0 && !tr.bad && res.found) ? q.level : -1;
        sq.max_its = its;
        sq.coarse_pos[0] = res.pos[0];
        sq.coarse_pos[1] = res.pos[1];
        __shared__ uint8_t sp_win[4][256];   // (a wave's own 16 x 16 window: no barrier)
        wave_subpix(L, sq, T, lane, sres, sp_win[threadIdx.x >> 6]);
        if (lane == 0) d.sr[s] = sres;
    }
#ifdef K7_TIMING
    if (lane == 0 && (s == 3 || s == 40 || s == 500) && (clock64() & 0x3f000) == 0)
        printf("search wave stage %d slot %d level %d kept %d its %d(%d): loads %lld | template %lld | search %lld (scored %d) | sub-pixel %lld\n", stage, s, q.level,
               kept, its, sres.iterations, ts1_ - ts0_, ts2_ - ts1_, ts3_ - ts2_, res.n_scored, (long long)__builtin_readcyclecounter() - ts3_);
#endif
    // the slot's outcome (the tail of SearchForPoints, :880-906), for the gather pass: one packed word + the position
    double2 v2pub = make_double2(0, 0);
    if (lane == 0) {
        const bool att = q.level >= 0 && !tr.bad;   // manMeasAttempted (:880)
        int found = att && res.found, sub = 0;
        double2 v2 = make_double2(0, 0);
        if (found) {
            if (its > 0) {
                sub = 1;
                found = sres.converged;   // :898-904
                v2 = make_double2(sres.pos[0], sres.pos[1]);
            } else
                v2 = make_double2(res.pos[0], res.pos[1]);
        }
        d.slot_found[s] = found;
        d.slot_subpix[s] = sub;
        d.slot_v2[s] = v2;
        v2pub = v2;
        const int stat = found | ((int)att << 1) | ((q.level & 3) << 2) | (kept << 4);
        d.slot_stat[s] = stat;
        d.rect[s] = make_int2(stat, id);
    }
    {
        // the slot's record: lane f stores field f (one store instruction for the fourteen planes)
        const double2 v2r = make_double2(__shfl(v2pub.x, 0, 64), __shfl(v2pub.y, 0, 64));
        const double fld[TM_REC_F] = {pw0, pw1, pw2, v2r.x, v2r.y, pcam0, pcam1, pcam2, u, v, pd0, pd1, pd2, pd3};
        double mine = 0;
#pragma unroll
        for (int f = 0; f < TM_REC_F; f++) mine = lane == f ? fld[f] : mine;
        if (lane < TM_REC_F) d.recf[(size_t)lane * d.cap + s] = mine;
    }
}
__global__ void __launch_bounds__(256) tm_search_kernel(DevCam cam, KfLevels L, TmDev d, int stage, unsigned coarse_range, int coarse_its) {
    tm_search_body(cam, L, d, stage, coarse_range, coarse_its, blockIdx.x);
}

// The tail of SearchForPoints (:883-909) and the measurement list of the pose loop that follows.  One workgroup.
//   stage 0: status of the coarse slots, nFound, mbDidCoarse, the coarse loop's measurements;
//   stage 1: status of the other slots, then vIterationSet's found entries in order (coarse, top level, fine).
struct TmMailbox {
    ptam_trackmap_result res;
    double depth3[3];
    unsigned long long seq;
    // ptam_track_frames_batch, a frame with a rotation estimator: the alignment and the pose predicted from it, written by the
    // frame's align workgroup (sbi.hip) — covered by the sequence word, which a later kernel of the same queue publishes
    ptam_sbi_alignment align;
    double pose_in[12];
    // ptam_track_frames_recover_batch, a recovering frame: the relocaliser's result, written by the frame's align workgroup likewise
    ptam_reloc_result reloc;
    // ptam_track_frames_report_batch: the head words of the frame's report, written by the fill at the chain's end (framereport.hip),
    // and the frame's sequence number behind them
    unsigned long long report_seq;
    int report_head[4];
};
// the last act of a gather pass: thread 0 books the per-level counts and the stage's outcome (coarse: mbDidCoarse and the
// fine range; fine: everything of the frame's result but the pose and the depth sums)
__device__ __forceinline__ void tm_gather_finish(const TmDev& d, TmCtl& c, int stage, unsigned coarse_min, TmMailbox* mbox, int total,
                                                 int (*lsum)[16], int n_kept) {
    const int tid = threadIdx.x;
    int tot[1] = {total};
    if (tid == 0) {
        const int n_reused = c.n_reused + n_kept;   // searched patches of the stages so far whose finder kept its template
        c.n_reused = n_reused;
        int f4[4], a4[4];
#pragma unroll
        for (int l = 0; l < 4; l++) {   // (unrolled: dynamically indexed local arrays are scratch memory)
            int tf = 0, ta = 0;
            for (int w = 0; w < 16; w++) {
                tf += lsum[l][w];
                ta += lsum[4 + l][w];
            }
            f4[l] = c.found[l] + tf;
            a4[l] = c.attempted[l] + ta;
            c.found[l] = f4[l];
            c.attempted[l] = a4[l];
        }
        if (stage == 0) {
            c.n_found_coarse = tot[0];
            c.did_coarse = c.do_coarse && (unsigned)tot[0] >= coarse_min;   // :550-551
            c.n_meas_coarse = c.did_coarse ? tot[0] : 0;
            c.fine_range = c.did_coarse ? 5 : 10;                           // :572
        } else {
            c.n_meas = tot[0];
            c.outlier_by_slot = 0;
            // everything of the frame's result but the pose and the depth sums (the fine pose loop publishes those, then
            // the sequence word)
            ptam_trackmap_result& r = mbox->res;
            r.templates_reused = n_reused;
            r.pad_ = 0;
            r.did_coarse = c.did_coarse;
#pragma unroll
            for (int l = 0; l < 4; l++) {
                r.n_pvs[l] = c.n_lvl[l];
                r.attempted[l] = a4[l];
                r.found[l] = f4[l];
            }
            r.n_coarse = c.nC;
            r.n_top = c.nH;
            r.n_fine = c.nF;
            r.n_meas = tot[0];
        }
    }
}

// One WAVE per 64 slots, as many workgroups as the capacity needs (a single 1024-thread workgroup spent 12-20 us copying
// ~250-byte records per slot through ONE CU).  The search kernel has left a packed status word per slot, so every wave
// counts the found slots in front of its own by itself (at most 1024 coalesced words) — no scan across workgroups, no
// barrier; workgroup 0 also counts everything and books the stage's outcome.
#define TM_GATHER_THREADS 64
__device__ __forceinline__ void tm_gather_body(const TmDev& d, int stage, int coarse_its, unsigned coarse_min, TmMailbox* mbox, int bx) {   // one wave
    __shared__ int lsum[8][16];
    TmCtl& c = *d.ctl;
    const int lane = threadIdx.x;
    const int g_end = stage == 0 ? c.nC : c.n_slots;            // slots compacted by this stage
    const int st_first = stage == 0 ? 0 : c.nC;                 // slots whose status this stage decided
    const int s0 = bx * TM_GATHER_THREADS;
    if (s0 >= g_end && bx != 0) return;
    // my slot: everything that does not depend on another load leaves at once
    const int s = s0 + lane;
    const bool valid = s < g_end;
    const int sc = valid ? s : 0;
    const int st = valid ? d.slot_stat[sc] : 0;
    const int id = g_end > 0 ? d.list[sc] : 0;
    const double2 v2 = d.slot_v2[sc];
    // (the point and its TrackerData state are requested as soon as the id is there, found or not: behind the `found` test
    //  they would be one more round trip at the end of the kernel)
    const int idc = g_end > 0 ? id : 0;
    const double w0 = d.pts[idc].world[0], w1 = d.pts[idc].world[1], w2 = d.pts[idc].world[2];
    const ptam_projection pj = d.pvs[idc].proj;
    // found slots in front of my workgroup's first (workgroup 0: also the totals and the per-level counts of this stage)
    const int upto = bx == 0 ? g_end : s0;
    int before = 0, total = 0, lf[4] = {0, 0, 0, 0}, la[4] = {0, 0, 0, 0}, nk = 0;
    // (eight status words per lane and round, requested together: one word per round was a round trip per 64 slots — twenty
    //  in a row for the last workgroup of a thousand-slot list)
    for (int jb = 0; jb < upto; jb += 8 * TM_GATHER_THREADS) {
        int wq[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = jb + u * TM_GATHER_THREADS + lane;
            wq[u] = j < upto ? d.slot_stat[j] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = jb + u * TM_GATHER_THREADS + lane, w = wq[u];
            total += w & 1;
            if (j < s0) before += w & 1;
            if (bx == 0 && j >= st_first && j < upto) {
                const int l = (w >> 2) & 3;
                nk += (w >> 4) & 1;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    lf[q] += (l == q) & (w & 1);
                    la[q] += (l == q) & ((w >> 1) & 1);
                }
            }
        }
    }
    before = wave_sum_i32(before);
    const int found = valid ? (st & 1) : 0;
    const int k = __builtin_amdgcn_readlane(before, 63) + wave_incl_scan_i32(found) - found;
    if (found) {
        ptam_pose_meas m;
        m.world[0] = w0, m.world[1] = w1, m.world[2] = w2;
        m.found[0] = v2.x;
        m.found[1] = v2.y;
        m.sqrt_inv_noise = 1.0 / (double)(1 << ((st >> 2) & 3));   // :889
        d.meas[k] = m;
        d.entry[k] = pj;
        d.midx[k] = id;
        d.mslot[k] = s;
    }
    if (bx != 0) return;
    total = wave_sum_i32(total);
    nk = wave_sum_i32(nk);
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const int tf = wave_sum_i32(lf[l]), ta = wave_sum_i32(la[l]);
        if (lane == 63) {
            lsum[l][0] = tf;
            lsum[4 + l][0] = ta;
#pragma unroll
            for (int w = 1; w < 16; w++) lsum[l][w] = lsum[4 + l][w] = 0;
        }
    }
    __syncthreads();
    tm_gather_finish(d, c, stage, coarse_min, mbox, __builtin_amdgcn_readlane(total, 63), lsum, __builtin_amdgcn_readlane(nk, 63));
}
__global__ void __launch_bounds__(TM_GATHER_THREADS) tm_gather_kernel(TmDev d, int stage, int coarse_its, unsigned coarse_min, TmMailbox* mbox) {
    tm_gather_body(d, stage, coarse_its, coarse_min, mbox, blockIdx.x);
}

// ---- SearchForPoints' bookkeeping + the pose loop in ONE launch (round 4) -----------------------------------------------
// The gather pass above exists to hand the pose kernel a compacted measurement list.  The register-resident pose loop does not
// need one: a slot without a measurement is a lane with weight zero.  So the loop's prologue takes its measurements straight
// from the search stage's slots — thread (q, tid) owns slot tid + q * THREADS — and books the stage's outcome itself: one
// launch (and its boundary) less per stage, 2 x (5.6 us kernel + 2.3 us boundary) per frame.  Lists of more slots than the
// kernel holds (a top-level set that outgrows MaxPatchesPerFrame) are told to the host, which sends the gather pass and the
// general pose kernel instead.
template <int MPT, int THREADS>
struct TmSlotLoader {
    const TmDev& d;
    int stage;
    unsigned coarse_min;
    TmMailbox* mbox;
    unsigned long long long_seq;   // what to publish when the list is too long (0: the host knows the capacity suffices)
    int id[MPT];
    int n_found;

    template <class SH>
    __device__ __forceinline__ bool begin(SH& sh, int& n, int cap, SmallMeas (&t)[MPT]) {
        const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
        // (A) every load that hangs on no other: the control block (uniform), and my slots' status word, point id and found
        //     position — fetched for the capacity, masked by the list's length afterwards: a load behind `slot < length` would
        //     wait for the control block first, and every dependent round trip of this single-workgroup kernel is ~1 us of frame
        const TmCtl c0 = *d.ctl;
        int st[MPT];
#pragma unroll
        for (int q = 0; q < MPT; q++) {
            // the slot's record: ONE round trip, nothing behind the point id, every load coalesced (field-major planes)
            const int sc = min(tid + q * THREADS, d.cap - 1);
            const int2 tg = d.rect[sc];
            st[q] = tg.x;
            id[q] = tg.y;
            const double* rf = d.recf + sc;
            const size_t pl = (size_t)d.cap;
            t[q].world[0] = rf[0], t[q].world[1] = rf[pl], t[q].world[2] = rf[2 * pl];
            t[q].fnd[0] = rf[3 * pl], t[q].fnd[1] = rf[4 * pl];
#pragma unroll
            for (int k = 0; k < 3; k++) t[q].cam3[k] = rf[(5 + k) * pl];
            t[q].img[0] = rf[8 * pl], t[q].img[1] = rf[9 * pl];
#pragma unroll
            for (int k = 0; k < 4; k++) t[q].D[k] = rf[(10 + k) * pl];
        }
        const int g_end = stage == 0 ? c0.nC : c0.n_slots;
        const int st_first = stage == 0 ? 0 : c0.nC;
        if (g_end > cap) {
            if (tid == 0 && long_seq) *(volatile unsigned long long*)&mbox->seq = long_seq | POSE_CHAIN_LONG;
            return false;
        }
        n = g_end;
        int p_tot = 0, p_f01 = 0, p_f23 = 0, p_a01 = 0, p_a23 = 0;
#pragma unroll
        for (int q = 0; q < MPT; q++) {
            const int s = tid + q * THREADS;
            const bool valid = s < g_end;
            st[q] = valid ? st[q] : 0;
            id[q] = valid ? id[q] : 0;
            // per-level counts of the slots this stage decided (found | attempted << 1 | level << 2 | kept << 4), two 16-bit
            // fields to a word: a list holds at most 1024 slots
            const int w = st[q], l = (w >> 2) & 3, mine = valid && s >= st_first;
            t[q].sn = 1.0 / (double)(1 << l);   // :889
            t[q].listed = w & 1;
            if (!(w & 1)) {   // (no measurement in this slot: benign values)
                t[q].world[0] = t[q].world[1] = t[q].world[2] = t[q].fnd[0] = t[q].fnd[1] = t[q].sn = 0;
                t[q].cam3[0] = t[q].cam3[1] = 0;
                t[q].cam3[2] = 1;
                t[q].img[0] = t[q].img[1] = 0;
                t[q].D[0] = t[q].D[1] = t[q].D[2] = t[q].D[3] = 0;
            }
            p_tot += (w & 1) | ((mine ? (w >> 4) & 1 : 0) << 16);
            const int f = mine ? (w & 1) : 0, a = mine ? (w >> 1) & 1 : 0;
            p_f01 += (l == 0 ? f : 0) | ((l == 1 ? f : 0) << 16);
            p_f23 += (l == 2 ? f : 0) | ((l == 3 ? f : 0) << 16);
            p_a01 += (l == 0 ? a : 0) | ((l == 1 ? a : 0) << 16);
            p_a23 += (l == 2 ? a : 0) | ((l == 3 ? a : 0) << 16);
        }
        p_tot = wave_sum_i32(p_tot);
        p_f01 = wave_sum_i32(p_f01);
        p_f23 = wave_sum_i32(p_f23);
        p_a01 = wave_sum_i32(p_a01);
        p_a23 = wave_sum_i32(p_a23);
        // (the pose loop's histogram is not in use yet: five words per wave meet there)
        if (lane == 63) {
            sh.hist[wid * 8 + 0] = (unsigned)p_tot;
            sh.hist[wid * 8 + 1] = (unsigned)p_f01;
            sh.hist[wid * 8 + 2] = (unsigned)p_f23;
            sh.hist[wid * 8 + 3] = (unsigned)p_a01;
            sh.hist[wid * 8 + 4] = (unsigned)p_a23;
        }
        __syncthreads();
        unsigned tt = 0, f01 = 0, f23 = 0, a01 = 0, a23 = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; w++) {
            tt += sh.hist[w * 8 + 0];
            f01 += sh.hist[w * 8 + 1];
            f23 += sh.hist[w * 8 + 2];
            a01 += sh.hist[w * 8 + 3];
            a23 += sh.hist[w * 8 + 4];
        }
        __syncthreads();   // (the words are read; the loop's own zeroing pass of the histogram follows)
        const int total = (int)(tt & 0xffffu), n_kept = (int)(tt >> 16);
        const int did = stage == 0 ? (c0.do_coarse && (unsigned)total >= coarse_min) : 1;
        if (tid == 0) {
            TmCtl& c = *d.ctl;
            const int lf[4] = {(int)(f01 & 0xffffu), (int)(f01 >> 16), (int)(f23 & 0xffffu), (int)(f23 >> 16)};
            const int la[4] = {(int)(a01 & 0xffffu), (int)(a01 >> 16), (int)(a23 & 0xffffu), (int)(a23 >> 16)};
            const int n_reused = c0.n_reused + n_kept;
            c.n_reused = n_reused;
            int f4[4], a4[4];
#pragma unroll
            for (int l = 0; l < 4; l++) {   // (unrolled: a dynamically indexed local array is scratch memory, and a kernel that
                                            //  needs scratch is dispatched later)
                f4[l] = c0.found[l] + lf[l];
                a4[l] = c0.attempted[l] + la[l];
                c.found[l] = f4[l];
                c.attempted[l] = a4[l];
            }
            if (stage == 0) {
                c.n_found_coarse = total;
                c.did_coarse = did;                                   // :550-551
                c.n_meas_coarse = did ? total : 0;
                c.fine_range = did ? 5 : 10;                          // :572
            } else {
                c.n_meas = total;
                c.outlier_by_slot = 1;
                // the frame's integer results: parked in LDS and written to the (host-mapped) result block at the kernel's end —
                // a store over PCIe issued here is waited for by this wave's next barrier (its release fence), i.e. by everybody
                int* bk = sh.book;   // ptam_trackmap_result from did_coarse on: did_coarse | n_pvs[4] | attempted[4] | found[4] | n_coarse n_top n_fine n_meas | depth_n | templates_reused | pad_
                bk[0] = c0.did_coarse;
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    bk[1 + l] = c0.n_lvl[l];
                    bk[5 + l] = a4[l];
                    bk[9 + l] = f4[l];
                }
                bk[13] = c0.nC;
                bk[14] = c0.nH;
                bk[15] = c0.nF;
                bk[16] = total;
                bk[17] = 0;
                bk[18] = n_reused;
                bk[19] = 0;
            }
        }
        n_found = did ? total : 0;
        if (!did) {   // the coarse stage found too little: no pose update (:550), nobody is listed
#pragma unroll
            for (int q = 0; q < MPT; q++) t[q].listed = 0;
        }
        return true;
    }
    __device__ __forceinline__ void load(int, int, int, SmallMeas&) const {}   // (begin has filled the slots)
    template <class SH>
    __device__ __forceinline__ void publish(SH& sh) const {
        static_assert(offsetof(ptam_trackmap_result, pad_) == offsetof(ptam_trackmap_result, did_coarse) + 19 * 4, "ptam_trackmap_result layout");
        if (stage == 1 && threadIdx.x < 20 && threadIdx.x != 17) (&mbox->res.did_coarse)[threadIdx.x] = sh.book[threadIdx.x];
    }
    __device__ __forceinline__ bool has_entry() const { return true; }
    __device__ __forceinline__ ptam_projection* td_target(int q, int, const PoseChainIo&) const { return &d.pvs[id[q]].proj; }
    // the slot's record follows the TrackerData the coarse loop leaves (the fine loop starts from it)
    __device__ __forceinline__ void td_also(int, int i, const SmallMeas& m) const {
        double* rf = d.recf + i;
        const size_t pl = (size_t)d.cap;
#pragma unroll
        for (int k = 0; k < 3; k++) rf[(5 + k) * pl] = m.cam3[k];
        rf[8 * pl] = m.img[0], rf[9 * pl] = m.img[1];
#pragma unroll
        for (int k = 0; k < 4; k++) rf[(10 + k) * pl] = m.D[k];
    }
    __device__ __forceinline__ int listed_total(int) const { return n_found; }
};

template <int MPT, int THREADS>
__device__ __forceinline__ void tm_pose_body(const DevCam& cam, const TmDev& d, int stage, unsigned coarse_min, TmMailbox* mbox,
                                             const ptam_gn_opts& opts, const PoseChainIo& io, double* updates, unsigned long long long_seq) {
    TmSlotLoader<MPT, THREADS> ld{d, stage, coarse_min, mbox, long_seq};
    // (no per-iteration record of the updates: nobody reads it in the chain, and a global store in front of a barrier is waited
    //  for by the barrier's release fence — ten times per loop, on the frame's critical path)
#if !defined(K7_TIMING) && !defined(TM_KEEP_UPDATES)   // (TM_KEEP_UPDATES: A/B builds)
    updates = nullptr;
#endif
    pose_gn_small_body<MPT, THREADS>(cam, THREADS * MPT, ld, d.pose, opts, stage == 1 ? d.outlier : nullptr, updates, nullptr, 0ull, nullptr, nullptr,
                                     io, 0);
}
template <int MPT, int THREADS>
__global__ void __launch_bounds__(THREADS) tm_pose_kernel(DevCam cam, TmDev d, int stage, unsigned coarse_min, TmMailbox* mbox, ptam_gn_opts opts,
                                                          PoseChainIo io, double* updates, unsigned long long long_seq) {
    tm_pose_body<MPT, THREADS>(cam, d, stage, coarse_min, mbox, opts, io, updates, long_seq);
}
typedef void (*tm_pose_fn)(DevCam, TmDev, int, unsigned, TmMailbox*, ptam_gn_opts, PoseChainIo, double*, unsigned long long);
// shape of the fused pose kernels for a list of at most cap slots (<= GS_LIMIT): 0 = one wave up to 64, 1 = one slot per thread up to
// GS_THREADS (512), 2 = GS_MPT (two) per thread up to GS_LIMIT (1024); the kernel tables below are in this order
static int tm_pose_shape(int cap, int* threads) {
    *threads = cap <= GS_WAVE_LIMIT ? GS_WAVE_LIMIT : GS_THREADS;
    return cap <= GS_WAVE_LIMIT ? 0 : cap <= GS_THREADS ? 1 : 2;
}
static const tm_pose_fn tm_pose_fns[3] = {tm_pose_kernel<1, GS_WAVE_LIMIT>, tm_pose_kernel<1, GS_THREADS>, tm_pose_kernel<GS_MPT, GS_THREADS>};

// =================================================================================================
// ---- a batch of frames in ONE chain of launches (ptam_track_map_frames_batch) ----
// A process gets four hardware queues, and a tracked frame occupies its queue for the whole dependent chain (two
// single-workgroup pose loops are 94 of its ~157 us): whatever the chip has idle, at most four frames of independent
// trackers are in flight (20 k frames/s, docs/LOG_r01_r04.md section 5).  A batch runs the SAME chain once for nb trackers: every
// launch gets a second grid dimension, workgroup row y works on frame y with that frame's arguments taken from a device
// array — the kernels' bodies are the single-frame ones.
struct TmBatchItem {
    PyrArgs pa;
    int n_pyr, n;          // pyramid workgroups (gx * gy), map points
    KfLevels L;
    TmDev d;
    PoseArg pv;            // use = 0: the pose is made on the device (ptam_track_frames_batch, a frame with a rotation estimator) —
                           // the PVS pass then runs behind the align workgroup, in tm_pvs_batch_kernel
    TmMailbox* mbox;
    // the frame's own bTryCoarse heuristics (src/Tracker.cc:503-514); ptam_track_map_frames_batch fills every frame with its one opts
    int try_coarse;
    unsigned coarse_max, coarse_range;
    // a recovering frame (ptam_track_frames_recover_batch; null otherwise): the relocaliser's verdict, written by the frame's align
    // workgroup in a launch in front of every kernel that reads it.  0: nothing of TrackMap happens — the kernels of the frame return
    // at their start, and the fine pose kernel only publishes the frame's sequence word
    const int* gate;
};
__device__ __forceinline__ bool tm_gated_off(const TmBatchItem& it) { return it.gate && !*it.gate; }
template <int VARIANT>
__global__ void __launch_bounds__(256) tm_pyr_pvs_batch_kernel(const TmBatchItem* __restrict__ items, int gx, DevCam cam) {
    const TmBatchItem& it = items[blockIdx.y];
    const int b = blockIdx.x;
    if (b < it.n_pyr)
        pyramid_body<VARIANT>(it.pa, (b % gx) * 64 + (threadIdx.x & 63), (b / gx) * 4 + (threadIdx.x >> 6));
    else if (it.pv.use && (b - it.n_pyr) * 256 < max(it.n, 1))
        track_pvs_body(cam, it.n, it.d.pts, it.d.pose, it.d.pvs, nullptr, it.pv, it.d.pose, b - it.n_pyr, &it.d.finder->bad, (int)sizeof(TmFinder));
}
// the PVS pass of the frames whose pose was made on the device: row y works on frame idx[y], the pose is read from the frame's d.pose
__global__ void __launch_bounds__(256) tm_pvs_batch_kernel(const TmBatchItem* __restrict__ items, const int* __restrict__ idx, DevCam cam) {
    const TmBatchItem& it = items[idx[blockIdx.y]];
    if (tm_gated_off(it)) return;
    if ((int)blockIdx.x * 256 < max(it.n, 1))
        track_pvs_body(cam, it.n, it.d.pts, it.d.pose, it.d.pvs, nullptr, it.pv, it.d.pose, blockIdx.x, &it.d.finder->bad, (int)sizeof(TmFinder));
}
__global__ void __launch_bounds__(1024) tm_compact_select_batch_kernel(const TmBatchItem* __restrict__ items, ptam_trackmap_opts o) {
    const TmBatchItem& it = items[blockIdx.y];
    if (blockIdx.x == 0) {
        if (tm_gated_off(it)) return;
        o.try_coarse = it.try_coarse;
        o.coarse_max = it.coarse_max;
        o.coarse_range = it.coarse_range;
        tm_select_body(it.d, o);
    } else
        fast_compact_body(it.L, blockIdx.x - 1, 0);
}
__global__ void __launch_bounds__(256) tm_search_batch_kernel(DevCam cam, const TmBatchItem* __restrict__ items, int stage, int coarse_its) {
    const TmBatchItem& it = items[blockIdx.y];
    if (tm_gated_off(it)) return;
    tm_search_body(cam, it.L, it.d, stage, it.coarse_range, coarse_its, blockIdx.x);
}
__global__ void __launch_bounds__(TM_GATHER_THREADS) tm_gather_batch_kernel(const TmBatchItem* __restrict__ items, int stage, int coarse_its,
                                                                            unsigned coarse_min) {
    const TmBatchItem& it = items[blockIdx.y];
    tm_gather_body(it.d, stage, coarse_its, coarse_min, it.mbox, blockIdx.x);
}
// the fused bookkeeping + pose loop (tm_pose_body) for the frames of a batch: one workgroup per frame; io and scratch of the frame's
// stage come from the pose items the unfused path uses.  idx (nullable): workgroup x works on frame idx[x] — the frames whose lists
// select this instantiation (ptam_track_frames_batch).  A fine list that outgrows the kernel is told to the host, as in the single frame.
template <int MPT, int THREADS>
__global__ void __launch_bounds__(THREADS) tm_pose_batch_kernel(DevCam cam, const TmBatchItem* __restrict__ items, const PoseBatchItem* __restrict__ pitems,
                                                                const int* __restrict__ idx, int stage, unsigned coarse_min, ptam_gn_opts opts) {
    const int f = idx ? idx[blockIdx.x] : (int)blockIdx.x;
    const TmBatchItem& it = items[f];
    const PoseBatchItem& pi = pitems[f];
    if (tm_gated_off(it)) {
        // (the relocaliser's result is in the frame's host-mapped block since the align launch, behind a system fence)
        if (stage == 1 && threadIdx.x == 0) {
            __threadfence_system();
            *(volatile unsigned long long*)pi.io.result_seq = pi.io.seq;
        }
        return;
    }
    tm_pose_body<MPT, THREADS>(cam, it.d, stage, coarse_min, it.mbox, opts, pi.io, pi.updates, stage == 1 && it.n > GS_LIMIT ? pi.io.seq : 0ull);
}
typedef void (*tm_pose_batch_fn)(DevCam, const TmBatchItem*, const PoseBatchItem*, const int*, int, unsigned, ptam_gn_opts);
static const tm_pose_batch_fn tm_pose_batch_fns[3] = {tm_pose_batch_kernel<1, GS_WAVE_LIMIT>, tm_pose_batch_kernel<1, GS_THREADS>,
                                                      tm_pose_batch_kernel<GS_MPT, GS_THREADS>};

struct ptam_tracker {
    ptam_ctx* ctx;
    TmDev d;
    void* block;
    TmMailbox* mbox;       // host-mapped
    TmMailbox* mbox_dev;
    unsigned long long seq;
    // the frame's two permutations in host-mapped memory (maps of at most TM_SEL_LDS = 8192 points: the set-choice kernel reads
    // every entry exactly once, at its start) — no upload, i.e. two copy kernels and their boundaries less per frame (~10 us);
    // d.perm_a / d.perm_b point either here or at the device arrays
    int* perm_host;        // [2][cap], host address
    int* perm_host_dev;    // device address of the same memory
    int *perm_dev_a, *perm_dev_b;
    unsigned long long* draw_keys;   // ptam_tracker_draw_shuffles' sort of a map of more than TR_DRAW_LDS_MAX points: [4][cap]; null for a smaller tracker
    // argument arrays of the batches this tracker leads (ptam_track_map_frames_batch): grown on demand
    void* batch_dev;
    size_t batch_cap;
    // the recovering cameras' SSD tables of the last batch this tracker led (inside batch_dev): rows x stride, row r holds reloc_count[r]
    const double* reloc_ssd;
    int reloc_stride;
    std::vector<int>* reloc_count;
    hipStream_t last_stream;   // the queue that last ran this tracker (its own context's, or a batch's lead tracker's)
    // ptam_tracker_take_map: the serials of the map's points (device, [cap]; valid iff has_serials), the map they belong to and
    // the (snapshot, generation) they were taken from.  ptam_tracker_set_map / update_map clear all of it.
    long long* serials;
    int has_serials;
    long long map_id, snap_uid, snap_generation;
    // stage timing of ptam_track_map_frame (ptam_tracker_set_profiling): an event after every launch of the frame
    bool prof;
    hipEvent_t ev[PTAM_TS_COUNT + 1];
    double stage_ms[PTAM_TS_COUNT];
    int stage_frames;
};

// ---- what the two ways of launching a frame share (track_map_impl passes the frame by value, ptam_track_map_frames_batch uploads
//      an array of frames) ----
// (A/B builds, `make ab`: the pyramid | FAST as two launches; the gather pass + pose kernel of rounds 2-3 instead of the fused one)
static const bool tm_kf_two = ptam_ab_env("PTAM_TM_KF_TWO_LAUNCHES") != nullptr;
static const bool tm_no_fuse = ptam_ab_env("PTAM_TM_NO_FUSE") != nullptr;
// (ptam_track_frames_batch: the FAST detection as a launch of its own in front of the images' make instead of inside the align launch)
static const bool tfb_plain = ptam_ab_env("PTAM_TFB_PLAIN") != nullptr;

// the instantiation of a kernel template for the context's halfSample variant
#define TM_HS_KERNEL(ctx, kernel) ((ctx)->halfsample == PTAM_HALFSAMPLE_T ? kernel<PTAM_HALFSAMPLE_T> : kernel<PTAM_HALFSAMPLE_R>)

// the caller's options, or the reference's, checked
static int tm_opts(const ptam_trackmap_opts* opts, ptam_trackmap_opts* o) {
    ptam_trackmap_opts_default(o);
    if (opts) *o = *opts;
    ARG_TRY(o->max_patches >= 0 && o->coarse_subpix_its >= 0 && o->coarse_subpix_its <= 64);
    // (coarse_max / coarse_min become ints on the device and size the coarse search grid: a value past INT_MAX / 2 turned the
    //  set sizes negative and the set choice wrote outside its lists; the range is a pixel radius inside a 640-pixel image)
    ARG_TRY(o->coarse_max <= (unsigned)INT_MAX / 2 && o->coarse_min <= (unsigned)INT_MAX / 2 && o->coarse_range <= 4096u);
    ARG_TRY(o->estimator == PTAM_EST_TUKEY || o->estimator == PTAM_EST_CAUCHY || o->estimator == PTAM_EST_HUBER);
    return PTAM_OK;
}
// the pose loop's schedule: stage 0 coarse (:554-568), stage 1 fine (:613-643)
static ptam_gn_opts tm_gn_opts(int stage, int estimator) {
    ptam_gn_opts g;
    ptam_gn_opts_default(&g);           // the fine schedule
    g.estimator = estimator;
    if (stage == 0) {
        g.nonlinear_mask = 0x3ff;       // every coarse iteration re-projects (:556-562)
        g.override_sigma_sq = 1.0;      // :565
        g.mark_outliers_iter = -1;      // CalcPoseUpdate(vIterationSet, dOverrideSigma): bMarkOutliers defaults to false
    }
    return g;
}
// what a tracker's pose loop leaves behind: the coarse one the TrackerData state of its measurements, the fine one the depth sums and
// — its last act — pose, depth sums and the sequence word in the mailbox
static PoseChainIo tm_chain_io(const ptam_tracker* t, int stage, unsigned long long seq) {
    const TmDev& d = t->d;
    PoseChainIo io{};
    if (stage == 0) {
        io.td_base = &d.pvs[0].proj;
        io.td_index = d.midx;
        io.td_stride = (int)sizeof(ptam_pvs_result);
    } else {
        io.depth_out = d.ctl->depth;
        io.result_pose = t->mbox_dev->res.pose;
        io.result_depth = t->mbox_dev->depth3;
        io.result_seq = &t->mbox_dev->seq;
        io.seq = seq;
    }
    return io;
}
// wait until the tracker's mailbox carries sequence number seq; *word (nullable): the word as read, POSE_CHAIN_LONG included
static int tm_wait_seq(const ptam_tracker* t, hipStream_t st, unsigned long long seq, const char* what, unsigned long long* word = nullptr) {
    unsigned long long v = 0;
    const int rc = ptam_wait_mapped(st, what, [&] { return ((v = *(volatile unsigned long long*)&t->mbox->seq) & ~POSE_CHAIN_LONG) == seq; });
    if (word) *word = v;
    return rc;
}
static void tm_read_result(const ptam_tracker* t, ptam_trackmap_result* out) {
    std::memcpy(out, (const void*)&t->mbox->res, sizeof *out);
    out->depth_sum = t->mbox->depth3[0];
    out->depth_sum_sq = t->mbox->depth3[1];
    out->depth_n = (int)t->mbox->depth3[2];
}

// Wait for frame `seq` of t, whose chain was enqueued on `st` (the tracker's own queue, or a batch's): the frame's last kernel
// publishes the sequence number — or, for a list of more than 1024 entries, asks for the general path, which the tracker's own queue
// then runs and which publishes it.  fused: the fine stage went out as the fused bookkeeping + pose kernel.
// *went_long (nullable) is set when the general path ran.
static int tm_wait_frame(ptam_tracker* t, hipStream_t st, const ptam_trackmap_opts& o, unsigned long long seq, bool fused, bool* went_long = nullptr) {
    ptam_ctx* ctx = t->ctx;
    const TmDev& d = t->d;
    const int n = d.n, n_fine = std::max(n, 1);
    const ptam_gn_opts g = tm_gn_opts(1, o.estimator);
    const PoseChainIo io = tm_chain_io(t, 1, seq);
    auto fine_chain = [&](int mode) { return pose_launch_chain(ctx, n_fine, &d.ctl->n_meas, d.meas, d.entry, d.pose, &g, d.outlier, io, mode); };
    for (int pass = 0; pass < 3; pass++) {
        unsigned long long v;
        int rc = tm_wait_seq(t, st, seq, "the frame's result", &v);
        if (rc) return rc;
        if (!(v & POSE_CHAIN_LONG)) break;
        if (went_long) *went_long = true;
        if (pass == 2) return PTAM_E_STATE;
        if (st != ctx->stream) {   // (a batch: the other frames' kernels still run there, and this frame goes on on its own queue)
            HIP_TRY(ptam_stream_wait(st));
            st = ctx->stream;
        } else if (went_long) {
            // (the report batch: the chain's fill kernel, queued behind the fine loop, reads this word to see that the frame is not
            //  finished — it must have run before the word is cleared)
            HIP_TRY(ptam_stream_wait(st));
        }
        t->mbox->seq = 0;   // (the stream is idle: nobody else writes the word until the next kernel does)
        if (fused) {
            // more slots than the fused kernel holds: compact them, then the register-resident kernel if the FOUND ones fit
            // (it says so otherwise: next pass)
            fused = false;
            hipLaunchKernelGGL(tm_gather_kernel, dim3(std::max(1, (n + TM_GATHER_THREADS - 1) / TM_GATHER_THREADS)), dim3(TM_GATHER_THREADS), 0, st, d, 1,
                               o.coarse_subpix_its, o.coarse_min, t->mbox_dev);
            rc = fine_chain(1);
        } else {
            rc = fine_chain(2);
        }
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
    }
    return PTAM_OK;
}

ptam_ctx* tracker_ctx(const ptam_tracker* t) { return t->ctx; }

extern "C" {

void ptam_trackmap_opts_default(ptam_trackmap_opts* o) {
    if (!o) return;
    o->try_coarse = 1;
    o->coarse_min = 20;          // Tracker.CoarseMin          src/Tracker.cc:492
    o->coarse_max = 60;          // Tracker.CoarseMax          :493
    o->coarse_range = 30;        // Tracker.CoarseRange        :494
    o->coarse_subpix_its = 8;    // Tracker.CoarseSubPixIts    :495
    o->max_patches = 1000;       // Tracker.MaxPatchesPerFrame :593
    o->estimator = PTAM_EST_TUKEY;
    o->pad_ = 0;
}

int ptam_tracker_create(ptam_ctx* ctx, int max_points, ptam_tracker** out) {
    ARG_TRY(ctx && out && max_points >= 1);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_tracker* t = new ptam_tracker();
    std::memset(t, 0, sizeof *t);
    t->ctx = ctx;
    const size_t cap = (size_t)max_points;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t o_pts = take(cap * sizeof(ptam_pvs_point)), o_src = take(cap * sizeof(TmSrc)), o_pa = take(cap * 4), o_pb = take(cap * 4),
                 o_pvs = take(cap * sizeof(ptam_pvs_result)), o_ll = take(cap * 16), o_fc = take(cap), o_list = take(cap * 4),
                 o_tr = take(cap * sizeof(ptam_template_result)),
                 o_q = take(cap * sizeof(ptam_patch_query)), o_r = take(cap * sizeof(ptam_patch_result)),
                 o_sr = take(cap * sizeof(ptam_subpix_result)), o_sf = take(cap * 4), o_st = take(cap * 4), o_ss = take(cap * 4), o_sv = take(cap * 16), o_rec = take(cap * TM_REC_F * 8), o_rect = take(cap * 8),
                 o_me = take(cap * sizeof(ptam_pose_meas)), o_en = take(cap * sizeof(ptam_projection)), o_mi = take(cap * 4),
                 o_ms = take(cap * 4), o_ou = take(cap * 4), o_ctl = take(sizeof(TmCtl)), o_pose = take(96),
                 o_fs = take(cap * sizeof(TmFinder)), o_ser = take(cap * sizeof(long long)),
                 o_dk = take(max_points > TR_DRAW_LDS_MAX ? cap * 32 : 0);
    // every failure past this point leaves through ONE path that releases what exists so far
    auto fail = [&](const char* what) {
        ptam_set_error("ptam_tracker_create: %s failed", what);
        if (t->perm_host) hipHostFree(t->perm_host);
        if (t->mbox) hipHostFree(t->mbox);
        if (t->block) hipFree(t->block);
        delete t;
        return PTAM_E_HIP;
    };
    if (hipMalloc(&t->block, off) != hipSuccess) return fail("hipMalloc");
    (void)hipMemsetAsync(t->block, 0, off, ctx->stream);
    char* b = (char*)t->block;
    TmDev& d = t->d;
    d.n = 0;
    d.cap = max_points;
    d.pts = (ptam_pvs_point*)(b + o_pts);
    d.src = (TmSrc*)(b + o_src);
    d.perm_a = (int*)(b + o_pa);
    d.perm_b = (int*)(b + o_pb);
    d.pvs = (ptam_pvs_result*)(b + o_pvs);
    d.lvl_list = (int*)(b + o_ll);
    d.isfc = (uint8_t*)(b + o_fc);
    d.list = (int*)(b + o_list);
    d.tres = (ptam_template_result*)(b + o_tr);
    d.q = (ptam_patch_query*)(b + o_q);
    d.r = (ptam_patch_result*)(b + o_r);
    d.sr = (ptam_subpix_result*)(b + o_sr);
    d.slot_found = (int*)(b + o_sf);
    d.slot_stat = (int*)(b + o_st);
    d.slot_subpix = (int*)(b + o_ss);
    d.slot_v2 = (double2*)(b + o_sv);
    d.recf = (double*)(b + o_rec);
    d.rect = (int2*)(b + o_rect);
    d.meas = (ptam_pose_meas*)(b + o_me);
    d.entry = (ptam_projection*)(b + o_en);
    d.midx = (int*)(b + o_mi);
    d.mslot = (int*)(b + o_ms);
    d.outlier = (int*)(b + o_ou);
    d.ctl = (TmCtl*)(b + o_ctl);
    d.pose = (double*)(b + o_pose);
    d.finder = (TmFinder*)(b + o_fs);   // (cleared with the block: no finder has made a template yet)
    t->serials = (long long*)(b + o_ser);
    t->draw_keys = max_points > TR_DRAW_LDS_MAX ? (unsigned long long*)(b + o_dk) : nullptr;
    void* h = nullptr;
    if (hipHostMalloc(&h, sizeof(TmMailbox), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail("hipHostMalloc");
    t->mbox = (TmMailbox*)h;
    std::memset(h, 0, sizeof(TmMailbox));
    void* dv = nullptr;
    if (hipHostGetDevicePointer(&dv, h, 0) != hipSuccess) return fail("hipHostGetDevicePointer");
    t->mbox_dev = (TmMailbox*)dv;
    t->perm_dev_a = d.perm_a;
    t->perm_dev_b = d.perm_b;
    {
        void *hp = nullptr, *dp = nullptr;
        if (hipHostMalloc(&hp, cap * 8, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail("hipHostMalloc");
        t->perm_host = (int*)hp;
        if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) return fail("hipHostGetDevicePointer");
        t->perm_host_dev = (int*)dp;
    }
    // identity shuffles until the caller sets its own
    std::vector<int> idp((size_t)max_points);
    for (int i = 0; i < max_points; i++) idp[(size_t)i] = i;
    if (hipMemcpy(d.perm_a, idp.data(), cap * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d.perm_b, idp.data(), cap * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail("hipMemcpy");
    if (ptam_stream_wait(ctx->stream) != hipSuccess) return fail("stream wait");
    *out = t;
    return PTAM_OK;
}

int ptam_tracker_destroy(ptam_tracker* t) {
    if (!t) return PTAM_OK;
    hipSetDevice(t->ctx->device);
    ptam_stream_wait(t->ctx->stream);
    if (t->block) hipFree(t->block);
    if (t->mbox) hipHostFree(t->mbox);
    if (t->perm_host) hipHostFree(t->perm_host);
    if (t->batch_dev) hipFree(t->batch_dev);
    delete t->reloc_count;
    if (t->ev[0])
        for (int i = 0; i <= PTAM_TS_COUNT; i++) hipEventDestroy(t->ev[i]);
    delete t;
    return PTAM_OK;
}

// new[i] = the finder of the point that was at prev[i] in the old map (a fresh one for prev[i] < 0 and past the new map's end)
__global__ void __launch_bounds__(256) tm_finder_carry_kernel(TmFinder* __restrict__ fresh, const TmFinder* __restrict__ old, const int* __restrict__ prev,
                                                              int n, int cap) {
    // (a finder is 112 bytes = 28 words: thread = (point, word))
    constexpr int W = (int)(sizeof(TmFinder) / 4);
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)cap * W) return;
    const int i = (int)(g / W), w = (int)(g % W);
    const int src = i < n ? prev[i] : -1;
    ((unsigned*)fresh)[g] = src >= 0 ? ((const unsigned*)old)[(long long)src * W + w] : 0u;
}
static_assert(sizeof(TmFinder) % 4 == 0, "TmFinder is copied word by word");

static int tracker_set_map_impl(ptam_tracker* t, int n, const ptam_pvs_point* pts, const ptam_template_query* src, const int32_t* prev_index) {
    ARG_TRY(t && n >= 0 && n <= t->d.cap && (n == 0 || (pts && src)));
    ptam_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if (prev_index) {   // every old point carries its finder to at most one new point
        std::vector<uint8_t> seen((size_t)std::max(t->d.n, 1), 0);
        for (int i = 0; i < n; i++) {
            ARG_TRY(prev_index[i] >= -1 && prev_index[i] < t->d.n);
            if (prev_index[i] >= 0) {
                ARG_TRY(!seen[(size_t)prev_index[i]]);
                seen[(size_t)prev_index[i]] = 1;
            }
        }
    }
    std::vector<TmSrc> s((size_t)n);
    for (int i = 0; i < n; i++) {
        const ptam_template_query& q = src[i];
        ARG_TRY(q.src_kf && q.src_level >= 0 && q.src_level < PTAM_LEVELS && q.src_kf->device == ctx->device);
        s[(size_t)i].im = q.src_kf->L.im[q.src_level];
        s[(size_t)i].w = q.src_kf->L.w[q.src_level];
        s[(size_t)i].h = q.src_kf->L.h[q.src_level];
        s[(size_t)i].cx = q.center_x;
        s[(size_t)i].cy = q.center_y;
    }
    HIP_TRY(ptam_stream_wait(ctx->stream));
    if (n > 0) {
        HIP_TRY(hipMemcpy(t->d.pts, pts, (size_t)n * sizeof(ptam_pvs_point), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t->d.src, s.data(), (size_t)n * sizeof(TmSrc), hipMemcpyHostToDevice));
    }
    if (prev_index && n > 0) {
        // the map changed, its points did not: a point that was in the old map keeps its TrackerData — the PatchFinder with its
        // template, warp matrix and mbTemplateBad (include/Tracker.h:42-67 lives as long as the MapPoint)
        const size_t bf = (size_t)t->d.cap * sizeof(TmFinder);
        const size_t bfa = (bf + 255) & ~(size_t)255;
        void* s_;
        const int rc = ctx_scratch(ctx, bfa + (size_t)n * 4 + 256, &s_);   // (the queue is idle: the scratch is nobody's)
        if (rc) return rc;
        int* d_prev = (int*)((char*)s_ + bfa);
        HIP_TRY(hipMemcpy(s_, t->d.finder, bf, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(d_prev, prev_index, (size_t)n * 4, hipMemcpyHostToDevice));
        const long long words = (long long)t->d.cap * (long long)(sizeof(TmFinder) / 4);
        hipLaunchKernelGGL(tm_finder_carry_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, t->d.finder, (const TmFinder*)s_,
                           (const int*)d_prev, n, t->d.cap);
        HIP_TRY(hipGetLastError());
        HIP_TRY(ptam_stream_wait(ctx->stream));
    } else {
        // a new map: new TrackerData, new PatchFinders (include/Tracker.h:42-67) — no template has been made, none is bad
        HIP_TRY(hipMemset(t->d.finder, 0, (size_t)t->d.cap * sizeof(TmFinder)));
    }
    if (n != t->d.n) {   // the shuffles are permutations of 0..n-1: back to the identity until the caller sets them again
        std::vector<int> idp((size_t)std::max(n, 1));
        for (int i = 0; i < n; i++) idp[(size_t)i] = i;
        t->d.perm_a = t->perm_dev_a;
        t->d.perm_b = t->perm_dev_b;
        if (n > 0) {
            HIP_TRY(hipMemcpy(t->d.perm_a, idp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(t->d.perm_b, idp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        }
    }
    t->d.n = n;
    t->has_serials = 0;   // the points have no identity any more: the next take treats every one as new
    t->map_id = t->snap_uid = t->snap_generation = 0;
    return PTAM_OK;
}

// ---- ptam_tracker_take_map: the map from a snapshot, device to device ----
// prev[i] = where new point i was in the tracker's map: its serial, searched in the old list (both strictly increasing, so no old
// index is found twice); n_old = 0 when the tracker has no list or the map is another one.  *n_carried counts the hits.
__global__ void __launch_bounds__(256) tm_take_prev_kernel(int n, const long long* __restrict__ fresh, int n_old, const long long* __restrict__ old,
                                                           int* __restrict__ prev, int* __restrict__ n_carried) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long key = fresh[i];
    int lo = 0, hi = n_old;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (old[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    const int at = lo < n_old && old[lo] == key ? lo : -1;
    prev[i] = at;
    if (at >= 0) atomicAdd(n_carried, 1);
}
// the shuffles back to the identity (the map's size changed: they are permutations of 0..n-1)
__global__ void __launch_bounds__(256) tm_identity_kernel(int n, int* __restrict__ a, int* __restrict__ b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = i, b[i] = i;
}
// the serial of every entry of the iteration set (list: search slot -> map point)
__global__ void __launch_bounds__(256) tm_iteration_serials_kernel(int ns, const int* __restrict__ list, int n, const long long* __restrict__ serials,
                                                                   long long* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ns) return;
    const int p = list[s];
    out[s] = p >= 0 && p < n ? serials[p] : -1;
}

// the device side of a take, from slot `sl` (held by the caller): everything enqueued on the context's queue, one wait
static int tracker_take_enqueue(ptam_tracker* t, const SnapSlot& sl, int* n_carried) {
    ptam_ctx* ctx = t->ctx;
    hipStream_t st = ctx->stream;
    const int n = sl.n, cap = t->d.cap;
    HIP_TRY(ptam_stream_wait(st));   // (as ptam_tracker_update_map: no frame of this tracker is in flight, the scratch is nobody's)
    if (t->last_stream && t->last_stream != st) HIP_TRY(ptam_stream_wait(t->last_stream));
    const size_t bf = (size_t)cap * sizeof(TmFinder), bfa = (bf + 255) & ~(size_t)255, bpa = ((size_t)n * 4 + 255) & ~(size_t)255;
    void *sc, *hp;
    if (int rc = ctx_scratch(ctx, bfa + bpa + 256, &sc)) return rc;
    if (int rc = ctx_pinned(ctx, 256, &hp)) return rc;
    int* d_prev = (int*)((char*)sc + bfa);
    int* d_count = (int*)((char*)sc + bfa + bpa);
    HIP_TRY(hipMemsetAsync(d_count, 0, 8, st));
    HIP_TRY(hipMemcpyAsync(sc, t->d.finder, bf, hipMemcpyDeviceToDevice, st));
    const int n_old = t->has_serials && t->map_id == sl.map_id ? t->d.n : 0;
    if (n > 0)
        hipLaunchKernelGGL(tm_take_prev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const long long*)sl.serials, n_old,
                           (const long long*)t->serials, d_prev, d_count);
    const long long words = (long long)cap * (long long)(sizeof(TmFinder) / 4);
    hipLaunchKernelGGL(tm_finder_carry_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, t->d.finder, (const TmFinder*)sc,
                       (const int*)d_prev, n, cap);
    HIP_TRY(hipGetLastError());
    if (n > 0) {   // (behind the search: the old serial list has been read)
        HIP_TRY(hipMemcpyAsync(t->d.pts, sl.pts, (size_t)n * sizeof(ptam_pvs_point), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->d.src, sl.src, (size_t)n * sizeof(TmSrc), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(t->serials, sl.serials, (size_t)n * sizeof(long long), hipMemcpyDeviceToDevice, st));
    }
    if (n != t->d.n) {   // the ≤ 8192-point path keeps the frame's shuffles in host-mapped memory: back to the device arrays
        t->d.perm_a = t->perm_dev_a;
        t->d.perm_b = t->perm_dev_b;
        if (n > 0) {
            hipLaunchKernelGGL(tm_identity_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, t->d.perm_a, t->d.perm_b);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipMemcpyAsync(hp, d_count, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    *n_carried = *(const int*)hp;
    return PTAM_OK;
}

int ptam_tracker_take_map(ptam_tracker* t, ptam_map_snapshot* snap, ptam_map_take_result* res) {
    ARG_TRY(t && snap && res);
    ptam_ctx* ctx = t->ctx;
    ARG_TRY(snap->device == ctx->device);
    ARG_TRY(snap->width == ctx->params.width && snap->height == ctx->params.height);
    ptam_map_take_result r = {};
    long long gen = 0;
    const int k = snap->slots.begin_read(t->snap_uid == snap->uid ? t->snap_generation : -1, &gen);
    if (k == SnapSlots::NEVER) {
        ptam_set_error("bad argument: ptam_tracker_take_map: nothing has been published into the snapshot");
        return PTAM_E_ARG;
    }
    if (k == SnapSlots::UNCHANGED) {   // the per-frame poll
        r.generation = gen;
        r.map_id = t->map_id;
        r.n_points = t->d.n;
        *res = r;
        return PTAM_OK;
    }
    const SnapSlot& sl = snap->slot[k];   // ours until end_read: the publisher leaves it alone
    if (sl.n > t->d.cap) {
        const int n = sl.n;
        snap->slots.end_read(k);
        ptam_set_error("bad argument: ptam_tracker_take_map: the snapshot holds %d points, the tracker %d at most", n, t->d.cap);
        return PTAM_E_ARG;
    }
    int rc = hipSetDevice(ctx->device) == hipSuccess ? PTAM_OK : PTAM_E_HIP;
    int carried = 0;
    if (!rc) rc = tracker_take_enqueue(t, sl, &carried);
    const int n = sl.n, n_old = t->d.n;
    const long long map_id = sl.map_id, generation = sl.generation;
    snap->slots.end_read(k);
    if (rc) return rc;
    t->d.n = n;
    t->has_serials = 1;
    t->map_id = map_id;
    t->snap_uid = snap->uid;
    t->snap_generation = generation;
    r.changed = 1;
    r.n_points = n;
    r.n_carried = carried;
    r.n_new = n - carried;
    r.n_dropped = n_old - carried;
    r.link_bytes = 8;
    r.generation = generation;
    r.map_id = map_id;
    *res = r;
    return PTAM_OK;
}

int ptam_tracker_point_serials(ptam_tracker* t, int first, int count, int64_t* out) {
    ARG_TRY(t && first >= 0 && count >= 0 && (long long)first + count <= (t->has_serials ? t->d.n : 0));
    ARG_TRY(count == 0 || out);
    if (count == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(t->ctx->device));
    HIP_TRY(hipMemcpyAsync(out, t->serials + first, (size_t)count * sizeof(long long), hipMemcpyDeviceToHost, t->ctx->stream));
    HIP_TRY(ptam_stream_wait(t->ctx->stream));
    return PTAM_OK;
}

int ptam_tracker_read_iteration_serials(ptam_tracker* t, int64_t* out, int cap, int* n_out) {
    ARG_TRY(t && n_out && cap >= 0);
    if (!t->has_serials) {
        ptam_set_error("ptam_tracker_read_iteration_serials: the tracker's map did not come from a snapshot");
        return PTAM_E_STATE;
    }
    ptam_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    TmCtl c;
    HIP_TRY(hipMemcpy(&c, t->d.ctl, sizeof c, hipMemcpyDeviceToHost));
    const int ns = std::min(std::max(c.n_slots, 0), t->d.cap);
    *n_out = ns;
    const int take = std::min(ns, cap);
    if (!out || take == 0) return PTAM_OK;
    void* sc;
    if (int rc = ctx_scratch(ctx, (size_t)take * sizeof(long long), &sc)) return rc;
    hipLaunchKernelGGL(tm_iteration_serials_kernel, dim3((unsigned)((take + 255) / 256)), dim3(256), 0, ctx->stream, take, (const int*)t->d.list, t->d.n,
                       (const long long*)t->serials, (long long*)sc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, sc, (size_t)take * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

// The frames the trackers tracked last into the reports: where each tracker's iteration set lies goes up as a job table, one launch
// of the report core fills all of them, one wait brings the counts down (framereport.hip)
int ptam_tracker_report_frames(int nb, ptam_tracker* const* trackers, ptam_frame_report* const* reports, const int64_t* tags) {
    // ---- refusals: nothing is enqueued, and no report is touched, before all of them have passed
    ARG_TRY(nb >= 1 && nb <= 4096 && trackers && reports);
    for (int i = 0; i < nb; i++) {
        ARG_TRY(trackers[i] && reports[i]);
        ARG_TRY(reports[i]->ctx->device == trackers[i]->ctx->device && trackers[i]->ctx->device == trackers[0]->ctx->device);
        for (int j = 0; j < i; j++) ARG_TRY(reports[j] != reports[i] && trackers[j] != trackers[i]);
    }
    for (int i = 0; i < nb; i++)
        if (!trackers[i]->has_serials) {
            ptam_set_error("ptam_tracker_report_frames: the map of tracker %d did not come from a snapshot", i);
            return PTAM_E_STATE;
        }
    ptam_tracker* lead = trackers[0];
    ptam_ctx* ctx = lead->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = lead->last_stream ? lead->last_stream : ctx->stream;
    // (every frame has been delivered: these find their queues idle)
    if (st != ctx->stream) HIP_TRY(ptam_stream_wait(ctx->stream));
    for (int i = 1; i < nb; i++) {
        hipStream_t si = trackers[i]->last_stream ? trackers[i]->last_stream : trackers[i]->ctx->stream;
        if (si != st) HIP_TRY(ptam_stream_wait(si));
    }
    for (int i = 0; i < nb; i++)
        if (int rc = fr_mark_room(reports[i], trackers[i]->d.n)) return rc;
    const size_t b_jobs = ((size_t)nb * sizeof(FrJob) + 255) & ~(size_t)255, b_heads = (size_t)nb * FR_HEAD_WORDS * sizeof(int);
    void *sc, *hp;
    if (int rc = ctx_scratch(ctx, b_jobs + b_heads, &sc)) return rc;
    if (int rc = ctx_pinned(ctx, b_heads, &hp)) return rc;
    std::vector<FrJob> jobs((size_t)nb);
    for (int i = 0; i < nb; i++) {
        const TmDev& d = trackers[i]->d;
        FrJob& j = jobs[(size_t)i];
        j = FrJob{};
        j.n_points = d.n;
        j.serials = trackers[i]->serials;
        j.cap = d.cap;
        j.n_slots = &d.ctl->n_slots;
        j.n_meas = &d.ctl->n_meas;
        j.outlier_by_slot = &d.ctl->outlier_by_slot;
        j.list = d.list;
        j.slot_found = d.slot_found;
        j.slot_subpix = d.slot_subpix;
        j.q = d.q;
        j.tres = d.tres;
        j.slot_v2 = d.slot_v2;
        j.outlier = d.outlier;
        j.mslot = d.mslot;
        j.mark = reports[i]->mark;
        j.rec = reports[i]->rec;
        j.max_records = reports[i]->max_records;
    }
    int* d_heads = (int*)((char*)sc + b_jobs);
    HIP_TRY(hipMemcpyAsync(sc, jobs.data(), (size_t)nb * sizeof(FrJob), hipMemcpyHostToDevice, st));
    if (int rc = fr_fill_core(st, nb, (const FrJob*)sc, d_heads)) return rc;
    HIP_TRY(hipMemcpyAsync(hp, d_heads, b_heads, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));   // the call's one wait: every report is whole
    const int* h = (const int*)hp;
    int too_small = -1;
    for (int i = 0; i < nb; i++, h += FR_HEAD_WORDS) {
        ptam_frame_report_info_t& info = reports[i]->info;
        info = ptam_frame_report_info_t{};
        if (h[FR_H_RECORDS] > reports[i]->max_records) {
            if (too_small < 0) {
                too_small = i;
                ptam_set_error("bad argument: ptam_tracker_report_frames: frame %d found %d points, its report holds %d records", i, h[FR_H_RECORDS],
                               reports[i]->max_records);
            }
            continue;
        }
        info.map_id = trackers[i]->map_id;
        info.tag = tags ? tags[i] : 0;
        info.n_records = h[FR_H_RECORDS];
        info.n_entries = h[FR_H_ENTRIES];
        info.n_outliers = h[FR_H_OUTLIERS];
    }
    return too_small < 0 ? PTAM_OK : PTAM_E_ARG;
}

int ptam_tracker_set_map(ptam_tracker* t, int n, const ptam_pvs_point* pts, const ptam_template_query* src) {
    return tracker_set_map_impl(t, n, pts, src, nullptr);
}
int ptam_tracker_update_map(ptam_tracker* t, int n, const ptam_pvs_point* pts, const ptam_template_query* src, const int32_t* prev_index) {
    ARG_TRY(prev_index || n == 0);
    return tracker_set_map_impl(t, n, pts, src, prev_index);
}

int ptam_tracker_set_shuffle(ptam_tracker* t, const int32_t* shuffle_levels, const int32_t* shuffle_fine) {
    ARG_TRY(t && shuffle_levels && shuffle_fine);
    const int n = t->d.n;
    if (n == 0) return PTAM_OK;
    // permutations of 0..n-1 (anything else would index outside the map on the device)
    std::vector<uint8_t> seen((size_t)n);
    for (int pass = 0; pass < 2; pass++) {
        const int32_t* p = pass ? shuffle_fine : shuffle_levels;
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < n; i++) {
            ARG_TRY(p[i] >= 0 && p[i] < n && !seen[(size_t)p[i]]);
            seen[(size_t)p[i]] = 1;
        }
    }
    HIP_TRY(hipSetDevice(t->ctx->device));
    if (n <= TM_SEL_LDS) {
        // host-mapped: the kernel of the coming frame reads the entries straight from here.  The previous frame's set choice
        // is certainly done once that frame's result has arrived; otherwise wait for the queue.
        // (a batch runs the tracker on the LEAD tracker's queue: that is the one to wait for)
        if (t->mbox->seq != t->seq) HIP_TRY(ptam_stream_wait(t->last_stream ? t->last_stream : t->ctx->stream));
        std::memcpy(t->perm_host, shuffle_levels, (size_t)n * 4);
        std::memcpy(t->perm_host + t->d.cap, shuffle_fine, (size_t)n * 4);
        t->d.perm_a = t->perm_host_dev;
        t->d.perm_b = t->perm_host_dev + t->d.cap;
        return PTAM_OK;
    }
    t->d.perm_a = t->perm_dev_a;
    t->d.perm_b = t->perm_dev_b;
    void* pin;
    int rc = ctx_pinned(t->ctx, (size_t)n * 8 + 64, &pin);
    if (rc) return rc;
    HIP_TRY(ptam_stream_wait(t->ctx->stream));   // (shared staging buffer; the previous frame has been read by now anyway)
    if (t->last_stream && t->last_stream != t->ctx->stream) HIP_TRY(ptam_stream_wait(t->last_stream));
    std::memcpy(pin, shuffle_levels, (size_t)n * 4);
    std::memcpy((char*)pin + (size_t)n * 4, shuffle_fine, (size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(t->d.perm_a, pin, (size_t)n * 4, hipMemcpyHostToDevice, t->ctx->stream));
    HIP_TRY(hipMemcpyAsync(t->d.perm_b, (char*)pin + (size_t)n * 4, (size_t)n * 4, hipMemcpyHostToDevice, t->ctx->stream));
    return PTAM_OK;
}

int ptam_tracker_draw_shuffles(ptam_tracker* t, uint64_t seed, uint64_t frame) {
    ARG_TRY(t);
    const int n = t->d.n;
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(t->ctx->device));
    // The draw runs on the tracker's own queue, where its next frame runs too (a batch joins the queues of its trackers first).  Only a
    // frame that another tracker's queue still holds could read the arrays while they are written: every entry that tracks returns
    // behind the frame's result, so this does not happen unless a caller broke that order
    if (t->last_stream && t->last_stream != t->ctx->stream && t->mbox->seq != t->seq) HIP_TRY(ptam_stream_wait(t->last_stream));
    t->d.perm_a = t->perm_dev_a;
    t->d.perm_b = t->perm_dev_b;
    return tr_draw_shuffles_on(t->ctx->stream, n, seed, frame, t->d.perm_a, t->d.perm_b, t->draw_keys);
}

int ptam_tracker_read_shuffle(ptam_tracker* t, int32_t* shuffle_levels, int32_t* shuffle_fine) {
    ARG_TRY(t && shuffle_levels && shuffle_fine);
    const int n = t->d.n;
    if (n == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(t->ctx->device));
    // (wherever the orders live: the device arrays, or the host-mapped copy of ptam_tracker_set_shuffle)
    HIP_TRY(hipMemcpyAsync(shuffle_levels, t->d.perm_a, (size_t)n * 4, hipMemcpyDefault, t->ctx->stream));
    HIP_TRY(hipMemcpyAsync(shuffle_fine, t->d.perm_b, (size_t)n * 4, hipMemcpyDefault, t->ctx->stream));
    HIP_TRY(ptam_stream_wait(t->ctx->stream));
    return PTAM_OK;
}

// d_new_frame (nullable): the current keyframe is made first — KeyFrame::MakeKeyFrame_Lite of this device-resident image, in
// the same queue.  (Measured and dropped: the keyframe kernels on a second queue beside the PVS pass and the set choice, which
// do not look at the image — the two cross-queue event waits cost more than the 13 us of overlap: 207-218 vs 193-200 us.)
// The frame's arguments ride in the launches: nothing is uploaded.
static int track_map_impl(ptam_tracker* t, ptam_kf* cur, const uint8_t* d_new_frame, const double pose_in[12],
                          const ptam_trackmap_opts* opts, ptam_trackmap_result* out) {
    ARG_TRY(t && cur && pose_in && out);
    ptam_ctx* ctx = t->ctx;
    ARG_TRY(cur->device == ctx->device);
    ptam_trackmap_opts o;
    int rc = tm_opts(opts, &o);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const TmDev& d = t->d;
    const int n = d.n, n_fine = std::max(n, 1);
    hipStream_t st = ctx->stream;
    const bool prof = t->prof && d_new_frame;
    auto mark = [&](int stage) {   // stage timing (ptam_tracker_set_profiling): the launches that follow belong to `stage`
        if (prof) hipEventRecord(t->ev[stage], st);
    };
    auto gather = [&](int cap, int stage) {
        hipLaunchKernelGGL(tm_gather_kernel, dim3(std::max(1, (cap + TM_GATHER_THREADS - 1) / TM_GATHER_THREADS)), dim3(TM_GATHER_THREADS), 0, st, d, stage,
                           o.coarse_subpix_its, o.coarse_min, t->mbox_dev);
    };
    // ---- keyframe + PVS + set choice ----
    mark(PTAM_TS_PYR_PVS);
    if (d_new_frame) {
        // KeyFrame::MakeKeyFrame_Lite (src/KeyFrame.cc:18-54) of the new image, the PVS pass (:453-478, the pose rides in as an
        // argument) and the set choice (:480-611) in three launches
        PyrArgs pa;
        int gx, gy;
        kf_lite_begin(cur, d_new_frame, &pa, &gx, &gy);
        PoseArg pv{};
        std::memcpy(pv.v, pose_in, 96);
        pv.use = 1;
        const int n_pyr = gx * gy, n_pvs = std::max(1, (n + 255) / 256);
        if (!tm_kf_two) {
            const int n_tiles = cur->n_blocks;
            hipLaunchKernelGGL(TM_HS_KERNEL(ctx, tm_kf_pvs_kernel), dim3(n_tiles + n_pvs), dim3(256), 0, st, pa, cur->L, n_tiles, ctx->cam, std::max(n, 0),
                               (const ptam_pvs_point*)d.pts, d.pvs, pv, d.pose, &d.finder->bad);
            mark(PTAM_TS_DETECT);
        } else {
            hipLaunchKernelGGL(TM_HS_KERNEL(ctx, tm_pyr_pvs_kernel), dim3(n_pyr + n_pvs), dim3(256), 0, st, pa, gx, n_pyr, ctx->cam, std::max(n, 0),
                               (const ptam_pvs_point*)d.pts, d.pvs, pv, d.pose, &d.finder->bad);
            mark(PTAM_TS_DETECT);
            kf_launch_detect(cur, st);
        }
        mark(PTAM_TS_COMPACT_SELECT);
        hipLaunchKernelGGL(tm_compact_select_kernel, dim3(1 + fast_compact_blocks(cur->L)), dim3(1024), 0, st, cur->L, d, o);
    } else {
        rc = pvs_launch_dev(ctx, n, d.pts, d.pose, pose_in, d.pvs, &d.finder->bad, (int)sizeof(TmFinder));   // :453-478 (the pose rides in as an argument)
        if (rc) return rc;
        hipLaunchKernelGGL(tm_select_kernel, dim3(1), dim3(1024), 0, st, d, o);   // :480-611
    }
    // ---- coarse stage :519-569 ----
    const int ncc = std::max(1, std::min(n, (int)o.coarse_max));
    mark(PTAM_TS_SEARCH_COARSE);
    hipLaunchKernelGGL(tm_search_kernel, dim3((ncc + 3) / 4), dim3(256), 0, st, ctx->cam, cur->L, d, 0, o.coarse_range, o.coarse_subpix_its);
    mark(PTAM_TS_GATHER_COARSE);
    void* d_st;
    double* d_upd;
    rc = pose_chain_scratch(ctx, n_fine, &d_st, &d_upd);
    if (rc) return rc;
    int thr;
    ptam_gn_opts g = tm_gn_opts(0, o.estimator);
    PoseChainIo io = tm_chain_io(t, 0, 0);
    if (ncc <= GS_LIMIT && !tm_no_fuse) {
        // SearchForPoints' bookkeeping and the ten coarse iterations in one launch (the coarse set holds at most CoarseMax slots)
        mark(PTAM_TS_POSE_COARSE);
        const tm_pose_fn fn = tm_pose_fns[tm_pose_shape(ncc, &thr)];
        hipLaunchKernelGGL(fn, dim3(1), dim3(thr), 0, st, ctx->cam, d, 0, o.coarse_min, t->mbox_dev, g, io, d_upd, 0ull);
    } else {
        gather(ncc, 0);
        mark(PTAM_TS_POSE_COARSE);
        rc = pose_launch_chain(ctx, ncc, &d.ctl->n_meas_coarse, d.meas, d.entry, d.pose, &g, nullptr, io);
        if (rc) return rc;
    }
    // ---- fine stage :571-643 ----
    mark(PTAM_TS_SEARCH_FINE);
    hipLaunchKernelGGL(tm_search_kernel, dim3(std::max(1, (n + 3) / 4)), dim3(256), 0, st, ctx->cam, cur->L, d, 1, 0u, 0);
    mark(PTAM_TS_GATHER_FINE);
    const unsigned long long seq = ++t->seq;
    t->last_stream = st;
    g = tm_gn_opts(1, o.estimator);
    io = tm_chain_io(t, 1, seq);
    auto fine_chain = [&](int mode) { return pose_launch_chain(ctx, n_fine, &d.ctl->n_meas, d.meas, d.entry, d.pose, &g, d.outlier, io, mode); };
    const bool fused = !tm_no_fuse;
    if (fused) {
        // bookkeeping + the ten fine iterations in one launch.  The iteration set holds at most max(MaxPatchesPerFrame, coarse
        // + top-level set) slots: with more than the kernel's 1024 it says so instead (POSE_CHAIN_LONG) and the gather pass
        // and the general kernel follow
        mark(PTAM_TS_POSE_FINE);
        const tm_pose_fn fn = tm_pose_fns[tm_pose_shape(std::min(n_fine, GS_LIMIT), &thr)];
        hipLaunchKernelGGL(fn, dim3(1), dim3(thr), 0, st, ctx->cam, d, 1, o.coarse_min, t->mbox_dev, g, io, d_upd, n > GS_LIMIT ? seq : 0ull);
    } else {
        gather(n, 1);
        mark(PTAM_TS_POSE_FINE);
        rc = fine_chain(1);
        if (rc) return rc;
    }
    mark(PTAM_TS_COUNT);
    HIP_TRY(hipGetLastError());
    rc = tm_wait_frame(t, st, o, seq, fused);
    if (rc) return rc;
    // ---- result ----
    tm_read_result(t, out);
    if (prof) {
        HIP_TRY(hipEventSynchronize(t->ev[PTAM_TS_COUNT]));
        for (int i = 0; i < PTAM_TS_COUNT; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
            t->stage_ms[i] += ms;
        }
        t->stage_frames++;
    }
    return PTAM_OK;
}

// Stage timing of ptam_track_map_frame (ptam_hip_bench.h): with profiling on, an event is recorded after every launch of the
// frame; the nine differences are added up per stage.  The events lengthen the frame (about 1 us per record): profiled frames
// are for the breakdown, not for the frame rate.
int ptam_tracker_set_profiling(ptam_tracker* t, int on) {
    ARG_TRY(t);
    HIP_TRY(hipSetDevice(t->ctx->device));
    if (on && !t->ev[0])
        for (int i = 0; i <= PTAM_TS_COUNT; i++) HIP_TRY(hipEventCreate(&t->ev[i]));
    t->prof = on != 0;
    for (int i = 0; i < PTAM_TS_COUNT; i++) t->stage_ms[i] = 0;
    t->stage_frames = 0;
    return PTAM_OK;
}
int ptam_tracker_stage_time(const ptam_tracker* t, int stage, double* total_ms, int* frames) {
    ARG_TRY(t && stage >= 0 && stage < PTAM_TS_COUNT && total_ms && frames);
    *total_ms = t->stage_ms[stage];
    *frames = t->stage_frames;
    return PTAM_OK;
}

int ptam_track_map(ptam_tracker* t, const ptam_kf* cur, const double pose_in[12], const ptam_trackmap_opts* opts,
                   ptam_trackmap_result* out) {
    return track_map_impl(t, const_cast<ptam_kf*>(cur), nullptr, pose_in, opts, out);
}

int ptam_track_map_frame(ptam_tracker* t, ptam_kf* cur, const uint8_t* d_frame, const double pose_in[12],
                         const ptam_trackmap_opts* opts, ptam_trackmap_result* out) {
    ARG_TRY(d_frame);
    return track_map_impl(t, cur, d_frame, pose_in, opts, out);
}

// =================================================================================================
// ---- the batch chain's host side: what ptam_track_map_frames_batch, ptam_track_frames_batch and ptam_track_frames_recover_batch
//      are made of.  Each of them reads check -> argument block -> fill -> upload -> keyframe / PVS / set choice -> two stages -> collect ----

// What every batch call refuses before it looks further (no HIP call).  All trackers must live on one device and share camera model,
// image geometry and halfSample variant; no tracker, keyframe or context comes twice.
static int tm_batch_check(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames) {
    ARG_TRY(nb >= 1 && nb <= 4096 && ts && curs && d_frames);
    for (int i = 0; i < nb; i++) ARG_TRY(ts[i] && curs[i] && d_frames[i]);
    const ptam_ctx* ctx = ts[0]->ctx;
    const KfLevels& L0 = curs[0]->L;
    for (int i = 0; i < nb; i++) {
        ARG_TRY(ts[i]->ctx->device == ctx->device && curs[i]->device == ctx->device);
        ARG_TRY(ts[i]->ctx->halfsample == ctx->halfsample && std::memcmp(&ts[i]->ctx->cam, &ctx->cam, sizeof(DevCam)) == 0);
        ARG_TRY(curs[i]->n_blocks == curs[0]->n_blocks);
        for (int l = 0; l < PTAM_LEVELS; l++) ARG_TRY(curs[i]->L.w[l] == L0.w[l] && curs[i]->L.h[l] == L0.h[l]);
        for (int j = 0; j < i; j++) ARG_TRY(ts[j] != ts[i] && curs[j] != curs[i] && ts[j]->ctx != ts[i]->ctx);   // (a context's scratch serves ONE frame)
    }
    return PTAM_OK;
}

// The chain runs on the first tracker's queue: whatever the other trackers' own queues still hold (a map upload, the tail of their
// last frame) must be done.
static int tm_batch_join(int nb, ptam_tracker* const* ts) {
    ptam_ctx* ctx = ts[0]->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    for (int i = 1; i < nb; i++)
        if (ts[i]->ctx != ctx) HIP_TRY(ptam_stream_wait(ts[i]->ctx->stream));
    return PTAM_OK;
}

// The argument block of a batch: a pinned copy the host fills and the device copy in the lead tracker's batch_dev, section by
// section at the same offsets, every section 256-byte aligned:
//   nb TmBatchItem | nb PoseBatchItem (coarse) | nb (fine) | n_est + n_rr SbiBatchRec | 3 x nb frame indices | n_rr SbiRelocRec
//   | n_rep FrChainJob | n_draw TrDrawJob          (ptam_track_frames_report_batch: the reports' fill and the shuffles' draw)
// and behind what is uploaded, on the device only, the recovering cameras' SSD tables (n_rr x rr_max_count) and gates.
// The frame indices: [frames whose pose is made on the device | coarse stage by instantiation | fine stage by instantiation],
// idx_stride ints apart.  ptam_track_map_frames_batch has n_est = n_rr = 0 and uploads the first three sections.
extern "C++" {   // (member templates, inside this file's extern "C")
struct TmBatchArgs {
    enum Section { ITEMS, POSE_COARSE, POSE_FINE, SBI_REC, FRAME_IDX, RELOC_REC, REPORT_JOB, DRAW_JOB, RELOC_SSD, RELOC_GATE, N_SECTIONS };
    enum { LAST_UPLOADED = DRAW_JOB };
    size_t off[N_SECTIONS + 1];
    size_t idx_stride;
    char* hb = nullptr;
    char* db = nullptr;

    TmBatchArgs(int nb, int n_est, int n_rr, int rr_max_count, int n_rep = 0, int n_draw = 0) {
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t b_idx = up((size_t)nb * 4);
        const size_t n = (size_t)nb, rr = (size_t)n_rr;
        const size_t bytes[N_SECTIONS] = {n * sizeof(TmBatchItem), n * sizeof(PoseBatchItem), n * sizeof(PoseBatchItem),
                                          (size_t)std::max(n_est + n_rr, 1) * sizeof(SbiBatchRec), 3 * b_idx, rr * sizeof(SbiRelocRec),
                                          (size_t)n_rep * sizeof(FrChainJob), (size_t)n_draw * sizeof(TrDrawJob),
                                          rr * (size_t)rr_max_count * 8, rr * 4};
        idx_stride = b_idx / 4;
        off[0] = 0;
        for (int s = 0; s < N_SECTIONS; s++) off[s + 1] = off[s] + up(bytes[s]);
    }
    size_t end(Section s) const { return off[s + 1]; }   // bytes up to and including section s
    template <class T> T* host(Section s) const { return (T*)(hb + off[s]); }
    template <class T> T* dev(Section s) const { return (T*)(db + off[s]); }
    int* host_idx(int list) const { return host<int>(FRAME_IDX) + (size_t)list * idx_stride; }
    const int* dev_idx(int list) const { return dev<int>(FRAME_IDX) + (size_t)list * idx_stride; }

    // the pinned copy from the lead tracker's context, and its batch_dev grown on demand
    int reserve(ptam_tracker* lead) {
        void* pin;
        const int rc = ctx_pinned(lead->ctx, end((Section)LAST_UPLOADED) + 64, &pin);
        if (rc) return rc;
        if (lead->batch_cap < end(RELOC_GATE)) {
            HIP_TRY(ptam_stream_wait(lead->ctx->stream));
            if (lead->batch_dev) HIP_TRY(hipFree(lead->batch_dev));
            lead->batch_dev = nullptr;
            lead->batch_cap = 0;
            HIP_TRY(hipMalloc(&lead->batch_dev, end(RELOC_GATE) * 2));
            lead->batch_cap = end(RELOC_GATE) * 2;
        }
        hb = (char*)pin;
        db = (char*)lead->batch_dev;
        return PTAM_OK;
    }
};
}

// what the launches of a batch are shaped by
struct TmBatchDims {
    int gx = 0, gy = 0;              // a frame's pyramid workgroups (one geometry: tm_batch_check)
    int n_max = 0, ncc_max = 1;      // the longest fine and the longest coarse list
    int n_shape[2][3], first[2][3];  // tm_group_by_shape
};

// one frame's pose loop of a batch: what pose_launch_chain takes as arguments (updates, st: the frame's own context's scratch)
static PoseBatchItem tm_pose_item(const ptam_tracker* t, int stage, int n_cap, double* updates, void* st, unsigned long long seq) {
    const TmDev& d = t->d;
    PoseBatchItem p;
    std::memset(&p, 0, sizeof p);
    p.n_cap = n_cap;
    p.n_dev = stage ? &d.ctl->n_meas : &d.ctl->n_meas_coarse;
    p.meas = d.meas;
    p.entry = d.entry;
    p.pose_io = d.pose;
    p.flags = stage ? d.outlier : nullptr;
    p.updates = updates;
    p.st = st;
    p.io = tm_chain_io(t, stage, seq);
    return p;
}

// Frame i of the block: the tracker's TmBatchItem and its two PoseBatchItem.  pose (nullable): the pose the host predicted; without
// it the device makes the pose and the frame's PVS pass runs in tm_pvs_batch_kernel.  f: the frame's own options (the bTryCoarse
// heuristics applied).  The fine loop publishes the tracker's NEXT sequence number; tm_commit_seqs makes it the tracker's own.
static int tm_fill_frame(const TmBatchArgs& a, int i, ptam_tracker* t, ptam_kf* cur, const uint8_t* d_frame, const double* pose,
                         const ptam_trackmap_opts& f, TmBatchDims* dm) {
    TmBatchItem& it = a.host<TmBatchItem>(TmBatchArgs::ITEMS)[i];
    std::memset(&it, 0, sizeof it);
    kf_lite_begin(cur, d_frame, &it.pa, &dm->gx, &dm->gy);
    it.n_pyr = dm->gx * dm->gy;
    it.n = t->d.n;
    it.L = cur->L;
    it.d = t->d;
    it.mbox = t->mbox_dev;
    it.try_coarse = f.try_coarse, it.coarse_max = f.coarse_max, it.coarse_range = f.coarse_range;
    if (pose) {
        std::memcpy(it.pv.v, pose, 96);
        it.pv.use = 1;
    }
    const int n = t->d.n, n_fine = std::max(n, 1), ncc = std::max(1, std::min(n, (int)f.coarse_max));
    dm->n_max = std::max(dm->n_max, n);
    dm->ncc_max = std::max(dm->ncc_max, ncc);
    void* sst;
    double* su;
    const int rc = pose_chain_scratch(t->ctx, n_fine, &sst, &su);   // (sized for the fine loop; the coarse one uses its start)
    if (rc) return rc;
    a.host<PoseBatchItem>(TmBatchArgs::POSE_COARSE)[i] = tm_pose_item(t, 0, ncc, su, sst, 0);
    a.host<PoseBatchItem>(TmBatchArgs::POSE_FINE)[i] = tm_pose_item(t, 1, n_fine, su, sst, t->seq + 1);
    return PTAM_OK;
}
// behind the last point where the call can refuse: the frames' sequence numbers become the trackers'
static void tm_commit_seqs(int nb, ptam_tracker* const* ts, hipStream_t st) {
    for (int i = 0; i < nb; i++) {
        ts[i]->seq++;
        ts[i]->last_stream = st;
    }
}

// The pose loops of a stage go out in one of three forms:
//   GROUPED     every frame in the fused kernel instantiation its OWN list length selects, the frames of one instantiation in one
//               launch with an index list — a frame's result is the single call's bit for bit (ptam_track_frames_batch)
//   ONE_LAUNCH  one fused launch shaped by the batch's longest list, no index list (ptam_track_map_frames_batch)
//   GATHER      the gather pass and the small / general kernel pair of pose_launch_chain_batch for everybody: results equal the single
//               calls' to rounding
// The fused kernels hold GS_LIMIT (1024) slots.  GROUPED needs every COARSE list to fit (a fine list that outgrows the kernel is
// finished on the frame's own queue after the wait, tm_wait_frame); ONE_LAUNCH needs every list of both stages to fit.
enum TmPoseForm { TM_POSE_GROUPED, TM_POSE_ONE_LAUNCH, TM_POSE_GATHER };
static TmPoseForm tm_pose_form(bool per_frame, int n_max, int ncc_max) {
    if (tm_no_fuse || ncc_max > GS_LIMIT) return TM_POSE_GATHER;
    if (per_frame) return TM_POSE_GROUPED;
    return n_max <= GS_LIMIT ? TM_POSE_ONE_LAUNCH : TM_POSE_GATHER;
}
// GROUPED: index lists 1 (coarse) and 2 (fine) of the block — the frames of every pose-kernel instantiation, n_shape[stage][k] frames
// from first[stage][k] on
static void tm_group_by_shape(const TmBatchArgs& a, int nb, TmBatchDims* dm) {
    int thr;
    for (int sg = 0; sg < 2; sg++) {
        const PoseBatchItem* p = a.host<PoseBatchItem>(sg ? TmBatchArgs::POSE_FINE : TmBatchArgs::POSE_COARSE);
        int* list = a.host_idx(1 + sg);
        int at = 0;
        for (int k = 0; k < 3; k++) {
            dm->first[sg][k] = at;
            for (int i = 0; i < nb; i++)
                if (tm_pose_shape(std::min(p[i].n_cap, GS_LIMIT), &thr) == k) list[at++] = i;
            dm->n_shape[sg][k] = at - dm->first[sg][k];
        }
    }
}
// stage sg of the chain (0 coarse :519-569, 1 fine :571-643): the search, then the pose loops
static int tm_enqueue_stage(ptam_ctx* ctx, int nb, const TmBatchArgs& a, const TmBatchDims& dm, const ptam_trackmap_opts& o, int sg,
                            TmPoseForm form) {
    hipStream_t st = ctx->stream;
    const TmBatchItem* d_it = a.dev<TmBatchItem>(TmBatchArgs::ITEMS);
    const PoseBatchItem* d_p = a.dev<PoseBatchItem>(sg ? TmBatchArgs::POSE_FINE : TmBatchArgs::POSE_COARSE);
    const int cap = sg ? std::max(dm.n_max, 1) : dm.ncc_max;
    hipLaunchKernelGGL(tm_search_batch_kernel, dim3(std::max(1, (cap + 3) / 4), nb), dim3(256), 0, st, ctx->cam, d_it, sg, sg ? 0 : (int)o.coarse_subpix_its);
    const ptam_gn_opts g = tm_gn_opts(sg, o.estimator);
    int thr;
    switch (form) {
    case TM_POSE_GROUPED:
        for (int k = 0; k < 3; k++) {
            if (dm.n_shape[sg][k] == 0) continue;
            hipLaunchKernelGGL(tm_pose_batch_fns[k], dim3(dm.n_shape[sg][k]), dim3(k == 0 ? GS_WAVE_LIMIT : GS_THREADS), 0, st, ctx->cam, d_it, d_p,
                               a.dev_idx(1 + sg) + dm.first[sg][k], sg, o.coarse_min, g);
        }
        return PTAM_OK;
    case TM_POSE_ONE_LAUNCH: {
        const tm_pose_batch_fn fn = tm_pose_batch_fns[tm_pose_shape(cap, &thr)];
        hipLaunchKernelGGL(fn, dim3(nb), dim3(thr), 0, st, ctx->cam, d_it, d_p, (const int*)nullptr, sg, o.coarse_min, g);
        return PTAM_OK;
    }
    default: {
        const int longest = sg ? dm.n_max : dm.ncc_max;
        hipLaunchKernelGGL(tm_gather_batch_kernel, dim3(std::max(1, (longest + TM_GATHER_THREADS - 1) / TM_GATHER_THREADS), nb), dim3(TM_GATHER_THREADS), 0, st,
                           d_it, sg, (int)o.coarse_subpix_its, o.coarse_min);
        return pose_launch_chain_batch(ctx, nb, cap, d_p, &g);
    }
    }
}

// Wait + result, frame by frame.  long_path: a frame whose fine list outgrew the fused kernel says so in its sequence word
// (POSE_CHAIN_LONG) and is finished on its own queue (tm_wait_frame; fused: the fine stage went out GROUPED); a batch that never sets
// the bit waits for the word alone.
// went_long (nullable): nb flags, set for the frames that were finished on their own queue.
static int tm_collect(int nb, ptam_tracker* const* ts, hipStream_t st, const ptam_trackmap_opts& o, bool long_path, bool fused,
                      ptam_trackmap_result* outs, bool* went_long = nullptr) {
    for (int i = 0; i < nb; i++) {
        const int rc = long_path ? tm_wait_frame(ts[i], st, o, ts[i]->seq, fused, went_long ? went_long + i : nullptr)
                                 : tm_wait_seq(ts[i], st, ts[i]->seq, "a frame's result");
        if (rc) {
            const std::string e = ptam_last_error();
            ptam_set_error("frame %d of the batch: %s", i, e.c_str());
            return rc;
        }
        tm_read_result(ts[i], outs + i);
    }
    return PTAM_OK;
}

// nb frames of nb independent trackers — each with its own map, keyframe and motion-model prediction — as ONE chain of
// launches on the first tracker's queue (see TmBatchItem).  Per frame the result is what ptam_track_map_frame gives (the same
// kernel bodies on the same data); opts apply to every frame.  No frame of this batch asks for the general path after the wait:
// with a map of more than 1024 points the stages go out in the GATHER form.
int ptam_track_map_frames_batch(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, const double* poses_in,
                                const ptam_trackmap_opts* opts, ptam_trackmap_result* outs) {
    ARG_TRY(poses_in && outs);
    int rc = tm_batch_check(nb, ts, curs, d_frames);
    ptam_trackmap_opts o;
    if (!rc) rc = tm_opts(opts, &o);
    if (rc) return rc;
    ptam_tracker* lead = ts[0];
    ptam_ctx* ctx = lead->ctx;
    hipStream_t st = ctx->stream;
    if (lead->reloc_count) lead->reloc_count->clear();   // (the argument block is rewritten: ptam_tracker_read_reloc_ssd has no rows)
    TmBatchArgs a(nb, 0, 0, 0);
    TmBatchDims dm;
    rc = tm_batch_join(nb, ts);
    if (!rc) rc = a.reserve(lead);
    for (int i = 0; i < nb && !rc; i++) rc = tm_fill_frame(a, i, ts[i], curs[i], d_frames[i], poses_in + 12 * (size_t)i, o, &dm);
    if (rc) return rc;
    tm_commit_seqs(nb, ts, st);
    HIP_TRY(hipMemcpyAsync(lead->batch_dev, a.hb, a.end(TmBatchArgs::POSE_FINE), hipMemcpyHostToDevice, st));
    // ---- keyframe + PVS + set choice ----
    const TmBatchItem* d_it = a.dev<TmBatchItem>(TmBatchArgs::ITEMS);
    const int n_pyr = dm.gx * dm.gy, n_pvs = std::max(1, (dm.n_max + 255) / 256);
    hipLaunchKernelGGL(TM_HS_KERNEL(ctx, tm_pyr_pvs_batch_kernel), dim3(n_pyr + n_pvs, nb), dim3(256), 0, st, d_it, dm.gx, ctx->cam);
    kf_launch_detect_batch(nb, curs[0]->L, d_it, sizeof(TmBatchItem), offsetof(TmBatchItem, L), st);
    hipLaunchKernelGGL(tm_compact_select_batch_kernel, dim3(1 + fast_compact_blocks(curs[0]->L), nb), dim3(1024), 0, st, d_it, o);
    // ---- the two stages, the wait ----
    const TmPoseForm form = tm_pose_form(false, dm.n_max, dm.ncc_max);
    for (int sg = 0; sg < 2 && !rc; sg++) rc = tm_enqueue_stage(ctx, nb, a, dm, o, sg, form);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return tm_collect(nb, ts, st, o, false, false, outs);
}


// ---- Tracker::TrackFrame's tracking branch (src/Tracker.cc:94-108, :134-137, :1013-1056) for nb cameras in ONE chain ----
// ptam_track_map_frames_batch with what ptam_track_frame / ptam_track_frame_sbi put around TrackMap: the bTryCoarse heuristics per
// camera (each frame's TmBatchItem carries its own), the motion model, and — for a frame with a rotation estimator — this frame's
// SmallBlurryImage, its alignment against last frame's and the prediction from the rotation, all on the device.  In three steps
// that share a TfbPlan: tfb_plan (host only), tfb_enqueue (the chain), tfb_finish (models, estimators, infos).
// rv (nullable): ptam_track_frames_recover_batch's recovering cameras — rv->recovering[i] != 0: frame i runs the relocaliser in the
// chain instead of a prediction, and TrackMap behind it only where the relocaliser's verdict is good (TmBatchItem::gate).  The caller
// has checked their banks and scratches.  Without rv, or with no camera recovering, nothing differs from the plain batch.
struct TfbRecover {
    const char* recovering;           // [nb]
    ptam_sbi_bank* const* banks;      // [nb]
    ptam_sbi* const* scratch;         // [nb]
    double blur, max_score;
    ptam_reloc_result* reloc;         // out: the recovering frames' results, frame i's reloc_stride bytes behind frame i - 1's
    size_t reloc_stride;
};
// rp (nullable): ptam_track_frames_report_batch's extras — the frames' reports filled at the chain's end, the shuffles drawn at its
// start.  The caller has checked the reports and made room for their marks.  Without rp nothing differs.
struct TfbReport {
    ptam_frame_report* const* reports;   // [nb], entries nullable
    const int64_t* tags;                 // nullable
    const uint64_t* seeds;               // nullable: no draw
    const int64_t* frames;               // [nb]: the draw's frame index
    ptam_track_report_info* infos;       // out, nullable
    int too_small;                       // out: the first camera whose report was too small for its frame, or -1
    bool enqueued;                       // out: the chain went out (the reports' records are being rewritten)
};
struct TfbPlan {
    int nb;
    ptam_rotation_estimator* const* ests;   // nullable, and so is every entry
    const TfbRecover* rv;
    ptam_trackmap_opts o;                   // the caller's, checked
    std::vector<ptam_trackmap_opts> fo;     // per frame: o with the frame's heuristics
    std::vector<ptam_motion_model> tmp;     // the models, advanced on copies (committed by tfb_finish)
    std::vector<int> est_of;                // the frames that have an estimator, those of recovering frames last
    std::vector<int> rr_of;                 // the recovering frames
    int n_est, n_rr, n_est_align, rr_max_count;
    bool est(int i) const { return ests && ests[i]; }
    bool recovering(int i) const { return rv && rv->recovering[i]; }
};

// Everything that needs no device: the options, the estimators' order and checks, the recovering list, the heuristics and the
// prediction.  ts / curs / d_frames have passed tm_batch_check.
static int tfb_plan(int nb, ptam_tracker* const* ts, const ptam_motion_model* models, ptam_rotation_estimator* const* ests,
                    const ptam_trackmap_opts* opts, const TfbRecover* rv, TfbPlan* p) {
    p->nb = nb, p->ests = ests, p->rv = rv;
    int rc = tm_opts(opts, &p->o);
    if (rc) return rc;
    // the estimators: each its tracker's context's, none twice, all of one image size and blur (their images are made in one launch)
    // (those of recovering frames last: their images are made with the others', but nothing is aligned, src/Tracker.cc:94-108 + :168-176)
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; ests && i < nb; i++) {
            if (!ests[i] || (int)p->recovering(i) != pass) continue;
            ARG_TRY(sbi_estimator_ctx(ests[i]) == ts[i]->ctx);
            for (int j : p->est_of) ARG_TRY(ests[j] != ests[i]);
            if (!p->est_of.empty()) ARG_TRY(sbi_estimators_alike(ests[p->est_of[0]], ests[i]));
            p->est_of.push_back(i);
        }
    for (int i = 0; i < nb; i++)
        if (p->recovering(i)) p->rr_of.push_back(i);
    p->n_est = (int)p->est_of.size(), p->n_rr = (int)p->rr_of.size();
    p->n_est_align = p->rr_max_count = 0;
    for (int i : p->est_of) p->n_est_align += !p->recovering(i);
    if (ts[0]->reloc_count) ts[0]->reloc_count->clear();
    for (int i : p->rr_of) {
        int c;
        sbi_bank_camera_positions(rv->banks[i], &c);
        p->rr_max_count = std::max(p->rr_max_count, c);
        if (p->est(i)) ARG_TRY(sbi_estimator_fits_bank(ests[i], rv->banks[i]));
    }
    // the heuristics, per frame, as ptam_track_frame has them; a recovering frame follows AttemptRecovery, which sets
    // mbJustRecoveredSoUseCoarse with TrackMap at once behind it (:171-173, :205, :508-513)
    p->tmp.assign(models, models + nb);
    p->fo.assign((size_t)nb, p->o);
    for (int i = 0; i < nb; i++) {
        ptam_motion_model& m = p->tmp[(size_t)i];
        if (track_coarse_heuristics(&p->fo[(size_t)i], &m, p->recovering(i))) {
            ptam_trackmap_opts checked;
            rc = tm_opts(&p->fo[(size_t)i], &checked);   // (the doubled values, as TrackMap checks them in the single call)
            if (rc) return rc;
        }
        if (p->recovering(i)) continue;   // (no prediction: the relocaliser's pose is the start; the model moves after the wait, if at all)
        if (p->est(i)) std::memcpy(m.start_pose, m.pose, 96);   // (the device makes the pose: ptam_motion_predict_sbi's first line)
        else ptam_motion_predict(&m);
    }
    return PTAM_OK;
}

// The block's records, host only: the frames, the estimators' records, the recovering frames' make and relocaliser records, the
// index lists.  *n_dev_pose: the frames whose pose is made on the device (index list 0: the aligned ones, then the recovering).
static int tfb_fill(const TfbPlan& p, const TmBatchArgs& a, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames,
                    TmBatchDims* dm, int* n_dev_pose) {
    int rc;
    for (int i = 0; i < p.nb; i++) {
        const bool host_pose = !p.est(i) && !p.recovering(i);
        rc = tm_fill_frame(a, i, ts[i], curs[i], d_frames[i], host_pose ? p.tmp[(size_t)i].pose : nullptr, p.fo[(size_t)i], dm);
        if (rc) return rc;
    }
    if (p.n_rr > 0 && tm_pose_form(true, dm->n_max, dm->ncc_max) != TM_POSE_GROUPED) {
        ptam_set_error("a recovering camera in a batch whose coarse lists exceed the fused pose kernels' %d entries", GS_LIMIT);
        return PTAM_E_ARG;
    }
    SbiBatchRec* h_rec = a.host<SbiBatchRec>(TmBatchArgs::SBI_REC);
    for (int k = 0; k < p.n_est; k++) {
        const int i = p.est_of[(size_t)k];
        SbiBatchRec& r = h_rec[k];
        std::memset(&r, 0, sizeof r);
        rc = sbi_batch_rec(p.ests[i], curs[i], &r);
        if (rc) return rc;
        std::memcpy(r.velocity, p.tmp[(size_t)i].velocity, sizeof r.velocity);
        std::memcpy(r.start_pose, p.tmp[(size_t)i].start_pose, sizeof r.start_pose);
        r.pose_out = ts[i]->d.pose;
        r.h_align = &ts[i]->mbox_dev->align;
        r.h_pose_in = ts[i]->mbox_dev->pose_in;
    }
    // the recovering frames: a make record behind the estimators', and the relocaliser's record; their SSD rows stay readable
    // through the lead tracker (ptam_tracker_read_reloc_ssd)
    ptam_tracker* lead = ts[0];
    double* d_ssd = a.dev<double>(TmBatchArgs::RELOC_SSD);
    int* d_gate = a.dev<int>(TmBatchArgs::RELOC_GATE);
    if (p.n_rr > 0) {
        if (!lead->reloc_count) lead->reloc_count = new std::vector<int>();
        lead->reloc_ssd = d_ssd;
        lead->reloc_stride = p.rr_max_count;
    }
    for (int k = 0; k < p.n_rr; k++) {
        const int i = p.rr_of[(size_t)k];
        SbiBatchRec& mk = h_rec[p.n_est + k];
        SbiRelocRec& r = a.host<SbiRelocRec>(TmBatchArgs::RELOC_REC)[k];
        std::memset(&mk, 0, sizeof mk);
        std::memset(&r, 0, sizeof r);
        sbi_reloc_rec(p.rv->banks[i], p.rv->scratch[i], curs[i], &mk, &r);
        r.ssd = d_ssd + (size_t)k * (size_t)p.rr_max_count;
        r.max_score = p.rv->max_score;
        r.pose_out = ts[i]->d.pose;
        r.h_reloc = &ts[i]->mbox_dev->reloc;
        r.gate = d_gate + k;
        a.host<TmBatchItem>(TmBatchArgs::ITEMS)[i].gate = d_gate + k;
        lead->reloc_count->push_back(r.count);
    }
    int* h_idx = a.host_idx(0);
    *n_dev_pose = 0;
    for (int k = 0; k < p.n_est_align; k++) h_idx[(*n_dev_pose)++] = p.est_of[(size_t)k];
    for (int i : p.rr_of) h_idx[(*n_dev_pose)++] = i;
    tm_group_by_shape(a, p.nb, dm);
    return PTAM_OK;
}

// The estimators' and the relocaliser's launches between the pyramid and the set choice (docs/LOG_sbi.md has the arrangements that
// were measured):   SBI make  ->  align + predict | FAST detect  ->  PVS of the frames whose pose the device made
// The detection shares the align launch: its workgroups fill the chip under the align workgroups' ~100 us of serial chain, and a
// launch boundary goes — 6-9 % per frame up to 64 cameras, 2-4 % slower at 128.
static int tfb_enqueue_sbi(const TfbPlan& p, ptam_ctx* ctx, const TmBatchArgs& a, const KfLevels& L0, int n_pvs, int n_dev_pose) {
    hipStream_t st = ctx->stream;
    const int nb = p.nb, n_est = p.n_est, n_rr = p.n_rr;
    const TmBatchItem* d_it = a.dev<TmBatchItem>(TmBatchArgs::ITEMS);
    const SbiBatchRec* d_rec = a.dev<SbiBatchRec>(TmBatchArgs::SBI_REC);
    const SbiRelocRec* d_rrec = a.dev<SbiRelocRec>(TmBatchArgs::RELOC_REC);
    const bool share = !tfb_plain && n_est + n_rr > 0;
    if (!share) kf_launch_detect_batch(nb, L0, d_it, sizeof(TmBatchItem), offsetof(TmBatchItem, L), st);
    if (n_est + n_rr == 0) return PTAM_OK;
    ptam_rotation_estimator* est0 = n_est ? p.ests[p.est_of[0]] : nullptr;
    int rc = n_est > 0 ? sbi_batch_launch_make(est0, n_est, d_rec, st) : PTAM_OK;
    if (n_rr > 0) {
        // a recovering camera in the batch: the relocaliser's images (a make launch of their own: the weights are a launch argument and
        // the blur is not the estimators'), every recovering camera's SSDs in one launch, and their align workgroups between the
        // estimators' and the detection's
        const ptam_sbi_bank* bank0 = p.rv->banks[p.rr_of[0]];
        if (!rc) rc = sbi_reloc_launch_make(ctx, bank0, p.rv->blur, n_rr, d_rec + n_est, st);
        if (!rc) rc = sbi_reloc_launch_ssd(bank0, n_rr, p.rr_max_count, d_rrec, st);
        if (!rc)
            rc = sbi_recover_launch_align(ctx, bank0, p.n_est_align, d_rec, n_rr, d_rrec, st, share ? nb : 0, &L0, d_it, sizeof(TmBatchItem),
                                          offsetof(TmBatchItem, L));
    } else if (!rc && share) {
        rc = sbi_batch_launch_align(est0, n_est, d_rec, st, nb, &L0, d_it, sizeof(TmBatchItem), offsetof(TmBatchItem, L));
    } else if (!rc) {
        rc = sbi_batch_launch_align(est0, n_est, d_rec, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(tm_pvs_batch_kernel, dim3(n_pvs, n_dev_pose), dim3(256), 0, st, d_it, a.dev_idx(0), ctx->cam);
    return PTAM_OK;
}

// The chain:   pyramid | PVS of the frames the host predicted  ->  tfb_enqueue_sbi  ->  set choice | corner compaction
//   ->  search, pose (coarse)  ->  search, pose (fine)
// *form: how the stages went out (tm_collect wants to know).  A non-zero return leaves the estimators stepped: the caller rolls back.
// The report of frame i of the chain: where ptam_tracker_report_frames says the iteration set lies, where the fill's head words go
static FrChainJob tfb_report_job(ptam_tracker* t, const ptam_frame_report* r, const int* d_gate) {
    const TmDev& d = t->d;
    FrChainJob c = {};
    FrJob& j = c.job;
    j.n_points = d.n;
    j.serials = t->serials;
    j.cap = d.cap;
    j.n_slots = &d.ctl->n_slots;
    j.n_meas = &d.ctl->n_meas;
    j.outlier_by_slot = &d.ctl->outlier_by_slot;
    j.list = d.list;
    j.slot_found = d.slot_found;
    j.slot_subpix = d.slot_subpix;
    j.q = d.q;
    j.tres = d.tres;
    j.slot_v2 = d.slot_v2;
    j.outlier = d.outlier;
    j.mslot = d.mslot;
    j.mark = r->mark;
    j.rec = r->rec;
    j.max_records = r->max_records;
    c.gate = d_gate;
    c.frame_word = &t->mbox_dev->seq;
    c.head = t->mbox_dev->report_head;
    c.head_seq = &t->mbox_dev->report_seq;
    c.seq = t->seq;
    return c;
}
static_assert(FR_FRAME_LONG == POSE_CHAIN_LONG, "the fill reads the frame's sequence word");

static int tfb_enqueue(const TfbPlan& p, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, TmPoseForm* form,
                       TfbReport* rp) {
    const int nb = p.nb;
    ptam_tracker* lead = ts[0];
    ptam_ctx* ctx = lead->ctx;
    hipStream_t st = ctx->stream;
    int rc = tm_batch_join(nb, ts);
    if (rc) return rc;
    for (int i : p.rr_of)   // (the recovering cameras' banks are read on this queue: their adds and pose uploads must be done)
        if (sbi_bank_ctx(p.rv->banks[i]) != ctx) HIP_TRY(ptam_stream_wait(sbi_bank_ctx(p.rv->banks[i])->stream));
    int n_rep = 0, n_draw = 0, n_draw_max = 0;
    for (int i = 0; rp && i < nb; i++) {
        n_rep += rp->reports && rp->reports[i];
        n_draw += rp->seeds && ts[i]->d.n > 0 && ts[i]->d.n <= TR_DRAW_LDS_MAX;
    }
    TmBatchArgs a(nb, p.n_est, p.n_rr, p.rr_max_count, n_rep, n_draw);
    TmBatchDims dm;
    int n_dev_pose = 0;
    rc = a.reserve(lead);
    if (!rc) rc = tfb_fill(p, a, ts, curs, d_frames, &dm, &n_dev_pose);
    if (rc) return rc;
    tm_commit_seqs(nb, ts, st);
    if (rp) {   // (host only)
        rp->enqueued = true;
        FrChainJob* h_rep = a.host<FrChainJob>(TmBatchArgs::REPORT_JOB);
        TrDrawJob* h_draw = a.host<TrDrawJob>(TmBatchArgs::DRAW_JOB);
        TmBatchItem* h_it = a.host<TmBatchItem>(TmBatchArgs::ITEMS);
        for (int i = 0, kr = 0, kd = 0; i < nb; i++) {
            if (rp->seeds && ts[i]->d.n > 0) {   // the frame reads the orders where the draw writes them
                h_it[i].d.perm_a = ts[i]->perm_dev_a;
                h_it[i].d.perm_b = ts[i]->perm_dev_b;
                if (ts[i]->d.n <= TR_DRAW_LDS_MAX) {
                    h_draw[kd++] = TrDrawJob{rp->seeds[i], (unsigned long long)rp->frames[i], ts[i]->perm_dev_a, ts[i]->perm_dev_b, ts[i]->d.n, 0};
                    n_draw_max = std::max(n_draw_max, ts[i]->d.n);
                }
            }
            if (rp->reports && rp->reports[i]) h_rep[kr++] = tfb_report_job(ts[i], rp->reports[i], h_it[i].gate);
        }
    }
    HIP_TRY(hipMemcpyAsync(lead->batch_dev, a.hb, a.end((TmBatchArgs::Section)TmBatchArgs::LAST_UPLOADED), hipMemcpyHostToDevice, st));
    if (rp && rp->seeds) {   // the frames' orders, in front of everything that could read them (the set choice)
        rc = tr_draw_shuffles_batch_on(st, n_draw, n_draw_max, a.dev<TrDrawJob>(TmBatchArgs::DRAW_JOB));
        for (int i = 0; i < nb && !rc; i++)
            if (ts[i]->d.n > TR_DRAW_LDS_MAX)
                rc = tr_draw_shuffles_on(st, ts[i]->d.n, rp->seeds[i], (uint64_t)rp->frames[i], ts[i]->perm_dev_a, ts[i]->perm_dev_b, ts[i]->draw_keys);
        if (rc) return rc;
        for (int i = 0; i < nb; i++)   // the draws are enqueued: from here on the trackers' orders are the drawn ones
            if (ts[i]->d.n > 0) ts[i]->d.perm_a = ts[i]->perm_dev_a, ts[i]->d.perm_b = ts[i]->perm_dev_b;
    }
    // ---- keyframe, the estimators' steps, PVS, set choice ----
    const TmBatchItem* d_it = a.dev<TmBatchItem>(TmBatchArgs::ITEMS);
    const KfLevels& L0 = curs[0]->L;
    const int n_pyr = dm.gx * dm.gy, n_pvs = std::max(1, (dm.n_max + 255) / 256);
    hipLaunchKernelGGL(TM_HS_KERNEL(ctx, tm_pyr_pvs_batch_kernel), dim3(n_pyr + n_pvs, nb), dim3(256), 0, st, d_it, dm.gx, ctx->cam);
    rc = tfb_enqueue_sbi(p, ctx, a, L0, n_pvs, n_dev_pose);
    if (rc) return rc;
    hipLaunchKernelGGL(tm_compact_select_batch_kernel, dim3(1 + fast_compact_blocks(L0), nb), dim3(1024), 0, st, d_it, p.o);
    // ---- the two stages ----
    *form = tm_pose_form(true, dm.n_max, dm.ncc_max);
    for (int sg = 0; sg < 2 && !rc; sg++) rc = tm_enqueue_stage(ctx, nb, a, dm, p.o, sg, *form);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (n_rep > 0) return fr_fill_chain_core(st, n_rep, a.dev<FrChainJob>(TmBatchArgs::REPORT_JOB));   // behind the fine pose loops
    return PTAM_OK;
}

// The reports of a chain that has delivered every frame.  A frame that stayed in the chain: its head words arrive behind the frame's own
// result, under the frame's sequence number — a wait on host-mapped words, as the frame's.  A frame that was finished on its own queue
// (went_long): ptam_tracker_report_frames behind its passes.  A frame whose recovery failed: an empty report.
static int tfb_collect_reports(const TfbPlan& p, ptam_tracker* const* ts, hipStream_t st, const bool* went_long, TfbReport* rp) {
    rp->too_small = -1;
    for (int i = 0; i < p.nb; i++) {
        ptam_frame_report* r = rp->reports ? rp->reports[i] : nullptr;
        ptam_track_report_info ri = {};
        if (r) {
            ptam_tracker* t = ts[i];
            const int64_t tag = rp->tags ? rp->tags[i] : 0;
            if (went_long[i]) {
                const int rc = ptam_tracker_report_frames(1, &t, &r, &tag);
                if (rc == PTAM_E_ARG) {   // (the arguments were checked before the chain: the report is too small)
                    if (rp->too_small < 0) rp->too_small = i;
                    ri.report_too_small = 1;
                } else if (rc) return rc;
            } else {
                const unsigned long long seq = t->seq;
                const int rc = ptam_wait_mapped(st, "a frame's report", [&] { return *(volatile unsigned long long*)&t->mbox->report_seq == seq; });
                if (rc) return rc;
                int h[FR_HEAD_WORDS];
                std::memcpy(h, (const void*)t->mbox->report_head, sizeof h);
                r->info = ptam_frame_report_info_t{};
                const bool tracked = !p.recovering(i) || t->mbox->reloc.good;
                if (h[FR_H_RECORDS] > r->max_records) {
                    ri.report_too_small = 1;
                    if (rp->too_small < 0) {
                        rp->too_small = i;
                        ptam_set_error("bad argument: ptam_track_frames_report_batch: frame %d found %d points, its report holds %d records", i,
                                       h[FR_H_RECORDS], r->max_records);
                    }
                } else if (tracked) {
                    r->info.map_id = t->map_id;
                    r->info.tag = tag;
                    r->info.n_records = h[FR_H_RECORDS];
                    r->info.n_entries = h[FR_H_ENTRIES];
                    r->info.n_outliers = h[FR_H_OUTLIERS];
                }
                ri.report_in_chain = 1;
            }
            ri.report = r->info;
        }
        if (rp->infos) rp->infos[i] = ri;
    }
    return PTAM_OK;
}

// Every frame has arrived: the models and the estimators move, the infos are written (info_stride: frame i's info lies that many
// bytes behind frame i - 1's — inside the caller's own per-frame struct, or an array).
static void tfb_finish(const TfbPlan& p, ptam_tracker* const* ts, ptam_motion_model* models, ptam_trackmap_result* outs,
                       ptam_track_frame_info* info, size_t info_stride) {
    for (int i = 0; i < p.nb; i++) {
        ptam_motion_model m = p.tmp[(size_t)i];
        const bool est = p.est(i), rec = p.recovering(i);
        ptam_reloc_result* rr = rec ? (ptam_reloc_result*)((char*)p.rv->reloc + (size_t)i * p.rv->reloc_stride) : nullptr;
        if (rec) std::memcpy(rr, (const void*)&ts[i]->mbox->reloc, sizeof *rr);
        else if (est) std::memcpy(m.pose, (const void*)ts[i]->mbox->pose_in, 96);
        if (info) {
            ptam_track_frame_info& fi = *(ptam_track_frame_info*)((char*)info + (size_t)i * info_stride);
            std::memset(&fi, 0, sizeof fi);
            if (!rec) std::memcpy(fi.pose_in, m.pose, 96);
            else if (rr->good) std::memcpy(fi.pose_in, rr->pose, 96);
            if (est && !rec) std::memcpy(&fi.align, (const void*)&ts[i]->mbox->align, sizeof fi.align);
            fi.try_coarse = p.fo[(size_t)i].try_coarse;
            fi.coarse_max = p.fo[(size_t)i].coarse_max;
            fi.coarse_range = p.fo[(size_t)i].coarse_range;
        }
        if (!rec) {
            ptam_motion_update(&m, outs + i);
            models[i] = m;
        } else if (rr->good) {
            // Tracker::AttemptRecovery :203-205, then TrackMap and no UpdateMotionModel (:171-175): the scene depth of :692-696 is
            // all that ptam_motion_update would do here
            std::memcpy(m.pose, outs[i].pose, 96);
            std::memcpy(m.start_pose, rr->pose, 96);
            std::memset(m.velocity, 0, sizeof m.velocity);
            m.just_recovered = 0;
            motion_update_scene_depth(&m, outs + i);
            models[i] = m;
        } else {
            std::memset(outs + i, 0, sizeof outs[i]);   // (the mailbox still holds the frame before: nothing of TrackMap ran)
        }
        if (rec) sbi_reloc_commit(p.rv->scratch[i]);
        if (est) sbi_estimator_commit(p.ests[i]);
    }
}

static int tfb_impl(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, ptam_motion_model* models,
                    ptam_rotation_estimator* const* ests, const ptam_trackmap_opts* opts, ptam_trackmap_result* outs, ptam_track_frame_info* info,
                    size_t info_stride, const TfbRecover* rv, TfbReport* rp = nullptr) {
    TfbPlan p;
    int rc = tfb_plan(nb, ts, models, ests, opts, rv, &p);
    if (rc) return rc;
    TmPoseForm form = TM_POSE_GROUPED;
    std::unique_ptr<bool[]> went_long(rp ? new bool[(size_t)nb]() : nullptr);
    rc = tfb_enqueue(p, ts, curs, d_frames, &form, rp);
    if (!rc) rc = tm_collect(nb, ts, ts[0]->ctx->stream, p.o, true, form == TM_POSE_GROUPED, outs, went_long.get());
    if (!rc && rp) rc = tfb_collect_reports(p, ts, ts[0]->ctx->stream, went_long.get(), rp);
    if (rc) {   // the estimators are where they were
        for (int i : p.est_of) sbi_estimator_rollback(ests[i]);
        // a failure behind the first enqueue (the HIP runtime's): the reports' records may be half rewritten, so none of the call's
        // reports keeps an info that describes them — all of them are empty, whichever camera the failure was met at
        for (int i = 0; rp && rp->enqueued && rp->reports && i < nb; i++)
            if (rp->reports[i]) rp->reports[i]->info = ptam_frame_report_info_t{};
        return rc;
    }
    tfb_finish(p, ts, models, outs, info, info_stride);
    return PTAM_OK;
}

int ptam_track_frames_batch(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, ptam_motion_model* models,
                            ptam_rotation_estimator* const* ests, const ptam_trackmap_opts* opts, ptam_trackmap_result* outs,
                            ptam_track_frame_info* info) {
    ARG_TRY(models && outs);
    if (int rc = tm_batch_check(nb, ts, curs, d_frames)) return rc;
    return tfb_impl(nb, ts, curs, d_frames, models, ests, opts, outs, info, sizeof(ptam_track_frame_info), nullptr);
}

// One camera's state after its frame of ptam_track_frames_recover_batch (host only): the closest keyframe of the tracked pose,
// the tracking quality, and — on the tracking branch — IsNeedNewKeyFrame and whether the tracker would hand the frame to the map maker
static void tfr_advance_state(ptam_track_state& s, ptam_track_frame_state_info& fi, bool rec, const ptam_motion_model& model,
                              const ptam_sbi_bank* bank, const ptam_trackmap_result& out, const ptam_track_state_opts& so) {
    if (!rec) std::memset(&fi.reloc, 0, sizeof fi.reloc);
    fi.closest_kf = -1;
    fi.closest_kf_dist = 0.0;
    fi.need_new_keyframe = fi.want_keyframe = 0;
    fi.branch = !rec ? PTAM_FRAME_TRACKED : fi.reloc.good ? PTAM_FRAME_RECOVERED : PTAM_FRAME_RECOVERY_FAILED;
    s.frame++;                                         // :111
    if (fi.branch == PTAM_FRAME_RECOVERY_FAILED) return;
    s.model = model;
    // ClosestKeyFrame (src/MapMaker.cc:736-752) of the tracked pose: the first strictly lowest distance
    int count = 0;
    const double* kp = bank ? sbi_bank_camera_positions(bank, &count) : nullptr;
    if (kp && count > 0) {
        double best = 9999999999.9, here[3];
        se3_camera_position(out.pose, here);
        for (int k = 0; k < count; k++) {
            const double* there = kp + 3 * (size_t)k;
            const double dx = there[0] - here[0], dy = there[1] - here[1], dz = there[2] - here[2];
            const double d = std::sqrt(dx * dx + dy * dy + dz * dz);   // KeyFrameLinearDist
            if (d < best) best = d, fi.closest_kf = k;
        }
        if (fi.closest_kf >= 0) fi.closest_kf_dist = best;
    }
    ptam_assess_tracking_quality(&s, out.attempted, out.found, fi.closest_kf_dist, &so);
    if (fi.branch == PTAM_FRAME_TRACKED) {         // :146-161; the recovery branch decides nothing about keyframes
        if (fi.closest_kf >= 0)                    // IsNeedNewKeyFrame, src/MapMaker.cc:754-763
            fi.need_new_keyframe = fi.closest_kf_dist * (1.0 / s.model.scene_depth_mean) > so.max_kf_dist_wiggle_mult * so.wiggle_scale_depth_normalized;
        fi.want_keyframe = s.quality == PTAM_TRACK_GOOD && s.frame - s.last_keyframe_dropped > 20;
    }
}

// ---- Tracker::TrackFrame for a good map (src/Tracker.cc:127-176) for nb cameras: ptam_track_frames_batch's chain, in which a camera
// that is lost runs the relocaliser instead of the prediction (tfb_impl with a TfbRecover); the state machine around it is host code ----
// rp (nullable): the report batch's extras, checked
static int tfr_impl(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, ptam_track_state* states,
                    ptam_rotation_estimator* const* ests, ptam_sbi_bank* const* banks, ptam_sbi* const* scratch, const ptam_trackmap_opts* opts,
                    const ptam_track_state_opts* state_opts, ptam_trackmap_result* outs, ptam_track_frame_state_info* info, TfbReport* rp) {
    ptam_track_state_opts so;
    ptam_track_state_opts_default(&so);
    if (state_opts) so = *state_opts;
    ARG_TRY(so.reloc_blur > 0.0 && so.reloc_blur <= 5.0);
    // the branches (:129, :168), and the recovering cameras' refusals — before anything is enqueued or moved
    std::vector<char> rec((size_t)nb, 0);
    int n_rr = 0;
    for (int i = 0; i < nb; i++) {
        if (states[i].lost_frames < 3) continue;
        rec[(size_t)i] = 1;
        n_rr++;
        if (!banks || !banks[i] || !scratch || !scratch[i]) {
            ptam_set_error("camera %d is lost and has no %s", i, banks && banks[i] ? "scratch image" : "bank");
            return PTAM_E_ARG;
        }
        if (int rc = sbi_reloc_check(banks[i], scratch[i], ts[0]->ctx->device, curs[i])) return rc;
        ARG_TRY(std::memcmp(&sbi_bank_ctx(banks[i])->cam, &ts[0]->ctx->cam, sizeof(DevCam)) == 0);
        for (int j = 0; j < i; j++) ARG_TRY(!rec[(size_t)j] || scratch[j] != scratch[i]);
    }
    std::vector<ptam_motion_model> models((size_t)nb);
    for (int i = 0; i < nb; i++) models[(size_t)i] = states[i].model;
    // (the frame's info and the relocaliser's result are written where they stay: info[i].frame and info[i].reloc, after every wait)
    std::vector<ptam_track_frame_state_info> own;
    if (!info) {
        own.resize((size_t)nb);
        info = own.data();
    }
    const size_t stride = sizeof(ptam_track_frame_state_info);
    const TfbRecover rv = {rec.data(), banks, scratch, so.reloc_blur, so.reloc_max_score, &info[0].reloc, stride};
    if (int rc = tfb_impl(nb, ts, curs, d_frames, models.data(), ests, opts, outs, &info[0].frame, stride, n_rr ? &rv : nullptr, rp)) return rc;
    // ---- every frame has arrived: the states move ----
    for (int i = 0; i < nb; i++)
        tfr_advance_state(states[i], info[i], rec[(size_t)i] != 0, models[(size_t)i], banks ? banks[i] : nullptr, outs[i], so);
    return PTAM_OK;
}

int ptam_track_frames_recover_batch(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, ptam_track_state* states,
                                    ptam_rotation_estimator* const* ests, ptam_sbi_bank* const* banks, ptam_sbi* const* scratch,
                                    const ptam_trackmap_opts* opts, const ptam_track_state_opts* state_opts, ptam_trackmap_result* outs,
                                    ptam_track_frame_state_info* info) {
    ARG_TRY(states && outs);
    if (int rc = tm_batch_check(nb, ts, curs, d_frames)) return rc;
    return tfr_impl(nb, ts, curs, d_frames, states, ests, banks, scratch, opts, state_opts, outs, info, nullptr);
}

// ---- the same frame with its report filled inside the chain and its two orders drawn there (framereport.hip, tracker_run.hip) ----
int ptam_track_frames_report_batch(int nb, ptam_tracker* const* ts, ptam_kf* const* curs, const uint8_t* const* d_frames, ptam_track_state* states,
                                   ptam_rotation_estimator* const* ests, ptam_sbi_bank* const* banks, ptam_sbi* const* scratch,
                                   const ptam_trackmap_opts* opts, const ptam_track_state_opts* state_opts, ptam_trackmap_result* outs,
                                   ptam_track_frame_state_info* info, ptam_frame_report* const* reports, const int64_t* tags,
                                   const uint64_t* shuffle_seeds, ptam_track_report_info* report_info) {
    ARG_TRY(states && outs);
    if (int rc = tm_batch_check(nb, ts, curs, d_frames)) return rc;
    // ---- the reports' refusals: nothing is enqueued, and no report is touched, before all of them have passed
    for (int i = 0; reports && i < nb; i++) {
        if (!reports[i]) continue;
        ARG_TRY(reports[i]->ctx->device == ts[i]->ctx->device);
        for (int j = 0; j < i; j++) ARG_TRY(reports[j] != reports[i]);
    }
    for (int i = 0; reports && i < nb; i++)
        if (reports[i] && !ts[i]->has_serials) {
            ptam_set_error("ptam_track_frames_report_batch: the map of tracker %d did not come from a snapshot", i);
            return PTAM_E_STATE;
        }
    for (int i = 0; reports && i < nb; i++)
        if (reports[i])
            if (int rc = fr_mark_room(reports[i], ts[i]->d.n)) return rc;
    std::vector<int64_t> frames((size_t)nb);
    for (int i = 0; i < nb; i++) frames[(size_t)i] = states[i].frame;
    TfbReport rp = {reports, tags, shuffle_seeds, frames.data(), report_info, -1, false};
    if (int rc = tfr_impl(nb, ts, curs, d_frames, states, ests, banks, scratch, opts, state_opts, outs, info, &rp)) return rc;
    return rp.too_small < 0 ? PTAM_OK : PTAM_E_ARG;   // (every frame is delivered and every state has moved; that report is empty)
}

int ptam_tracker_read_reloc_ssd(ptam_tracker* lead, int row, int count, double* ssd_out) {
    ARG_TRY(lead && ssd_out && lead->reloc_count && row >= 0 && row < (int)lead->reloc_count->size());
    ARG_TRY(count >= 1 && count <= (*lead->reloc_count)[(size_t)row]);
    HIP_TRY(hipSetDevice(lead->ctx->device));
    HIP_TRY(ptam_stream_wait(lead->ctx->stream));
    HIP_TRY(hipMemcpy(ssd_out, lead->reloc_ssd + (size_t)row * (size_t)lead->reloc_stride, (size_t)count * 8, hipMemcpyDeviceToHost));
    return PTAM_OK;
}

int ptam_tracker_read_iteration_set(ptam_tracker* t, ptam_trackmap_meas* out, int cap, int* n_out) {
    ARG_TRY(t && n_out);
    ptam_ctx* ctx = t->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    TmCtl c;
    HIP_TRY(hipMemcpy(&c, t->d.ctl, sizeof c, hipMemcpyDeviceToHost));
    const int ns = c.n_slots;
    *n_out = ns;
    if (!out || ns == 0) return PTAM_OK;
    std::vector<int> list((size_t)ns), sf((size_t)ns), ss((size_t)ns), ms((size_t)std::max(c.n_meas, 1)), ou((size_t)std::max(c.n_meas, 1));
    std::vector<ptam_patch_query> q((size_t)ns);
    std::vector<ptam_template_result> tr((size_t)ns);
    std::vector<double2> v2((size_t)ns);
    HIP_TRY(hipMemcpy(list.data(), t->d.list, (size_t)ns * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sf.data(), t->d.slot_found, (size_t)ns * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ss.data(), t->d.slot_subpix, (size_t)ns * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q.data(), t->d.q, (size_t)ns * sizeof(ptam_patch_query), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(v2.data(), t->d.slot_v2, (size_t)ns * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tr.data(), t->d.tres, (size_t)ns * sizeof(ptam_template_result), hipMemcpyDeviceToHost));
    if (c.n_meas > 0) {
        HIP_TRY(hipMemcpy(ms.data(), t->d.mslot, (size_t)c.n_meas * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ou.data(), t->d.outlier, (size_t)c.n_meas * 4, hipMemcpyDeviceToHost));
    }
    for (int s = 0; s < ns && s < cap; s++) {
        ptam_trackmap_meas& m = out[s];
        m.point = list[(size_t)s];
        m.level = tr[(size_t)s].bad ? -1 : q[(size_t)s].level;   // (a bad template: the point was dropped before the search)
        m.found = sf[(size_t)s];
        m.did_subpix = ss[(size_t)s];
        m.outlier = 0;
        m.pad_ = 0;
        m.v2_found[0] = v2[(size_t)s].x;
        m.v2_found[1] = v2[(size_t)s].y;
    }
    if (c.outlier_by_slot) {   // (fused pose kernel: the flags sit at the slots)
        std::vector<int> os((size_t)ns);
        HIP_TRY(hipMemcpy(os.data(), t->d.outlier, (size_t)ns * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < ns && s < cap; s++) out[s].outlier = sf[(size_t)s] ? os[(size_t)s] : 0;
        return PTAM_OK;
    }
    for (int k = 0; k < c.n_meas; k++)
        if (ms[(size_t)k] < cap) out[ms[(size_t)k]].outlier = ou[(size_t)k];
    return PTAM_OK;
}

}   // extern "C"

int pose_hazards_read_trackmap(hipStream_t st, unsigned long long* out) {   // (this translation unit's copy of the counter)
    HIP_TRY(hipMemcpyFromSymbolAsync(out, HIP_SYMBOL(g_pose_hazards), 8, 0, hipMemcpyDeviceToHost, st));
    return PTAM_OK;
}
void trackmap_preload_kernels() {
    ptam_preload((const void*)tm_select_kernel);
    ptam_preload((const void*)tm_pyr_pvs_kernel<PTAM_HALFSAMPLE_R>);
    ptam_preload((const void*)tm_pyr_pvs_kernel<PTAM_HALFSAMPLE_T>);
    ptam_preload((const void*)tm_compact_select_kernel);
    ptam_preload((const void*)tm_kf_pvs_kernel<PTAM_HALFSAMPLE_R>);
    ptam_preload((const void*)tm_kf_pvs_kernel<PTAM_HALFSAMPLE_T>);
    ptam_preload((const void*)tm_search_kernel);
    ptam_preload((const void*)tm_gather_kernel);
    ptam_preload((const void*)tm_finder_carry_kernel);
    ptam_preload((const void*)tm_take_prev_kernel);
    ptam_preload((const void*)tm_identity_kernel);
    ptam_preload((const void*)tm_iteration_serials_kernel);
    ptam_preload((const void*)tm_pose_kernel<1, GS_WAVE_LIMIT>);
    ptam_preload((const void*)tm_pose_kernel<1, GS_THREADS>);
    ptam_preload((const void*)tm_pose_kernel<GS_MPT, GS_THREADS>);
    ptam_preload((const void*)tm_pose_batch_kernel<1, GS_WAVE_LIMIT>);
    ptam_preload((const void*)tm_pose_batch_kernel<1, GS_THREADS>);
    ptam_preload((const void*)tm_pose_batch_kernel<GS_MPT, GS_THREADS>);
    ptam_preload((const void*)tm_pyr_pvs_batch_kernel<PTAM_HALFSAMPLE_R>);
    ptam_preload((const void*)tm_pyr_pvs_batch_kernel<PTAM_HALFSAMPLE_T>);
    ptam_preload((const void*)tm_compact_select_batch_kernel);
    ptam_preload((const void*)tm_search_batch_kernel);
    ptam_preload((const void*)tm_gather_batch_kernel);
    ptam_preload((const void*)tm_pvs_batch_kernel);
}
