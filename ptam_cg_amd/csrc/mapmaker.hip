// mapmaker.hip — MapMaker::AddSomeMapPoints (src/MapMaker.cc:448-457) on gfx950: ThinCandidates (:415-441) and
// AddPointEpipolar (:529-688) for a list of levels, enqueued back to back without a host round trip.
//
// Per visited level, three launches:
//   epi_select_kernel  ONE WORKGROUP (1024 lanes): the level's maximal corners 1024 at a time, lane = corner.  Candidate =
//                      Shi-Tomasi score > threshold (src/KeyFrame.cc:66-76); a candidate is thinned against the device busy
//                      list in integer arithmetic; two ordered compactions (ballot + per-wave counts) give every kept
//                      candidate its index before thinning and its slot in the kept list.
//   epi_point_kernel   ONE WAVE PER KEPT CANDIDATE (grid sized by the level's maximal corners, the wave reads the kept count):
//                      the ray / line geometry in wave-uniform fp64 in the reference's operation order without FMA
//                      contraction (its results feed comparisons), then wave_epipolar_scan and wave_subpix (patch_device.h,
//                      the code of ptam_epipolar_search_batch / ptam_subpix_batch), the triangulation by one-sided Jacobi on
//                      the 4x4 system and RefreshPixelVectors; lane 0 writes the point and its return path.
//   epi_emit_kernel    ONE WORKGROUP: the made points in kept order appended to the output, their SRC_ROOT positions to the busy
//                      list of the later levels (:679-683), the per-level counts of every return path.
#include "common.h"
#include <vector>

#include "keyframe.h"
#include "track_internal.h"
#include "patch_device.h"
#include "mapmaker_device.h"
#include "mapmaker_internal.h"   // EpiBusy, EpiRun, the chain's launch sequence

namespace {

struct EpiCand {        // a kept candidate: index before thinning, irLevelPos
    int cand, x, y, pad_;
};
struct EpiArgs {
    DevCam cam;
    double Rs[9], ts[3], Rt[9], tt[3];   // kSrc.se3CfromW, kTarget.se3CfromW
    double depth_mean, depth_sigma, wiggle;
    int its;
};
enum { EPI_MADE = 0, EPI_RAY, EPI_LINE, EPI_TEMPLATE_BAD, EPI_NO_MATCH, EPI_SUBPIX, EPI_N };

}   // namespace

// ---- ThinCandidates (:415-441) on the level's candidates ----------------------------------------------------------------
__global__ void __launch_bounds__(1024) epi_select_kernel(KfLevels S, int lev, double thr, const EpiBusy* __restrict__ busy,
                                                          const int* __restrict__ d_nbusy, EpiCand* __restrict__ kept,
                                                          int* __restrict__ d_nkept, ptam_epipolar_level_stats* __restrict__ st) {
    __shared__ int wc[16], wk[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n = S.nmax[lev], nb = *d_nbusy;
    const double scale = (double)(1 << lev);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int base_c = 0, base_k = 0;
    for (int start = 0; start < n; start += 1024) {
        const int i = start + tid;
        bool isc = false, keep = false;
        ptam_int2 c = {0, 0};
        if (i < n) {
            isc = S.st[lev][i] > thr;   // vCandidates: Shi-Tomasi score > MapMaker.CandidateMinShiTomasiScore
            c = S.mcorners[lev][i];
        }
        if (isc) {
            keep = true;
            for (int b = 0; b < nb; b++) {
                const EpiBusy e = busy[b];
                if (e.level != lev && e.level != lev + 1) continue;
                const double bx = e.x / scale, by = e.y / scale;   // ir_rounded(v2RootPos / LevelScale(nLevel))
                const int ix = (int)(bx > 0.0 ? bx + 0.5 : bx - 0.5), iy = (int)(by > 0.0 ? by + 0.5 : by - 0.5);
                const unsigned dx = (unsigned)(ix - c.x), dy = (unsigned)(iy - c.y);
                if (dx * dx + dy * dy < 100u) {   // mag_squared() < nMinMagSquared (unsigned comparison)
                    keep = false;
                    break;
                }
            }
        }
        const unsigned long long mc = __ballot(isc), mk = __ballot(keep);
        if (lane == 0) {
            wc[wid] = __popcll(mc);
            wk[wid] = __popcll(mk);
        }
        __syncthreads();
        int pc = 0, pk = 0, tc = 0, tk = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wid) pc += wc[w], pk += wk[w];
            tc += wc[w];
            tk += wk[w];
        }
        if (keep) {
            EpiCand e;
            e.cand = base_c + pc + __popcll(mc & lt);
            e.x = c.x;
            e.y = c.y;
            e.pad_ = 0;
            kept[base_k + pk + __popcll(mk & lt)] = e;
        }
        base_c += tc;
        base_k += tk;
        __syncthreads();   // (wc / wk are rewritten by the next chunk)
    }
    if (tid == 0) {
        *d_nkept = base_k;
        st->candidates = base_c;
        st->kept_after_thinning = base_k;
    }
}

// ---- AddPointEpipolar (:529-688), one wave per kept candidate ------------------------------------------------------------
__global__ void __launch_bounds__(256) epi_point_kernel(EpiArgs a, KfLevels S, KfLevels T, int lev, const double2* __restrict__ implane,
                                                        const EpiCand* __restrict__ kept, const int* __restrict__ d_nkept,
                                                        int* __restrict__ status, ptam_new_map_point* __restrict__ pts) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= *d_nkept) return;
    const EpiCand cd = kept[k];
    const int nLevelScale = 1 << lev;
    const double scale = (double)nLevelScale;
    // v2RootPos = LevelZeroPos(irLevelPos, nLevel)
    const double root_x = nc_sub(nc_mul(nc_add((double)cd.x, 0.5), scale), 0.5);
    const double root_y = nc_sub(nc_mul(nc_add((double)cd.y, 0.5), scale), 0.5);
    double ray_sc[3];   // v3Ray_SC, normalised (also v3Center_NC)
    unit_ray(a.cam, root_x, root_y, ray_sc);
    double ray_wc[3], dirn[3];
#pragma unroll
    for (int i = 0; i < 3; i++) ray_wc[i] = rt_row(a.Rs, i, ray_sc);   // kSrc.se3CfromW.get_rotation().inverse() * v3Ray_SC
#pragma unroll
    for (int i = 0; i < 3; i++) dirn[i] = r_row(a.Rt, i, ray_wc);      // kTarget.se3CfromW.get_rotation() * v3RayUnit_WC
    const double ms = nc_sub(a.depth_mean, a.depth_sigma), ps = nc_add(a.depth_mean, a.depth_sigma);
    const double start_depth = a.wiggle < ms ? ms : a.wiggle;                           // max(mdWiggleScale, dMean - dSigma)
    const double w40 = nc_mul(40.0, a.wiggle);
    const double end_depth = ps < w40 ? ps : w40;                                        // min(40 * mdWiggleScale, dMean + dSigma)
    double cw[3], ctc[3], rs[3], re[3];
#pragma unroll
    for (int i = 0; i < 3; i++) cw[i] = -rt_row(a.Rs, i, a.ts);                        // kSrc.se3CfromW.inverse().get_translation()
#pragma unroll
    for (int i = 0; i < 3; i++) ctc[i] = nc_add(r_row(a.Rt, i, cw), a.tt[i]);         // kTarget.se3CfromW * v3CamCenter_WC
#pragma unroll
    for (int i = 0; i < 3; i++) {
        rs[i] = nc_add(ctc[i], nc_mul(start_depth, dirn[i]));
        re[i] = nc_add(ctc[i], nc_mul(end_depth, dirn[i]));
    }
    int code = EPI_MADE;
    ptam_new_map_point P;
    if (re[2] <= rs[2] || re[2] <= 0.0) code = EPI_RAY;   // :569-572
    ptam_epipolar_query q;
    if (code == EPI_MADE) {
        if (rs[2] <= 0.0) {   // :573-574
            const double s = nc_sub(0.001, rs[2] / dirn[2]);
#pragma unroll
            for (int i = 0; i < 3; i++) rs[i] = nc_add(rs[i], nc_mul(dirn[i], s));
        }
        const double Ax = rs[0] / rs[2], Ay = rs[1] / rs[2], Bx = re[0] / re[2], By = re[1] / re[2];   // project()
        double alx = nc_sub(Ax, Bx), aly = nc_sub(Ay, By);
        const double len2 = nc_add(nc_mul(alx, alx), nc_mul(aly, aly));
        if (len2 < 1e-8) code = EPI_LINE;   // :581-584
        else {
            const double nrm = sqrt(len2);
            alx = alx / nrm;
            aly = aly / nrm;
            const double nx = aly, ny = -alx;
            const double nd = nc_add(nc_mul(Ax, nx), nc_mul(Ay, ny));   // v2A * v2Normal
            if (fabs(nd) > a.cam.largest_radius) code = EPI_LINE;     // :588-589
            else {
                const double la = nc_add(nc_mul(alx, Ax), nc_mul(aly, Ay)), lb = nc_add(nc_mul(alx, Bx), nc_mul(aly, By));
                double mn = nc_sub(lb < la ? lb : la, 0.05), mx = nc_add(la < lb ? lb : la, 0.05);
                if (mn < -2.0) mn = -2.0;
                if (mx < -2.0) mx = -2.0;
                if (mn > 2.0) mn = 2.0;
                if (mx > 2.0) mx = 2.0;
                const double dmax = nc_mul(a.cam.one_pixel_dist, nc_add(4.0, nc_mul(1.0, scale)));
                q.level_x = cd.x;
                q.level_y = cd.y;
                q.normal[0] = nx;
                q.normal[1] = ny;
                q.norm_dist = nd;
                q.along[0] = alx;
                q.along[1] = aly;
                q.min_len = mn;
                q.max_len = mx;
                q.max_dist_sq = nc_mul(dmax, dmax);
            }
        }
    }
    if (code == EPI_MADE) {
        ptam_epipolar_result r;
        const int Tp = wave_epipolar_scan(S, T, lev, implane, q, lane, r);
        if (r.template_bad) code = EPI_TEMPLATE_BAD;
        else if (r.best < 0) code = EPI_NO_MATCH;
        else {
            const ptam_int2 c = T.corners[lev][r.best];
            ptam_subpix_query sq;
            sq.level = lev;
            sq.max_its = a.its;
            sq.coarse_pos[0] = (c.x + 0.5) * nLevelScale - 0.5;   // LevelZeroPos(vIR[nBest], nLevel)
            sq.coarse_pos[1] = (c.y + 0.5) * nLevelScale - 0.5;
            ptam_subpix_result sr;
            wave_subpix(T, sq, Tp, lane, sr);
            if (!sr.converged) code = EPI_SUBPIX;
            else {
                P.target_pos[0] = sr.pos[0];
                P.target_pos[1] = sr.pos[1];
                P.target_corner = r.best;
                P.best_zmssd = r.best_zmssd;
            }
        }
    }
    if (code == EPI_MADE) {
        // se3SrcfromTarget = kSrc.se3CfromW * kTarget.se3CfromW.inverse(): R = Rs Rt^T, t = ts + Rs (-(Rt^T tt))
        double R[9], tti[3], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                R[3 * i + j] = nc_add(nc_add(nc_mul(a.Rs[3 * i], a.Rt[3 * j]), nc_mul(a.Rs[3 * i + 1], a.Rt[3 * j + 1])),
                                      nc_mul(a.Rs[3 * i + 2], a.Rt[3 * j + 2]));
#pragma unroll
        for (int i = 0; i < 3; i++) tti[i] = -rt_row(a.Rt, i, a.tt);
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = nc_add(a.ts[i], r_row(a.Rs, i, tti));
        double uax, uay, ubx, uby;
        cam_unproject(a.cam, root_x, root_y, uax, uay);
        cam_unproject(a.cam, P.target_pos[0], P.target_pos[1], ubx, uby);
        double A[16] = {-1.0, 0.0, ubx, 0.0, 0.0, -1.0, uby, 0.0};
#pragma unroll
        for (int j = 0; j < 4; j++) {   // A[2] = v2A[0] * PDash[2] - PDash[0], A[3] = v2A[1] * PDash[2] - PDash[1]
            const double p0 = j < 3 ? R[j] : t[0], p1 = j < 3 ? R[3 + j] : t[1], p2 = j < 3 ? R[6 + j] : t[2];
            A[8 + j] = nc_sub(nc_mul(uax, p2), p0);
            A[12 + j] = nc_sub(nc_mul(uay, p2), p1);
        }
        double v4[4];
        smallest_right_singular_vector(A, v4);
        if (v4[3] == 0.0) v4[3] = 0.00001;
        const double xt[3] = {v4[0] / v4[3], v4[1] / v4[3], v4[2] / v4[3]};   // project(v4Smallest): point in kTarget's frame
        double world[3];
#pragma unroll
        for (int i = 0; i < 3; i++) world[i] = nc_add(rt_row(a.Rt, i, xt), tti[i]);   // kTarget.se3CfromW.inverse() * v3
        // the patch source: v3Center_NC, v3OneRightFromCenter_NC, v3OneDownFromCenter_NC (:661-667)
        double right[3], down[3];
        unit_ray(a.cam, nc_add(root_x, scale), root_y, right);
        unit_ray(a.cam, root_x, nc_add(root_y, scale), down);
        // MapPoint::RefreshPixelVectors (src/Map.cc:40-65), v3Normal_NC = (0, 0, -1)
        double pc[3];
#pragma unroll
        for (int i = 0; i < 3; i++) pc[i] = nc_add(r_row(a.Rs, i, world), a.ts[i]);
        auto dot_n = [](const double v[3]) { return fabs(nc_add(nc_add(nc_mul(v[0], 0.0), nc_mul(v[1], 0.0)), nc_mul(v[2], -1.0))); };
        const double cam_h = dot_n(pc), rc = dot_n(ray_sc), rr = dot_n(right), rd = dot_n(down);
        double dr_[3], dd_[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double cen = nc_mul(ray_sc[i], cam_h) / rc;
            dr_[i] = nc_sub(nc_mul(right[i], cam_h) / rr, cen);
            dd_[i] = nc_sub(nc_mul(down[i], cam_h) / rd, cen);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            P.point.world[i] = world[i];
            P.point.pixel_right_w[i] = rt_row(a.Rs, i, dr_);
            P.point.pixel_down_w[i] = rt_row(a.Rs, i, dd_);
            P.center_nc[i] = ray_sc[i];
            P.one_right_nc[i] = right[i];
            P.one_down_nc[i] = down[i];
        }
        P.src_root_pos[0] = root_x;
        P.src_root_pos[1] = root_y;
        P.level = lev;
        P.center_x = cd.x;
        P.center_y = cd.y;
        P.candidate = cd.cand;
    }
    if (lane == 0) {
        status[k] = code;
        if (code == EPI_MADE) pts[k] = P;
    }
}

// ---- the level's made points, in candidate order, to the output and the busy list (:675-683) -----------------------------
__global__ void __launch_bounds__(1024) epi_emit_kernel(int lev, const int* __restrict__ d_nkept, const int* __restrict__ status,
                                                        const ptam_new_map_point* __restrict__ pts, ptam_new_map_point* __restrict__ out,
                                                        int* __restrict__ d_nout, EpiBusy* __restrict__ busy, int* __restrict__ d_nbusy,
                                                        ptam_epipolar_level_stats* __restrict__ st) {
    __shared__ int wm[16], cnt[EPI_N];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < EPI_N) cnt[tid] = 0;
    const int n = *d_nkept, out0 = *d_nout, busy0 = *d_nbusy;
    const unsigned long long lt = (1ull << lane) - 1ull;
    __syncthreads();
    int base = 0;
    for (int start = 0; start < n; start += 1024) {
        const int i = start + tid;
        const int s = i < n ? status[i] : -1;
        if (s >= 0 && s < EPI_N) atomicAdd(&cnt[s], 1);
        const bool made = s == EPI_MADE;
        const unsigned long long m = __ballot(made);
        if (lane == 0) wm[wid] = __popcll(m);
        __syncthreads();
        int pm = 0, tm = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wid) pm += wm[w];
            tm += wm[w];
        }
        if (made) {
            const int o = base + pm + __popcll(m & lt);
            const ptam_new_map_point p = pts[i];
            out[out0 + o] = p;
            EpiBusy b;
            b.x = p.src_root_pos[0];
            b.y = p.src_root_pos[1];
            b.level = lev;
            b.pad_ = 0;
            busy[busy0 + o] = b;   // kSrc.mMeasurements[pNew] = m (SRC_ROOT)
        }
        base += tm;
        __syncthreads();
    }
    if (tid == 0) {
        *d_nout = out0 + base;
        *d_nbusy = busy0 + base;
        st->ray_rejected = cnt[EPI_RAY];
        st->line_rejected = cnt[EPI_LINE];
        st->template_bad = cnt[EPI_TEMPLATE_BAD];
        st->no_match = cnt[EPI_NO_MATCH];
        st->subpix_failed = cnt[EPI_SUBPIX];
        st->made = cnt[EPI_MADE];
    }
}

extern "C" {

void ptam_epipolar_opts_default(ptam_epipolar_opts* o) {
    if (!o) return;
    o->depth_mean = 1.0;   // Tracker's initial scene depth (src/Tracker.cc:56)
    o->depth_sigma = 1.0;
    o->wiggle_scale = 0.1;   // MapMaker.WiggleScale
    o->min_shi_tomasi = 70.0;   // MapMaker.CandidateMinShiTomasiScore default (src/KeyFrame.cc:63)
    o->subpix_max_its = 10;   // src/MapMaker.cc:642
    o->n_levels = 4;
    const int lv[4] = {3, 0, 1, 2};   // AddKeyFrameFromTopOfQueue :511-514
    for (int i = 0; i < 4; i++) o->levels[i] = lv[i];
}

int ptam_add_map_points_epipolar(ptam_ctx* ctx, const ptam_kf* src, const double src_pose[12], ptam_kf* target, const double target_pose[12],
                                 const ptam_epipolar_opts* opts, int n_busy, const int32_t* busy_level, const double* busy_root_xy,
                                 ptam_new_map_point* out, int cap, int32_t* n_out, ptam_epipolar_level_stats* stats) {
    ARG_TRY(ctx && src && src_pose && target && target_pose && opts && n_out);
    ARG_TRY(n_busy >= 0 && cap >= 0);
    ARG_TRY(n_busy == 0 || (busy_level && busy_root_xy));
    ARG_TRY(out || cap == 0);
    ARG_TRY(src->device == ctx->device && target->device == ctx->device);
    for (int i = 0; i < n_busy; i++) ARG_TRY(busy_level[i] >= 0 && busy_level[i] < PTAM_LEVELS);
    if (int rc = epi_check(src, opts)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    EpiRun run;
    if (int rc = epi_sizes(ctx, src, opts, run)) return rc;
    const int sum = run.sum, nl = run.nl;
    ARG_TRY(cap >= sum);
    if (int rc = epi_carve(ctx, target, opts, n_busy, run)) return rc;
    const size_t b_res = EPI_HDR_BYTES;
    void* hp;
    if (int rc = ctx_pinned(ctx, b_res + sizeof(ptam_new_map_point) * (size_t)sum, &hp)) return rc;
    int* h_hdr = (int*)hp;
    ptam_new_map_point* h_out = (ptam_new_map_point*)((char*)hp + b_res);
    // the caller's busy measurements (pageable: staged before the call returns, which is after the final wait)
    std::vector<EpiBusy> hb((size_t)n_busy);
    for (int i = 0; i < n_busy; i++) {
        hb[(size_t)i].x = busy_root_xy[2 * i];
        hb[(size_t)i].y = busy_root_xy[2 * i + 1];
        hb[(size_t)i].level = busy_level[i];
        hb[(size_t)i].pad_ = 0;
    }
    if (n_busy > 0) HIP_TRY(hipMemcpyAsync(run.d_busy, hb.data(), sizeof(EpiBusy) * (size_t)n_busy, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(run.d_hdr, 0, b_res, ctx->stream));
    HIP_TRY(hipMemcpyAsync(run.d_hdr, &n_busy, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = epi_launch_chain(ctx, src, src_pose, target, target_pose, opts, run)) return rc;
    HIP_TRY(hipMemcpyAsync(h_hdr, run.d_hdr, b_res, hipMemcpyDeviceToHost, ctx->stream));
    if (sum > 0) HIP_TRY(hipMemcpyAsync(h_out, run.d_out, sizeof(ptam_new_map_point) * (size_t)sum, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    const int made = h_hdr[1];
    if (made > sum) {
        ptam_set_error("add_map_points_epipolar: %d points made, room for %d", made, sum);
        return PTAM_E_STATE;
    }
    if (made > 0) std::memcpy(out, h_out, sizeof(ptam_new_map_point) * (size_t)made);
    *n_out = made;
    if (stats) std::memcpy(stats, (const char*)h_hdr + 16, sizeof(ptam_epipolar_level_stats) * (size_t)nl);
    return PTAM_OK;
}

}   // extern "C"

int epi_check(const ptam_kf* src, const ptam_epipolar_opts* opts) {
    ARG_TRY(src && opts);
    const int nl = opts->n_levels;
    ARG_TRY(nl >= 1 && nl <= PTAM_LEVELS);
    for (int i = 0; i < nl; i++) {
        ARG_TRY(opts->levels[i] >= 0 && opts->levels[i] < PTAM_LEVELS);
        for (int j = 0; j < i; j++) ARG_TRY(opts->levels[i] != opts->levels[j]);
    }
    if (!src->rest_made) {
        ptam_set_error("add_map_points_epipolar: the source keyframe has no MakeKeyFrame_Rest since its MakeKeyFrame_Lite");
        return PTAM_E_STATE;
    }
    return PTAM_OK;
}

int epi_sizes(ptam_ctx* ctx, const ptam_kf* src, const ptam_epipolar_opts* opts, EpiRun& run) {
    run.nl = opts->n_levels;
    run.sum = run.most = 0;
    for (int i = 0; i < run.nl; i++) {
        int rc = ptam_kf_rest_info(ctx, src, opts->levels[i], &run.n_max[i]);
        if (rc) return rc;
        run.sum += run.n_max[i];
        run.most = max(run.most, run.n_max[i]);
    }
    return PTAM_OK;
}

int epi_carve(ptam_ctx* ctx, ptam_kf* target, const ptam_epipolar_opts* opts, int n_busy, EpiRun& run) {
    for (int i = 0; i < run.nl; i++) {
        int rc = kf_build_implane(ctx, target, opts->levels[i]);   // (bImplaneCornersCached :609-614)
        if (rc) return rc;
    }
    // device scratch: busy list (caller's + one per made point), kept list, per-candidate status and point, output, counters
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int sum = run.sum, most = run.most;
    const size_t b_busy = up(sizeof(EpiBusy) * (size_t)(n_busy + sum + 1)), b_kept = up(sizeof(EpiCand) * (size_t)(most + 1)),
                 b_stat = up(sizeof(int) * (size_t)(most + 1)), b_pts = up(sizeof(ptam_new_map_point) * (size_t)(most + 1)),
                 b_out = up(sizeof(ptam_new_map_point) * (size_t)(sum + 1)), b_hdr = up(EPI_HDR_BYTES);
    void* s;
    int rc = ctx_scratch(ctx, b_busy + b_kept + b_stat + b_pts + b_out + b_hdr, &s);
    if (rc) return rc;
    char* p = (char*)s;
    run.d_busy = (EpiBusy*)p;
    run.d_kept = (void*)(p += b_busy);
    run.d_status = (int*)(p += b_kept);
    run.d_pts = (ptam_new_map_point*)(p += b_stat);
    run.d_out = (ptam_new_map_point*)(p += b_pts);
    run.d_hdr = (int*)(p += b_out);   // {n_busy, n_out, n_kept, pad} then the per-level stats
    return PTAM_OK;
}

int epi_launch_chain(ptam_ctx* ctx, const ptam_kf* src, const double src_pose[12], const ptam_kf* target, const double target_pose[12],
                     const ptam_epipolar_opts* opts, const EpiRun& run) {
    EpiBusy* d_busy = run.d_busy;
    EpiCand* d_kept = (EpiCand*)run.d_kept;
    int* d_hdr = run.d_hdr;
    ptam_epipolar_level_stats* d_stats = (ptam_epipolar_level_stats*)(d_hdr + 4);
    EpiArgs a;
    a.cam = ctx->cam;
    for (int i = 0; i < 9; i++) a.Rs[i] = src_pose[i], a.Rt[i] = target_pose[i];
    for (int i = 0; i < 3; i++) a.ts[i] = src_pose[9 + i], a.tt[i] = target_pose[9 + i];
    a.depth_mean = opts->depth_mean;
    a.depth_sigma = opts->depth_sigma;
    a.wiggle = opts->wiggle_scale;
    a.its = opts->subpix_max_its;
    for (int i = 0; i < run.nl; i++) {
        const int lev = opts->levels[i];
        hipLaunchKernelGGL(epi_select_kernel, dim3(1), dim3(1024), 0, ctx->stream, src->L, lev, opts->min_shi_tomasi, (const EpiBusy*)d_busy,
                           (const int*)d_hdr, d_kept, d_hdr + 2, d_stats + i);
        if (run.n_max[i] > 0)
            hipLaunchKernelGGL(epi_point_kernel, dim3((run.n_max[i] + 3) / 4), dim3(256), 0, ctx->stream, a, src->L, target->L, lev,
                               (const double2*)target->implane[lev], (const EpiCand*)d_kept, (const int*)(d_hdr + 2), run.d_status, run.d_pts);
        hipLaunchKernelGGL(epi_emit_kernel, dim3(1), dim3(1024), 0, ctx->stream, lev, (const int*)(d_hdr + 2), (const int*)run.d_status,
                           (const ptam_new_map_point*)run.d_pts, run.d_out, d_hdr + 1, d_busy, d_hdr, d_stats + i);
        HIP_TRY(hipGetLastError());
    }
    return PTAM_OK;
}

void mapmaker_preload_kernels() {
    ptam_preload((const void*)epi_select_kernel);
    ptam_preload((const void*)epi_point_kernel);
    ptam_preload((const void*)epi_emit_kernel);
}
