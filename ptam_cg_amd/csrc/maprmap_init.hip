// maprmap_init.hip — the first map, made in the resident map (rmap_internal.h):
//   ptam_rmap_init_from_stereo   MapMaker::InitFromStereo (src/MapMaker.cc:268-405) as one call: the match table and the homography
//                                (trails.hip, homography.hip), the point loop's kernel (trails.hip) with its made records compacted in
//                                match order (mt_made_records_core, maptables.hip), the bundles and their outlier routing
//                                (ptam_rmap_bundle_adjust / ptam_rmap_apply_outliers), the scene depth, the epipolar points
//                                (rm_epipolar_points, maprmap_keyframe.hip), the convergence loop and the plane alignment
//   ptam_rmap_align_to_plane     ApplyGlobalTransformationToMap(CalcPlaneAligner()) (:397) on the resident tables: the plane kernels of
//                                mapalign.hip on the resident points, the apply kernel reading the aligner from device memory
//   ptam_rmap_clear              MapMaker::Reset (:37-43) for the tables
// Stages 1-3 of the first call work in the context's scratch (and, for a host match table, in a buffer of the handle's own): the live
// tables are first written when stage 3's count has come down and nothing can refuse the call any more.
// The one kernel here packs the point rows' pixel vectors for the caller that asks for them; it waits for no other workgroup.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rmap_internal.h"
#include "homography.h"
#include "mapmaker_internal.h"
#include "trails_internal.h"

#pragma clang fp contract(off)   // stage 2 is the reference's arithmetic, operation by operation

namespace {

// the point rows' pixel vectors into a packed table
__global__ void __launch_bounds__(256) rm_init_pack_pvs_kernel(int n, const ptam_map_refind_point* __restrict__ rows, ptam_pvs_point* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = rows[i].pv;
}

const double RM_IDENTITY[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

void rm_clear(ptam_rmap* m) {
    for (int i = 0; i < RM_N_COUNTS; i++) m->n[i] = 0;
    m->kfs.clear();
    m->h_poses.clear();
    m->h_fixed.clear();
    m->kf_epoch++;   // (index 0 names another keyframe from now on)
}

bool rm_kf_usable(const ptam_ctx* ctx, const ptam_kf* k) {
    return k && k->device == ctx->device && k->L.w[0] == ctx->params.width && k->L.h[0] == ctx->params.height;
}

// the body of ptam_rmap_align_to_plane; options checked by the caller
int rm_align_to_plane(ptam_rmap* m, const ptam_plane_opts* o, double se3_aligner[12], ptam_plane_info* info, ptam_pvs_point* out_rows) {
    const int K = m->n[RM_N_KF], N = m->n[RM_N_POINTS];
    MapPlaneWork w;
    char* h_still;
    ptam_pvs_point* packed;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        map_plane_layout(c, pin, N, o->trials, w);
        packed = c.piece<ptam_pvs_point>(out_rows ? (size_t)N : 0);
        h_still = pin.piece<char>(256);
    }));
    STAGE_TRY(map_plane_core(s, w, o, N, rm_points3(m)));
    m->d2h += 256;   // (the record: written by the kernel into host-mapped memory)
    // the poses into the second buffer, the points in place, the pixel vectors into the point rows: all of it decided by the status
    // the apply kernel reads in device memory
    if (K + N > 0)
        STAGE_TRY(map_apply_core(s, w.d_record, K, rm_poses(m), rm_poses_alt(m), N, rm_points3(m), rm_sources(m), (ptam_pvs_point*)rm_points(m),
                                 (int)sizeof(ptam_map_refind_point)));
    HIP_TRY(ptam_stream_wait(s.st));
    map_plane_result(w, info, se3_aligner);
    if (K + N > 0) {
        if (info->status == PTAM_PLANE_DEGENERATE) {   // nothing was written: the pixel vectors against the poses as they stand
            STAGE_TRY(map_record_up(s, w.d_record, h_still, PTAM_PLANE_TOO_FEW, RM_IDENTITY));
            STAGE_TRY(map_apply_core(s, w.d_record, K, rm_poses(m), rm_poses_alt(m), N, rm_points3(m), rm_sources(m),
                                     (ptam_pvs_point*)rm_points(m), (int)sizeof(ptam_map_refind_point)));
        }
        STAGE_TRY(s.down(m->h_poses.data(), rm_poses_alt(m), (size_t)K * 96));   // the mirror
        if (out_rows && N > 0) {
            hipLaunchKernelGGL(rm_init_pack_pvs_kernel, dim3(s.blocks(N)), dim3(256), 0, s.st, N, rm_points(m), packed);
            HIP_TRY(hipGetLastError());
            STAGE_TRY(s.down(out_rows, packed, (size_t)N * sizeof(ptam_pvs_point)));
        }
        HIP_TRY(ptam_stream_wait(s.st));
        m->t[PTAM_RMAP_KF_POSES].cur ^= 1;
    }
    return PTAM_OK;
}

// the level list as ptam_add_map_points_epipolar refuses it (the keyframe's MakeKeyFrame_Rest is this call's own to run)
int rm_init_check_levels(const ptam_epipolar_opts* e) {
    ARG_TRY(e->n_levels >= 1 && e->n_levels <= PTAM_LEVELS);
    for (int i = 0; i < e->n_levels; i++) {
        ARG_TRY(e->levels[i] >= 0 && e->levels[i] < PTAM_LEVELS);
        for (int j = 0; j < i; j++) ARG_TRY(e->levels[i] != e->levels[j]);
    }
    return PTAM_OK;
}

// a host match table's place on the device: the trails, then their matches
int rm_init_room(ptam_rmap* m, int n, ptam_trail** d_trails, ptam_homography_match** d_matches) {
    const size_t b_tr = ((size_t)n * sizeof(ptam_trail) + 255) & ~(size_t)255, need = b_tr + (size_t)n * sizeof(ptam_homography_match);
    if (need > m->d_init_bytes) {
        HIP_TRY(ptam_stream_wait(m->ctx->stream));   // (nothing queued reads the old buffer any more)
        if (m->d_init) HIP_TRY(hipFree(m->d_init));
        m->d_init = nullptr;
        m->d_init_bytes = 0;
        const size_t cap = std::max(need, (size_t)65536);
        if (hipMalloc(&m->d_init, cap) != hipSuccess) {
            m->d_init = nullptr;
            ptam_set_error("ptam_rmap_init_from_stereo: no device memory for %d matches", n);
            return PTAM_E_HIP;
        }
        m->d_init_bytes = cap;
    }
    *d_trails = (ptam_trail*)m->d_init;
    *d_matches = (ptam_homography_match*)((char*)m->d_init + b_tr);
    return PTAM_OK;
}

// stages 4-8, on the map as stage 3 left it; n_kf0: the rows of keyframe 0 in the measurement table
int rm_init_finish(ptam_rmap* m, ptam_kf* second, const ptam_rmap_init_opts* opts, const volatile unsigned char* stop_flag, int n_kf0,
                   ptam_rmap_init_result& r) {
    std::vector<ptam_map_outlier> outl;
    // BundleAdjustAll() with the outlier routing of :916-932
    auto bundle = [&](const volatile unsigned char* abort_flag) -> int {
        outl.resize((size_t)std::max(m->n[RM_N_MEAS], 1));
        ptam_map_ba_result br;
        if (int rc = ptam_rmap_bundle_adjust(m, &opts->ba, PTAM_MAP_BA_ALL, abort_flag, &br, outl.data(), (int)outl.size(), nullptr, nullptr)) return rc;
        r.n_bundles++;
        r.n_accepted += br.accepted > 0 ? 1 : 0;
        r.n_outliers += br.n_outliers;
        r.converged = br.converged;
        if (br.n_outliers > 0) {
            r.n_outlier_bundles++;
            for (int i = 0; i < br.n_outliers; i++)   // (a row leaves the table with these two actions)
                if (outl[(size_t)i].kf == 0 && outl[(size_t)i].action != PTAM_MAP_OUT_POINT_BAD) n_kf0--;
            ptam_map_outliers_result orr;
            if (int rc = ptam_rmap_apply_outliers(m, br.n_outliers, outl.data(), &orr)) return rc;
        }
        return PTAM_OK;
    };
    // ---- (4) :374-375
    for (int i = 0; i < opts->first_bundles; i++)
        if (int rc = bundle(nullptr)) return rc;
    // ---- (5) :378-380
    if (int rc = ptam_rmap_scene_depth(m, r.depth)) return rc;
    r.wiggle_scale_depth_normalized = opts->wiggle_scale / r.depth[0].depth_mean;
    // ---- (6) :382-385: kSrc = the newest keyframe = second, kTarget = its closest = first
    ptam_epipolar_opts epi = opts->epipolar;
    epi.depth_mean = r.depth[1].depth_mean;
    epi.depth_sigma = r.depth[1].depth_sigma;
    if (int rc = epi_check(second, &epi)) return rc;
    EpiRun run = {};
    if (int rc = epi_sizes(m->ctx, second, &epi, run)) return rc;
    ARG_TRY((long long)m->n[RM_N_POINTS] + run.sum < (1ll << 31) && (long long)m->n[RM_N_MEAS] + 2ll * run.sum < (1ll << 31));
    r.first_epipolar_point = m->n[RM_N_POINTS];
    if (n_kf0 < 0 || n_kf0 > m->n[RM_N_MEAS]) {
        ptam_set_error("ptam_rmap_init_from_stereo: %d rows of keyframe 0 among %d", n_kf0, m->n[RM_N_MEAS]);
        return PTAM_E_STATE;
    }
    if (int rc = rm_epipolar_points(m, 1, second, m->h_poses.data() + 12, 0, &epi, run, n_kf0, m->n[RM_N_MEAS] - n_kf0, &r.n_epipolar, r.levels))
        return rc;
    // ---- (7) :387-394
    r.converged = 0;
    bool stopped = false;
    for (int done = 1;; done++) {
        if (int rc = bundle(stop_flag)) return rc;
        if (stop_flag && *stop_flag) {
            stopped = true;
            break;
        }
        if (r.converged) break;
        if (opts->max_bundles > 0 && done >= opts->max_bundles) {
            stopped = true;
            break;
        }
    }
    if (stopped) {   // Reset() after `return false`
        rm_clear(m);
        r.status = PTAM_INIT_MAP_STOPPED;
        return PTAM_OK;
    }
    // ---- (8) :397
    if (int rc = rm_align_to_plane(m, &opts->plane, r.se3_aligner, &r.plane, nullptr)) return rc;
    std::copy(m->h_poses.begin() + 12, m->h_poses.begin() + 24, r.tracker_pose);   // :400
    r.status = PTAM_INIT_MAP_OK;
    return PTAM_OK;
}

}   // namespace

extern "C" {

int ptam_rmap_init_opts_default(ptam_rmap_init_opts* o) {
    ARG_TRY(o);
    std::memset(o, 0, sizeof *o);
    ptam_homography_opts_default(&o->homography);
    o->wiggle_scale = 0.1;
    o->subpix_max_its = 10;
    o->first_bundles = 5;
    o->max_bundles = 0;
    ptam_ba_opts_default(&o->ba);
    ptam_epipolar_opts_default(&o->epipolar);
    o->epipolar.n_levels = 4;
    const int32_t levels[4] = {0, 3, 1, 2};   // :382-385
    std::copy(levels, levels + 4, o->epipolar.levels);
    ptam_plane_opts_default(&o->plane);
    return PTAM_OK;
}

int ptam_rmap_clear(ptam_rmap* m) {
    ARG_TRY(m);
    rm_clear(m);
    return PTAM_OK;
}

int ptam_rmap_align_to_plane(ptam_rmap* m, const ptam_plane_opts* opts, double se3_aligner[12], ptam_plane_info* info, ptam_pvs_point* out_rows) {
    ARG_TRY(m && opts && se3_aligner && info);
    if (int rc = map_plane_check(m->n[RM_N_POINTS], opts)) return rc;
    HIP_TRY(hipSetDevice(m->ctx->device));
    return rm_align_to_plane(m, opts, se3_aligner, info, out_rows);
}

int ptam_rmap_init_from_stereo(ptam_rmap* m, const ptam_kf* first, ptam_kf* second, ptam_trails* trails, int n_matches,
                               const ptam_trail* matches, const ptam_rmap_init_opts* opts, const volatile unsigned char* stop_flag,
                               ptam_rmap_init_result* res) {
    // ---- refusals: nothing is enqueued before all of them have passed
    ARG_TRY(m && first && second && opts && res);
    ptam_ctx* ctx = m->ctx;
    ARG_TRY(first != second && rm_kf_usable(ctx, first) && rm_kf_usable(ctx, second));
    TrailsView tv = {};
    int n = n_matches;
    if (trails) {
        trails_view(trails, &tv);
        ARG_TRY(tv.ctx == ctx && tv.w == ctx->params.width && tv.h == ctx->params.height);
        if (!tv.started) {
            ptam_set_error("ptam_rmap_init_from_stereo: no ptam_trails_start yet");
            return PTAM_E_STATE;
        }
        n = tv.n_live;
    } else
        ARG_TRY(matches);
    ARG_TRY(n >= 4);
    if (int rc = homog_check(n, &opts->homography)) return rc;
    ARG_TRY(opts->wiggle_scale > 0.0 && opts->subpix_max_its >= 1 && opts->first_bundles >= 0 && opts->max_bundles >= 0);
    if (int rc = rm_init_check_levels(&opts->epipolar)) return rc;
    if (int rc = map_plane_check(0, &opts->plane)) return rc;
    ARG_TRY(opts->plane.samples == nullptr);
    HIP_TRY(hipSetDevice(ctx->device));
    {   // the bundle's options, as every bundle of the call will be created with them
        ptam_ba* probe = nullptr;
        if (int rc = ptam_ba_create(ctx, &opts->ba, &probe)) return rc;
        ptam_ba_destroy(probe);
    }
    ptam_rmap_init_result r = {};
    r.n_matches = n;
    // ---- :371-372 (what the candidates of stage 6 and the caller's later insertions need)
    if (!first->rest_made)
        if (int rc = ptam_make_keyframe_rest(ctx, const_cast<ptam_kf*>(first))) return rc;
    if (!second->rest_made)
        if (int rc = ptam_make_keyframe_rest(ctx, second)) return rc;
    // ---- (1) :272-287
    const ptam_trail* d_trails = tv.d_trails;
    ptam_homography_match* d_matches = tv.d_out;
    if (!trails) {
        ptam_trail* d_up;
        if (int rc = rm_init_room(m, n, &d_up, &d_matches)) return rc;
        MapStage up = rm_stage(m);
        STAGE_TRY(up.up(d_up, matches, (size_t)n * sizeof(ptam_trail)));   // (pageable: staged before stage 1's wait)
        d_trails = d_up;
    }
    if (int rc = trails_matches_enqueue(ctx, n, d_trails, d_matches)) return rc;
    double se3[12];
    if (int rc = homog_run(ctx, n, d_matches, nullptr, &opts->homography, se3, &r.homography, nullptr)) return rc;
    m->d2h += 256;
    if (n >= 10) m->h2d += (unsigned long long)opts->homography.trials * 16;
    if (r.homography.status != PTAM_HOMOG_OK) {
        r.status = PTAM_INIT_MAP_NO_HOMOGRAPHY;
        *res = r;
        return PTAM_OK;
    }
    // ---- (2) :290-297
    r.baseline = std::sqrt(0.0 + se3[9] * se3[9] + se3[10] * se3[10] + se3[11] * se3[11]);
    if (r.baseline < 1e-6) {
        r.status = PTAM_INIT_MAP_ZERO_BASELINE;
        *res = r;
        return PTAM_OK;
    }
    const double scale = opts->wiggle_scale / r.baseline;
    for (int i = 9; i < 12; i++) se3[i] *= scale;
    // ---- (3) :299-367, in the scratch until the count is known
    int* d_status;
    int *tiles, *hw;
    ptam_new_map_point *d_pts, *d_made;
    MapStage s = rm_stage(m);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_status = c.piece<int>((size_t)n);
        d_pts = c.piece<ptam_new_map_point>((size_t)n);
        d_made = c.piece<ptam_new_map_point>((size_t)n);
        tiles = c.piece<int>((size_t)mt_tiles(n));
        hw = pin.piece<int>(RM_WORDS);
    }));
    if (int rc = rm_words_reset(m)) return rc;
    if (int rc = init_points_enqueue(ctx, first, second, se3, opts->subpix_max_its, n, d_trails, d_status, d_pts)) return rc;
    static_assert(RM_W_TOT + MT_MADE_WORDS <= RM_WORDS, "stage 3's counts fit behind the refusal words");
    if (int rc = mt_made_records_core(s.st, n, d_status, d_pts, d_made, tiles, m->d_words + RM_W_TOT)) return rc;
    if (int rc = rm_words_wait(s, m, hw)) return rc;
    const int* tot = hw + RM_W_TOT;
    r.n_made = tot[1 + PTAM_INIT_MADE];
    r.n_subpix_failed = tot[1 + PTAM_INIT_SUBPIX_FAILED];
    r.n_behind_camera = tot[1 + PTAM_INIT_BEHIND_CAMERA];
    r.n_template_bad = tot[1 + PTAM_INIT_TEMPLATE_BAD];
    if (tot[0] != r.n_made || r.n_made < 0 || r.n_made > n) {
        ptam_set_error("ptam_rmap_init_from_stereo: %d records compacted, %d made, of %d matches", tot[0], r.n_made, n);
        return PTAM_E_STATE;
    }
    if (r.n_made < 3) {   // where assert(nMeas > 2) stands (:1216)
        r.status = PTAM_INIT_MAP_TOO_FEW_POINTS;
        *res = r;
        return PTAM_OK;
    }
    // ---- the new map: two keyframes (first: the identity, fixed; second: se3, free) and no point yet.  From here on the outcomes
    //      are OK and STOPPED; a failure of the device leaves the handle empty.
    rm_clear(m);
    int rc = rm_room(m, PTAM_RMAP_KF_POSES, 2);
    if (!rc) rc = rm_room(m, PTAM_RMAP_KF_FIXED, 2);
    if (!rc) {
        m->h_poses.assign(RM_IDENTITY, RM_IDENTITY + 12);
        m->h_poses.insert(m->h_poses.end(), se3, se3 + 12);
        m->h_fixed = {1, 0};
        m->kfs = {first, second};
        rc = s.up(rm_poses(m), m->h_poses.data(), 192);
    }
    if (!rc) rc = s.up(rm_fixed(m), m->h_fixed.data(), 2);
    if (!rc) {
        m->n[RM_N_KF] = 2;
        rc = rm_add_points_device(m, 0, 1, PTAM_MAP_SRC_TRAIL, r.n_made, d_made);
    }
    // ---- (4)-(8)
    if (!rc) rc = rm_init_finish(m, second, opts, stop_flag, r.n_made, r);
    if (rc) {
        rm_clear(m);
        return rc;
    }
    ptam_rmap_counts(m, &r.counts);
    *res = r;
    return PTAM_OK;
}

}   // extern "C"

void maprmap_init_preload_kernels() { ptam_preload((const void*)rm_init_pack_pvs_kernel); }
