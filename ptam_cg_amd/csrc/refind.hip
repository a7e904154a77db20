// refind.hip — the mapmaker's data association: MapMaker::ReFind_Common (src/MapMaker.cc:943-1020) over the map points of one
// keyframe (ptam_refind_batch) and over a list of (keyframe, point) pairs through one PatchFinder (ptam_refinder_*, ptam_refind_pairs).
#include "refind_internal.h"
#include "patch_device.h"
#include "keyframe_device.h"
#include "pvs_device.h"

// ---- MapMaker::ReFind_Common (src/MapMaker.cc:943-1020), batched over the map points of one keyframe ----
// stage 1: projection + visibility tests (:950-975), derivatives, CalcSearchLevelAndWarpMatrix (:979, verdict unused),
// the template job at the level its loop stopped at, and the search query ir(v2Image), range 4 (:988)
__global__ void __launch_bounds__(256) refind_prep_kernel(DevCam cam, int n, const ptam_pvs_point* __restrict__ pts,
                                                          const TmSrc* __restrict__ src, const double* __restrict__ pose,
                                                          TemplateJob* __restrict__ jobs, ptam_patch_query* __restrict__ q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = pose[k];
    const ptam_pvs_point p = pts[i];
    TemplateJob j;
    j.im = nullptr;
    j.w = j.h = 0;
    j.search_level = -1;
    j.cx = j.cy = 0;
    j.wi[0] = j.wi[1] = j.wi[2] = j.wi[3] = 0;
    ptam_patch_query qq;
    qq.x = qq.y = 0;
    qq.level = -1;
    qq.range = 4;
    double X, Y, Z;
    se3_apply(T, p.world[0], p.world[1], p.world[2], X, Y, Z);
    if (!(Z < 0.001)) {
        const double x = X / Z, y = Y / Z;
        if (!(x * x + y * y > cam.largest_radius * cam.largest_radius)) {
            double u, v, rr, f;
            cam_project(cam, x, y, u, v, rr, f);
            if (!(rr > cam.max_r) && !(u < 0 || v < 0 || u > cam.width || v > cam.height)) {
                double D[4];
                cam_derivs(cam, x, y, rr, f, D);
                double det = pvs_warp_matrix(T, X, Y, Z, D, p, j.wi);
                int l = 0;
                while (det > 3 && l < PTAM_LEVELS - 1) {
                    l++;
                    det *= 0.25;
                }
                const TmSrc sr = src[i];
                j.im = sr.im;
                j.w = sr.w;
                j.h = sr.h;
                j.cx = sr.cx;
                j.cy = sr.cy;
                j.search_level = l;
                qq.x = (int)u;   // ir(): truncation
                qq.y = (int)v;
                qq.level = l;
            }
        }
    }
    jobs[i] = j;
    q[i] = qq;
}
// stage 2: Finder.TemplateBad() (:982-986) takes the point out of the search
__global__ void __launch_bounds__(256) refind_mask_kernel(int n, const ptam_template_result* __restrict__ tres, ptam_patch_query* __restrict__ q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && q[i].level >= 0 && tres[i].bad) q[i].level = -2 - q[i].level;   // (remembers the level for the report)
}
// stage 3: the measurement (:995-1011)
__global__ void __launch_bounds__(256) refind_finish_kernel(int n, const ptam_patch_query* __restrict__ q, const ptam_patch_result* __restrict__ r,
                                                            const ptam_subpix_result* __restrict__ sr, ptam_refind_result* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    ptam_refind_result o;
    const int lv = q[i].level;
    o.found = 0;
    o.level = lv >= 0 ? lv : (lv <= -2 ? -2 - lv : -1);
    o.sub_pix = 0;
    o.never_retry = 1;
    o.root_pos[0] = o.root_pos[1] = 0;
    if (lv >= 0 && r[i].found) {
        o.found = 1;
        o.never_retry = 0;
        if (lv > 0) {   // sub-pixel position whether or not the iteration converged (:1000-1006)
            o.sub_pix = 1;
            o.root_pos[0] = sr[i].pos[0];
            o.root_pos[1] = sr[i].pos[1];
        } else {
            o.root_pos[0] = r[i].pos[0];
            o.root_pos[1] = r[i].pos[1];
        }
    }
    out[i] = o;
}

// ---- ReFind_Common over a list of (keyframe, point) pairs through ONE PatchFinder (src/MapMaker.cc:977, :1046-1082) ----
// The finder's state makes the list a sequence: whether pair i re-makes the template depends on the last pair that did.
// But only inside a RUN of consecutive pairs (of those that reach the finder) with the same map point: another point always
// re-makes it (src/PatchFinder.cc:103).  So: (1) every pair's exits, level, warp and m2 in parallel; (2) one workgroup
// compacts the reaching pairs and walks each run with one thread — which pair re-makes, which template a kept one uses,
// whether a rejected warp has raised mbTemplateBad since; (3) the re-made templates; (4) one wave per pair searches with its
// template; (5) the finder's state after the last pair.
__global__ void __launch_bounds__(256) rp_prep_kernel(DevCam cam, RpDev d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const RpPair& pr = d.pairs[i];
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = pr.pose[k];
    const ptam_pvs_point p = pr.pt;
    TemplateJob j;
    j.im = nullptr;
    j.w = j.h = 0;
    j.search_level = -1;
    j.cx = j.cy = 0;
    j.wi[0] = j.wi[1] = j.wi[2] = j.wi[3] = 0;
    ptam_patch_query qq;
    qq.x = qq.y = 0;
    qq.level = -1;
    qq.range = 4;
    int reach = 0, detbad = 0;
    double m2[4] = {0, 0, 0, 0};
    double X, Y, Z;
    se3_apply(T, p.world[0], p.world[1], p.world[2], X, Y, Z);
    if (!pr.skip && !(Z < 0.001)) {                                                     // :947-955
        const double x = X / Z, y = Y / Z;
        if (!(x * x + y * y > cam.largest_radius * cam.largest_radius)) {               // :957-961
            double u, v, rr, f;
            cam_project(cam, x, y, u, v, rr, f);
            if (!(rr > cam.max_r) && !(u < 0 || v < 0 || u > cam.width || v > cam.height)) {   // :963-975
                double D[4];
                cam_derivs(cam, x, y, rr, f, D);
                double det = pvs_warp_matrix(T, X, Y, Z, D, p, j.wi);
                int l = 0;
                while (det > 3 && l < PTAM_LEVELS - 1) {
                    l++;
                    det *= 0.25;
                }
                detbad = (det > 3 || det < 0.25) ? 1 : 0;                               // src/PatchFinder.cc:78-81
                j.im = pr.src.im;
                j.w = pr.src.w;
                j.h = pr.src.h;
                j.cx = pr.src.cx;
                j.cy = pr.src.cy;
                j.search_level = l;
                template_m2(j, m2);
                qq.x = (int)u;   // ir(): truncation
                qq.y = (int)v;
                qq.level = l;
                reach = 1;
            }
        }
    }
    d.jobs[i] = j;
    d.q[i] = qq;
    d.reach[i] = reach;
    d.detbad[i] = detbad;
#pragma unroll
    for (int k = 0; k < 4; k++) d.m2[4 * i + k] = m2[k];
}
__global__ void __launch_bounds__(1024) rp_scan_kernel(RpDev d) {
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < d.n; b0 += 1024) {   // stable compaction of the reaching pairs
        const int i = b0 + tid;
        const int f = i < d.n ? d.reach[i] : 0;
        const int incl = wave_incl_scan_i32(f);
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        int off = base_s, tot = 0;
        for (int w = 0; w < 16; w++) {
            if (w < wid) off += wsum[w];
            tot += wsum[w];
        }
        if (f) d.R[off + incl - 1] = i;
        __syncthreads();
        if (tid == 0) base_s += tot;
        __syncthreads();
    }
    const int nr = base_s;
    if (tid == 0) *d.nr = nr;
    __threadfence_block();
    __syncthreads();
    const RpFinder st = *d.st;
    const double lim = 0.07 * 0.07;
    for (int k = tid; k < nr; k += 1024) {
        const int i0 = d.R[k];
        const long long id = d.pairs[i0].id;
        const bool head = k == 0 ? !(st.valid && st.pt == id) : d.pairs[d.R[k - 1]].id != id;
        if (!head && k != 0) continue;   // (a run is walked by the thread of its first pair)
        int cur = head ? i0 : -1, acc = 0;
        double l0 = st.m2[0], l1 = st.m2[1], l2 = st.m2[2], l3 = st.m2[3];
        for (int kk = k; kk < nr; kk++) {
            const int i = d.R[kk];
            if (kk > k && d.pairs[i].id != id) break;
            const double* m = d.m2 + 4 * i;
            bool refresh = kk == k && head;
            if (!refresh) {
                const double ax = m[0] - l0, ay = m[2] - l2, bx = m[1] - l1, by = m[3] - l3;   // columns m2.T()[0], m2.T()[1]
                refresh = ax * ax + ay * ay > lim || bx * bx + by * by > lim;
            }
            if (refresh) {
                cur = i;
                l0 = m[0], l1 = m[1], l2 = m[2], l3 = m[3];
                acc = 0;
            } else
                acc |= d.detbad[i];
            d.refresh[i] = refresh;
            d.srcp[i] = cur;
            d.dacc[i] = acc;
        }
    }
}
__global__ void __launch_bounds__(256) rp_template_kernel(RpDev d) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= d.n || !d.reach[i] || !d.refresh[i]) return;
    ptam_template_result tr;
    const int T = wave_make_template(d.jobs[i], lane, tr);
    d.tm[(size_t)i * 64 + lane] = (uint8_t)T;
    if (lane == 0) d.tres[i] = tr;
}
__global__ void __launch_bounds__(256) rp_search_kernel(RpDev d) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= d.n) return;
    ptam_refind_result o;
    o.found = 0;
    o.level = -1;
    o.sub_pix = 0;
    o.never_retry = d.pairs[i].skip ? 0 : 1;
    o.root_pos[0] = o.root_pos[1] = 0;
    int kept = 0;
    if (d.reach[i]) {
        const int src = d.srcp[i], refresh = d.refresh[i];
        const int T = src >= 0 ? d.tm[(size_t)src * 64 + lane] : d.st->tpl[lane];
        const int bad = refresh ? d.tres[i].bad : (((src >= 0 ? d.tres[src].bad : d.st->bad) != 0) || d.dacc[i]);
        kept = !refresh;
        const ptam_patch_query q = d.q[i];
        o.level = q.level;
        if (lane == 0) d.bad[i] = bad;
        const KfLevels& L = d.Ls[d.pairs[i].kf];
        ptam_patch_result res;
        __shared__ __attribute__((aligned(16))) unsigned rp_win[4][SW_BYTES / 4];
        wave_find_patch_coarse(L, q, !bad, T, lane, res, rp_win[threadIdx.x >> 6]);   // :982-988 (range 4)
        if (!bad && res.found) {
            o.found = 1;
            o.never_retry = 0;
            if (q.level > 0) {                                                          // :1000-1006 (convergence is not looked at)
                ptam_subpix_query sq;
                sq.level = q.level;
                sq.max_its = 8;
                sq.coarse_pos[0] = res.pos[0];
                sq.coarse_pos[1] = res.pos[1];
                ptam_subpix_result sres;
                wave_subpix(L, sq, T, lane, sres, (uint8_t*)rp_win[threadIdx.x >> 6]);   // (the search is done with the buffer)
                o.sub_pix = 1;
                o.root_pos[0] = sres.pos[0];
                o.root_pos[1] = sres.pos[1];
            } else {
                o.root_pos[0] = res.pos[0];
                o.root_pos[1] = res.pos[1];
            }
        }
    }
    if (lane == 0) {
        d.out[i] = o;
        d.kept[i] = kept;
    }
}
__global__ void __launch_bounds__(64) rp_state_kernel(RpDev d) {
    const int nr = *d.nr, lane = threadIdx.x;
    if (nr == 0) return;
    const int last = d.R[nr - 1], src = d.srcp[last];
    if (src >= 0) {
        d.st->tpl[lane] = d.tm[(size_t)src * 64 + lane];
        if (lane == 0) {
            d.st->pt = d.pairs[last].id;
            for (int k = 0; k < 4; k++) d.st->m2[k] = d.m2[4 * src + k];
            d.st->valid = 1;
        }
    }
    if (lane == 0) d.st->bad = d.bad[last];
}

static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t rp_carve(RpDev& d, char* b, size_t off, int n) {
    const size_t N = (size_t)n;
    auto take = [&](size_t bytes) {
        char* p = b ? b + off : nullptr;
        off += up256(bytes);
        return p;
    };
    d.jobs = (TemplateJob*)take(N * sizeof(TemplateJob));
    d.q = (ptam_patch_query*)take(N * sizeof(ptam_patch_query));
    d.m2 = (double*)take(N * 32);
    d.reach = (int*)take(N * 4);
    d.detbad = (int*)take(N * 4);
    d.R = (int*)take(N * 4);
    d.nr = (int*)take(4);
    d.refresh = (int*)take(N * 4);
    d.srcp = (int*)take(N * 4);
    d.dacc = (int*)take(N * 4);
    d.bad = (int*)take(N * 4);
    d.tm = (uint8_t*)take(N * 64);
    d.tres = (ptam_template_result*)take(N * sizeof(ptam_template_result));
    d.out = (ptam_refind_result*)take(N * sizeof(ptam_refind_result));
    d.kept = (int*)take(N * 4);
    return off;
}
void rp_launch_chain(hipStream_t st, const DevCam& cam, const RpDev& d) {
    const int n = d.n;
    hipLaunchKernelGGL(rp_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, st, cam, d);
    hipLaunchKernelGGL(rp_scan_kernel, dim3(1), dim3(1024), 0, st, d);
    hipLaunchKernelGGL(rp_template_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d);
    hipLaunchKernelGGL(rp_search_kernel, dim3((n + 3) / 4), dim3(256), 0, st, d);
    hipLaunchKernelGGL(rp_state_kernel, dim3(1), dim3(64), 0, st, d);
}

extern "C" {

int ptam_refind_batch(ptam_ctx* ctx, const ptam_kf* kf, const double kf_pose[12], int n, const ptam_pvs_point* points,
                      const ptam_template_query* sources, ptam_refind_result* out) {
    ARG_TRY(ctx && kf && kf_pose && n >= 0);
    if (n == 0) return PTAM_OK;
    ARG_TRY(points && sources && out);
    ARG_TRY(kf->device == ctx->device);
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<TmSrc> hs((size_t)n);
    for (int i = 0; i < n; i++) {
        const ptam_template_query& q = sources[i];
        ARG_TRY(q.src_kf && q.src_level >= 0 && q.src_level < PTAM_LEVELS && q.src_kf->device == ctx->device);
        hs[(size_t)i].im = q.src_kf->L.im[q.src_level];
        hs[(size_t)i].w = q.src_kf->L.w[q.src_level];
        hs[(size_t)i].h = q.src_kf->L.h[q.src_level];
        hs[(size_t)i].cx = q.center_x;
        hs[(size_t)i].cy = q.center_y;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    };
    const size_t N = (size_t)n;
    const size_t o_pts = take(N * sizeof(ptam_pvs_point)), o_src = take(N * sizeof(TmSrc)), o_pose = take(96),
                 o_jobs = take(N * sizeof(TemplateJob)), o_tm = take(N * 64), o_tr = take(N * sizeof(ptam_template_result)),
                 o_q = take(N * sizeof(ptam_patch_query)), o_r = take(N * sizeof(ptam_patch_result)),
                 o_sr = take(N * sizeof(ptam_subpix_result)), o_out = take(N * sizeof(ptam_refind_result));
    void* s;
    int rc = ctx_scratch(ctx, off, &s);
    if (rc) return rc;
    char* b = (char*)s;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(b + o_pts, points, N * sizeof(ptam_pvs_point), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_src, hs.data(), N * sizeof(TmSrc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_pose, kf_pose, 96, hipMemcpyHostToDevice, st));
    const int g = (n + 255) / 256;
    TemplateJob* d_jobs = (TemplateJob*)(b + o_jobs);
    ptam_patch_query* d_q = (ptam_patch_query*)(b + o_q);
    ptam_patch_result* d_r = (ptam_patch_result*)(b + o_r);
    ptam_subpix_result* d_sr = (ptam_subpix_result*)(b + o_sr);
    ptam_template_result* d_tr = (ptam_template_result*)(b + o_tr);
    uint8_t* d_tm = (uint8_t*)(b + o_tm);
    hipLaunchKernelGGL(refind_prep_kernel, dim3(g), dim3(256), 0, st, ctx->cam, n, (const ptam_pvs_point*)(b + o_pts), (const TmSrc*)(b + o_src),
                       (const double*)(b + o_pose), d_jobs, d_q);
    rc = patch_launch_templates_dev(ctx, n, d_jobs, d_tm, d_tr, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(refind_mask_kernel, dim3(g), dim3(256), 0, st, n, (const ptam_template_result*)d_tr, d_q);
    rc = patch_launch_search_dev(ctx, kf, n, d_q, d_tm, d_r, nullptr, nullptr);
    if (rc) return rc;
    rc = patch_launch_subpix_dev(ctx, kf, n, d_q, d_r, d_tm, d_sr, nullptr, 8);
    if (rc) return rc;
    hipLaunchKernelGGL(refind_finish_kernel, dim3(g), dim3(256), 0, st, n, (const ptam_patch_query*)d_q, (const ptam_patch_result*)d_r,
                       (const ptam_subpix_result*)d_sr, (ptam_refind_result*)(b + o_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, b + o_out, N * sizeof(ptam_refind_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));   // (also keeps hs[] alive until its pageable copy has been staged)
    return PTAM_OK;
}

int ptam_refinder_create(ptam_ctx* ctx, ptam_refinder** out) {
    ARG_TRY(ctx && out);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_refinder* f = new ptam_refinder();
    f->ctx = ctx;
    if (hipMalloc((void**)&f->st, sizeof(RpFinder)) != hipSuccess || hipMemset(f->st, 0, sizeof(RpFinder)) != hipSuccess) {
        if (f->st) hipFree(f->st);
        delete f;
        ptam_set_error("ptam_refinder_create: allocation failed");
        return PTAM_E_HIP;
    }
    *out = f;
    return PTAM_OK;
}
int ptam_refinder_destroy(ptam_refinder* f) {
    if (!f) return PTAM_OK;
    hipSetDevice(f->ctx->device);
    ptam_stream_wait(f->ctx->stream);
    hipFree(f->st);
    delete f;
    return PTAM_OK;
}
int ptam_refind_pairs(ptam_ctx* ctx, ptam_refinder* finder, int n, const ptam_refind_pair* pairs, ptam_refind_result* out,
                      int32_t* template_kept) {
    ARG_TRY(ctx && finder && finder->ctx->device == ctx->device && n >= 0);
    if (n == 0) return PTAM_OK;
    ARG_TRY(pairs && out);
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<RpPair> hp((size_t)n);
    std::vector<KfLevels> hl;
    std::vector<const ptam_kf*> seen;
    for (int i = 0; i < n; i++) {
        const ptam_refind_pair& p = pairs[i];
        const ptam_template_query& q = p.source;
        ARG_TRY(p.kf && p.kf->device == ctx->device);
        ARG_TRY(q.src_kf && q.src_level >= 0 && q.src_level < PTAM_LEVELS && q.src_kf->device == ctx->device);
        RpPair& r = hp[(size_t)i];
        r.pt = p.point;
        r.src.im = q.src_kf->L.im[q.src_level];
        r.src.w = q.src_kf->L.w[q.src_level];
        r.src.h = q.src_kf->L.h[q.src_level];
        r.src.cx = q.center_x;
        r.src.cy = q.center_y;
        std::memcpy(r.pose, p.kf_pose, 96);
        r.id = (long long)p.point_id;
        r.skip = p.skip != 0;
        int k = -1;   // (lists name few keyframes, mostly in runs: a linear search from the back finds the last one at once)
        for (int s = (int)seen.size() - 1; s >= 0; s--)
            if (seen[(size_t)s] == p.kf) {
                k = s;
                break;
            }
        if (k < 0) {
            k = (int)seen.size();
            seen.push_back(p.kf);
            hl.push_back(p.kf->L);
        }
        r.kf = k;
    }
    const size_t N = (size_t)n;
    const size_t o_pairs = 0, o_ls = up256(N * sizeof(RpPair)), o_work = o_ls + up256(hl.size() * sizeof(KfLevels));
    RpDev d;
    void* sc;
    int rc = ctx_scratch(ctx, rp_carve(d, nullptr, o_work, n), &sc);
    if (rc) return rc;
    char* b = (char*)sc;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(b + o_pairs, hp.data(), N * sizeof(RpPair), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b + o_ls, hl.data(), hl.size() * sizeof(KfLevels), hipMemcpyHostToDevice, st));
    rp_carve(d, b, o_work, n);
    d.n = n;
    d.pairs = (const RpPair*)(b + o_pairs);
    d.Ls = (const KfLevels*)(b + o_ls);
    d.st = finder->st;
    rp_launch_chain(st, ctx->cam, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d.out, N * sizeof(ptam_refind_result), hipMemcpyDeviceToHost, st));
    if (template_kept) HIP_TRY(hipMemcpyAsync(template_kept, d.kept, N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));   // (also keeps the staging vectors alive until their pageable copies have been staged)
    return PTAM_OK;
}

}   // extern "C"

void refind_preload_kernels() {
    ptam_preload((const void*)refind_prep_kernel);
    ptam_preload((const void*)refind_mask_kernel);
    ptam_preload((const void*)refind_finish_kernel);
    ptam_preload((const void*)rp_prep_kernel);
    ptam_preload((const void*)rp_scan_kernel);
    ptam_preload((const void*)rp_template_kernel);
    ptam_preload((const void*)rp_search_kernel);
    ptam_preload((const void*)rp_state_kernel);
}
