// sbi.hip — the SmallBlurryImage (src/ImageProcess.cc:255-495) on the device: MakeFromKF + MakeJacs, the ESM aligner
// IteratePosRelToTarget with SE3fromSE2, the relocaliser's nearest-keyframe search (src/Relocaliser.cc:12-38) and the tracker's
// per-frame pair (src/Tracker.cc:94-108).  An SBI is 1 200 pixels at 640x480: everything here is one workgroup per image and is
// bounded by launches, so a make is one launch, an alignment (all iterations, the arg-min over a bank, SE3fromSE2, the result into
// host-mapped memory) is one launch, and the bank's SSDs are one launch.  The libCVD rules (halfSample, transform / sample,
// convolveGaussian) are the project's own restatement: ptam_hip.h, "SmallBlurryImage".
#include "sbi.h"

#include "keyframe_device.h"   // half4: the pyramid's halfSample
#include "patch_device.h"      // nc_*: products and sums that are never contracted; cam_unproject
#include "wait_mapped.h"
#include "snapshot_internal.h"   // the keyframe section of a ptam_map_snapshot
#include "motion_device.h"     // the prediction behind SE3fromSE2 (a batch's frames)

#define SBI_THREADS 256
#define SBI_MAX_PIXELS 4096    // LDS: make 48 KB (f32 template + f64 row pass), align 32 KB (template + warped image)
#define SBI_MAX_SIDE 256
#define SBI_MAX_TAPS 15        // ceil(3 sigma), sigma <= 5
#define SBI_MAX_ITERATIONS 64

// ---- make: MakeFromKF (:279-304) + MakeJacs (:170-191) ----------------------------------------------------------------------
struct SbiMakeArgs {
    const uint8_t* l3;   // aLevels[3].im; or, for a grid of several images:
    const uint8_t* const* l3_list;   // image b's level 3 (device array, nullable); its outputs follow b images further on
    const SbiBatchRec* recs;         // or (nullable) a record per image: its level 3 and its own three output arrays
    int w3, w, h, k;     // level-3 row pitch; the SBI's size; taps each side
    uint8_t* small;      // mimSmall
    float* tmpl;         // mimTemplate
    float* jacs;         // mimImageJacs: (x, y) per pixel
    double wt[2 * SBI_MAX_TAPS + 1];
};

template <int VARIANT>
__global__ __launch_bounds__(SBI_THREADS) void sbi_make_kernel(SbiMakeArgs a) {
    __shared__ float s_t[SBI_MAX_PIXELS];
    __shared__ double s_h[SBI_MAX_PIXELS];
    __shared__ unsigned s_sum[SBI_THREADS / 64];
    const int tid = threadIdx.x, n = a.w * a.h;
    const SbiBatchRec* rec = a.recs ? a.recs + blockIdx.x : nullptr;
    const uint8_t* __restrict__ l3 = rec ? rec->l3 : a.l3_list ? a.l3_list[blockIdx.x] : a.l3;
    uint8_t* __restrict__ o_small = rec ? rec->small : a.small + (size_t)blockIdx.x * n;
    float* __restrict__ o_tmpl = rec ? rec->tmpl : a.tmpl + (size_t)blockIdx.x * n;
    float* __restrict__ o_jacs = rec ? rec->jacs : a.jacs + (size_t)blockIdx.x * 2 * n;
    unsigned sum = 0;   // (exact: at most 4096 * 255)
    for (int i = tid; i < n; i += SBI_THREADS) {
        const int x = i % a.w, y = i / a.w;
        const uint8_t* p = l3 + (size_t)(2 * y) * a.w3 + 2 * x;
        const int v = half4<VARIANT>(p[0], p[1], p[a.w3], p[a.w3 + 1]);
        o_small[i] = (uint8_t)v;
        s_t[i] = (float)v;
        sum += v;
    }
    sum = (unsigned)wave_sum_i32((int)sum);
    if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    unsigned total = 0;
    for (int i = 0; i < SBI_THREADS / 64; i++) total += s_sum[i];
    const float mean = (float)total / (float)n;   // fMean = ((float) nSum) / mirSize.area()
    for (int i = tid; i < n; i += SBI_THREADS) s_t[i] = s_t[i] - mean;
    __syncthreads();
    // convolveGaussian: rows, then columns, fp64 in between, taps in ascending order; outside the image counts as 0
    for (int i = tid; i < n; i += SBI_THREADS) {
        const int x = i % a.w, y = i / a.w;
        double acc = 0.0;
        for (int j = -a.k; j <= a.k; j++)
            if (x + j >= 0 && x + j < a.w) acc = nc_add(acc, nc_mul(a.wt[j + a.k], (double)s_t[y * a.w + x + j]));
        s_h[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < n; i += SBI_THREADS) {
        const int x = i % a.w, y = i / a.w;
        double acc = 0.0;
        for (int j = -a.k; j <= a.k; j++)
            if (y + j >= 0 && y + j < a.h) acc = nc_add(acc, nc_mul(a.wt[j + a.k], s_h[(y + j) * a.w + x]));
        const float t = (float)acc;
        s_t[i] = t;   // (the row pass no longer reads s_t: every thread is past the barrier above)
        o_tmpl[i] = t;
    }
    __syncthreads();
    for (int i = tid; i < n; i += SBI_THREADS) {
        const int x = i % a.w, y = i / a.w;
        float gx = 0.f, gy = 0.f;
        if (x >= 1 && y >= 1 && x < a.w - 1 && y < a.h - 1) {   // in_image_with_border(ir, 1); the 0.5 is left out, as there
            gx = s_t[i + 1] - s_t[i - 1];
            gy = s_t[i + a.w] - s_t[i - a.w];
        }
        o_jacs[2 * i] = gx;
        o_jacs[2 * i + 1] = gy;
    }
}

// ---- the bank's SSDofImgs (:88-105): one workgroup per keyframe ------------------------------------------------------------------
__global__ __launch_bounds__(SBI_THREADS) void sbi_ssd_kernel(const float* __restrict__ cur, const float* __restrict__ bank, int n,
                                                             double* __restrict__ ssd, double* __restrict__ h_ssd) {
    __shared__ double s_part[SBI_THREADS / 64];
    const float* b = bank + (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += SBI_THREADS) {
        const double d = (double)(cur[i] - b[i]);   // the difference in float, its square and the sum in double
        acc = nc_add(acc, nc_mul(d, d));
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_part[0];
        for (int i = 1; i < SBI_THREADS / 64; i++) s += s_part[i];
        ssd[blockIdx.x] = s;
        if (h_ssd) h_ssd[blockIdx.x] = s;   // (host-mapped; the align kernel's sequence word, later on the same queue, covers it)
    }
}
// ... for a batch's recovering cameras: row y is camera y's image against its own bank, into its own table; the sums are sbi_ssd_kernel's
__global__ __launch_bounds__(SBI_THREADS) void sbi_ssd_batch_kernel(const SbiRelocRec* __restrict__ recs, int n) {
    __shared__ double s_part[SBI_THREADS / 64];
    const SbiRelocRec& r = recs[blockIdx.y];
    if ((int)blockIdx.x >= r.count) return;
    const float* __restrict__ cur = r.cur;
    const float* __restrict__ b = r.bank_tmpl + (size_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += SBI_THREADS) {
        const double d = (double)(cur[i] - b[i]);
        acc = nc_add(acc, nc_mul(d, d));
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = s_part[0];
        for (int i = 1; i < SBI_THREADS / 64; i++) s += s_part[i];
        r.ssd[blockIdx.x] = s;
    }
}

// ---- ptam_sbi_bank_take_keyframes ----
// the take's device side in one launch: entries [first, n_kf) of the three image arrays (one thread per pixel: 1 + 4 + 8 bytes)
// and the pose table [0, n_kf) (one thread per double), from a slot's section into a bank
struct SbiTakeArgs {
    const uint8_t* s_small;
    const float* s_tmpl;
    const float2* s_jacs;
    const double* s_poses;
    uint8_t* d_small;
    float* d_tmpl;
    float2* d_jacs;
    double* d_poses;
    long long px_first, px_count;   // the pixels [px_first, px_first + px_count) of the arrays
    int n_pose;                     // 12 n_kf
};
__global__ __launch_bounds__(256) void sbi_take_kernel(SbiTakeArgs a) {
    const long long stride = (long long)gridDim.x * 256;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long i = t; i < a.px_count; i += stride) {
        const long long p = a.px_first + i;
        a.d_small[p] = a.s_small[p];
        a.d_tmpl[p] = a.s_tmpl[p];
        a.d_jacs[p] = a.s_jacs[p];
    }
    for (long long i = t; i < a.n_pose; i += stride) a.d_poses[i] = a.s_poses[i];
}

// ---- align: IteratePosRelToTarget (:313-417) + SE3fromSE2 (:427-476) --------------------------------------------------------
struct SbiOut {   // host-mapped
    ptam_sbi_alignment a;
    int32_t best, pad_;
    double best_ssd;
    unsigned long long seq;
};
struct SbiAlignArgs {
    const float* cur;         // this image's mimTemplate
    const float* tgt_tmpl;    // the target's mimTemplate / mimImageJacs; with a bank: entry 0's
    const float* tgt_jacs;
    const double* ssd;        // bank: the SSD of every entry (the target is the first strictly smallest); else null
    int count;
    int w, h, iterations;
    DevCam cam;               // the camera at the SBI's size (camera.SetImageSize(mirSize), :429)
    SbiOut* out;
    unsigned long long seq;
    // a batch's frames (nullable): workgroup b aligns record b's image against record b's target, then predicts the frame's pose;
    // cur, tgt_*, ssd, out and seq are not used
    const SbiBatchRec* recs;
    // ... with, in the same launch, the FAST detection of the batch's keyframes (det_items nullable): it needs the pyramid only, as the
    // images do, so its workgroups — behind the n_align align workgroups, det_blocks per keyframe, keyframe f's KfLevels at
    // det_items + f * det_stride + det_off — fill the chip while the align workgroups walk their ~100 us of serial chain
    const char* det_items;
    size_t det_stride, det_off;
    int det_blocks, n_align;
    // ... and (rrecs nullable) the relocaliser of the batch's recovering cameras: workgroups n_est .. n_align - 1, one per record — the
    // arg-min over the camera's SSD table, the alignment against that entry, then mse3Best, `good` and the frame's gate
    const SbiRelocRec* rrecs;
    int n_est;
};

// TooN Cholesky<N> (L D L^T, the scaled column cached in the upper half) + backsub.  false: a pivot that is not strictly positive.
template <int N>
__device__ bool sbi_ldlt_solve(double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
    for (int col = 0; col < N; col++) {
        double inv_diag = 1.0;
        for (int row = col; row < N; row++) {
            double val = A[row][col];
            for (int c2 = 0; c2 < col; c2++) val -= A[c2][col] * A[row][c2];
            if (row == col) {
                if (!(val > 0.0)) return false;
                A[row][col] = val;
                inv_diag = 1.0 / val;
            } else {
                A[col][row] = val;
                A[row][col] = val * inv_diag;
            }
        }
    }
    double y[N];
    for (int i = 0; i < N; i++) {
        double val = b[i];
        for (int j = 0; j < i; j++) val -= A[i][j] * y[j];
        y[i] = val;
    }
    for (int i = 0; i < N; i++) y[i] /= A[i][i];
    for (int i = N - 1; i >= 0; i--) {
        double val = y[i];
        for (int j = i + 1; j < N; j++) val -= A[j][i] * x[j];
        x[i] = val;
    }
    return true;
}

// SE3fromSE2: two points five pixels either side of the centre, warped by the SE2, and three Gauss-Newton steps of an SO3 onto them.
// An SE2 that is exactly the identity gives exactly the identity (the reference's three steps leave ~1e-17 of Project(UnProject())).
__device__ void sbi_se3_from_se2(const DevCam& c, int w, int h, const double R2[4], const double t2[2], double Rm[9]) {
    for (int i = 0; i < 9; i++) Rm[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (R2[0] == 1.0 && R2[1] == 0.0 && R2[2] == 0.0 && R2[3] == 1.0 && t2[0] == 0.0 && t2[1] == 0.0) return;
    const double ccx = (double)(w / 2), ccy = (double)(h / 2);
    double turned[2][2], orig[2][3];
    for (int i = 0; i < 2; i++) {
        const double vx = i ? -5.0 : 5.0;
        turned[i][0] = ccx + ((R2[0] * vx + R2[1] * 0.0) + t2[0]);
        turned[i][1] = ccy + ((R2[2] * vx + R2[3] * 0.0) + t2[1]);
        cam_unproject(c, ccx + vx, ccy, orig[i][0], orig[i][1]);
        orig[i][2] = 1.0;
    }
    for (int it = 0; it < 3; it++) {
        double C[3][3] = {{10.0, 0, 0}, {0, 10.0, 0}, {0, 0, 10.0}}, v[3] = {0, 0, 0};   // wls.add_prior(10.0)
        for (int i = 0; i < 2; i++) {
            double cam[3];
            for (int r = 0; r < 3; r++) cam[r] = Rm[3 * r] * orig[i][0] + Rm[3 * r + 1] * orig[i][1] + Rm[3 * r + 2] * orig[i][2];
            const double x = cam[0] / cam[2], y = cam[1] / cam[2];
            double u, vv, rr, f, D[4];
            cam_project(c, x, y, u, vv, rr, f);
            cam_derivs(c, x, y, rr, f, D);
            const double err[2] = {turned[i][0] - u, turned[i][1] - vv};
            const double ooz = 1.0 / cam[2];
            const double mot[3][3] = {{0.0, -cam[2], cam[1]}, {cam[2], 0.0, -cam[0]}, {-cam[1], cam[0], 0.0}};   // SO3<>::generator_field
            double J[2][3];
            for (int m = 0; m < 3; m++) {
                const double f0 = (mot[m][0] - cam[0] * mot[m][2] * ooz) * ooz, f1 = (mot[m][1] - cam[1] * mot[m][2] * ooz) * ooz;
                J[0][m] = D[0] * f0 + D[1] * f1;
                J[1][m] = D[2] * f0 + D[3] * f1;
            }
            for (int k = 0; k < 2; k++)
                for (int r = 0; r < 3; r++) {
                    for (int cc = 0; cc < 3; cc++) C[r][cc] += J[k][r] * J[k][cc];
                    v[r] += err[k] * J[k][r];
                }
        }
        double mu[3];
        if (!sbi_ldlt_solve<3>(C, v, mu)) return;   // (cannot happen: the prior makes the matrix positive definite)
        const double mu6[6] = {0, 0, 0, mu[0], mu[1], mu[2]};
        double E[9], et[3], P[9];
        se3_exp_parts<false>(mu6, E, et);
        for (int r = 0; r < 3; r++)
            for (int cc = 0; cc < 3; cc++) P[3 * r + cc] = E[3 * r] * Rm[cc] + E[3 * r + 1] * Rm[3 + cc] + E[3 * r + 2] * Rm[6 + cc];
        for (int i = 0; i < 9; i++) Rm[i] = P[i];
    }
}

// n steps of CVD::transform's walk: p += across, one rounded addition per step like the reference's loop.  The whole of an image's
// rows is one dependent chain (1 230 steps at 40x30, walked by one thread per iteration): eight steps per branch, because a taken
// branch costs more than the two additions of a step.
__device__ __forceinline__ void sbi_walk(double& px, double& py, double ax, double ay, int n) {
    int i = 0;
    for (; i + 8 <= n; i += 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            px = nc_add(px, ax);
            py = nc_add(py, ay);
        }
    }
    for (; i < n; i++) {
        px = nc_add(px, ax);
        py = nc_add(py, ay);
    }
}

struct SbiWalk {   // CVD::transform's walk for one iteration, made by thread 0
    double ax, ay;            // across = M.T()[0]
    double mean_offset;       // dMeanOffset
    int all_inside, stop;
};

__global__ __launch_bounds__(SBI_THREADS) void sbi_align_kernel(SbiAlignArgs g) {
    __shared__ float s_cur[SBI_MAX_PIXELS], s_warp[SBI_MAX_PIXELS];
    __shared__ double s_rowx[SBI_MAX_SIDE], s_rowy[SBI_MAX_SIDE];
    __shared__ double s_red[SBI_THREADS / 64][16];
    __shared__ int s_cnt[SBI_THREADS / 64];
    __shared__ SbiWalk s_walk;
    __shared__ double s_bv[SBI_THREADS];
    __shared__ int s_bi[SBI_THREADS];
    if (g.det_items && (int)blockIdx.x >= g.n_align) {
        const int d = (int)blockIdx.x - g.n_align;
        fast_detect_tall_body<FAST_BATCH_TH>(*(const KfLevels*)(g.det_items + (size_t)(d / g.det_blocks) * g.det_stride + g.det_off), d % g.det_blocks);
        return;
    }
    const int tid = threadIdx.x, w = g.w, h = g.h, n = w * h;
    // the relocaliser's nearest keyframe: the first strictly smallest SSD (src/Relocaliser.cc:21-31) = the smallest value, and among
    // equal values the lowest index.  Each thread scans every 256th entry in ascending order, then a tree over the workgroup.
    int best = -1;
    double best_ssd = 0.0;
    const SbiRelocRec* rr = g.rrecs && (int)blockIdx.x >= g.n_est ? g.rrecs + ((int)blockIdx.x - g.n_est) : nullptr;
    const double* __restrict__ ssd_tab = g.ssd;
    int count = g.count;
    if (rr) ssd_tab = rr->ssd, count = rr->count;
    if (ssd_tab) {
        double bv = INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < count; i += SBI_THREADS) {
            const double v = ssd_tab[i];
            if (v < bv) bv = v, bi = i;
        }
        s_bv[tid] = bv;
        s_bi[tid] = bi;
        __syncthreads();
        for (int half = SBI_THREADS / 2; half >= 1; half >>= 1) {
            if (tid < half) {
                const double v = s_bv[tid + half];
                const int i = s_bi[tid + half];
                if (v < s_bv[tid] || (v == s_bv[tid] && i < s_bi[tid])) s_bv[tid] = v, s_bi[tid] = i;
            }
            __syncthreads();
        }
        best = s_bi[0];
        best_ssd = s_bv[0];
        if (rr && best >= count) best = 0;   // (no SSD compared below infinity: cannot happen with images made from bytes)
    }
    const SbiBatchRec* rec = g.recs && !rr ? g.recs + blockIdx.x : nullptr;
    const float *tgt_base = g.tgt_tmpl, *tjac_base = g.tgt_jacs;
    if (rr) tgt_base = rr->bank_tmpl, tjac_base = rr->bank_jacs;
    const float* __restrict__ tgt = rec ? rec->tgt_tmpl : tgt_base + (size_t)(best > 0 ? best : 0) * n;
    const float* __restrict__ tjac = rec ? rec->tgt_jacs : tjac_base + (size_t)(best > 0 ? best : 0) * 2 * n;
    const float* __restrict__ cur = rec ? rec->tmpl : g.cur;
    // (volatile: otherwise the compiler selects among the three ADDRESSES the pointer is read from, which needs a copy of g.cur in scratch
    //  memory, and a kernel that needs scratch is dispatched later)
    if (rr) cur = *(const float* const volatile*)&rr->cur;
    for (int i = tid; i < n; i += SBI_THREADS) s_cur[i] = cur[i];
    // thread 0's state
    double R2[4] = {1.0, 0.0, 0.0, 1.0}, t2[2] = {0.0, 0.0}, mean_offset = 0.0, score = 0.0;
    int done = 0, n_used = 0, degenerate = 0;
    const int icx = w / 2, icy = h / 2;   // irCenter = mirSize / 2
    for (int it = 0; it < g.iterations; it++) {
        if (tid == 0) {
            // se2XForm = se2WfromC * se2CtoC * se2WfromC.inverse(): rotation R, translation (c + t) + R * (-c)
            const double cx = (double)icx, cy = (double)icy;
            const double Tx = nc_add(nc_add(cx, t2[0]), nc_add(nc_mul(R2[0], -cx), nc_mul(R2[1], -cy)));
            const double Ty = nc_add(nc_add(cy, t2[1]), nc_add(nc_mul(R2[2], -cx), nc_mul(R2[3], -cy)));
            // CVD::transform(in, out, M = R, inOrig = T, outOrig = 0): p0 = inOrig - M * outOrig = T
            const double ax = R2[0], ay = R2[2], dx = R2[1], dy = R2[3];
            double min_x = Tx, min_y = Ty, max_x = Tx, max_y = Ty;
            if (ax < 0) min_x = nc_add(min_x, nc_mul(w, ax)); else max_x = nc_add(max_x, nc_mul(w, ax));
            if (dx < 0) min_x = nc_add(min_x, nc_mul(h, dx)); else max_x = nc_add(max_x, nc_mul(h, dx));
            if (ay < 0) min_y = nc_add(min_y, nc_mul(w, ay)); else max_y = nc_add(max_y, nc_mul(w, ay));
            if (dy < 0) min_y = nc_add(min_y, nc_mul(h, dy)); else max_y = nc_add(max_y, nc_mul(h, dy));
            const double crx = nc_sub(dx, nc_mul(w, ax)), cry = nc_sub(dy, nc_mul(w, ay));   // carriage_return
            s_walk.ax = ax;
            s_walk.ay = ay;
            s_walk.all_inside = min_x >= 0 && min_y >= 0 && max_x < w - 1 && max_y < h - 1;
            s_walk.stop = 0;
            s_walk.mean_offset = mean_offset;
            // the walk's row starts: the reference adds `across` pixel by pixel and the carriage return per row, and so does this
            double px = Tx, py = Ty;
            for (int y = 0; y < h; y++) {
                s_rowx[y] = px;
                s_rowy[y] = py;
                sbi_walk(px, py, ax, ay, w);
                px = nc_add(px, crx);
                py = nc_add(py, cry);
            }
        }
        __syncthreads();
        {
            const double ax = s_walk.ax, ay = s_walk.ay;
            const bool all_inside = s_walk.all_inside;
            for (int i = tid; i < n; i += SBI_THREADS) {
                const int x = i % w, y = i / w;
                double px = s_rowx[y], py = s_rowy[y];
                sbi_walk(px, py, ax, ay, x);
                float out = -9e20f;   // defaultValue
                if (all_inside || (0 <= px && 0 <= py && px < (double)(w - 1) && py < (double)(h - 1))) {
                    // CVD::sample: the bilinear blend in double, rounded once to float
                    const int lx = (int)px, ly = (int)py;
                    const double fx = nc_sub(px, (double)lx), fy = nc_sub(py, (double)ly);
                    const float* p = s_cur + ly * w + lx;
                    const double a = p[0], b = p[1], c = p[w], d = p[w + 1];
                    const double omx = nc_sub(1.0, fx), omy = nc_sub(1.0, fy);
                    const double top = nc_add(nc_mul(omx, a), nc_mul(fx, b)), bot = nc_add(nc_mul(omx, c), nc_mul(fx, d));
                    out = (float)nc_add(nc_mul(omy, top), nc_mul(fy, bot));
                }
                s_warp[i] = out;
            }
        }
        __syncthreads();
        double acc[15];   // v4Accum (4), v10Triangle (10), dFinalScore
#pragma unroll
        for (int k = 0; k < 15; k++) acc[k] = 0.0;
        int cnt = 0;
        const double moff = s_walk.mean_offset;
        for (int i = tid; i < n; i += SBI_THREADS) {
            const int x = i % w, y = i / w;
            if (!(x >= 1 && y >= 1 && x < w - 1 && y < h - 1)) continue;
            const float l = s_warp[i - 1], r = s_warp[i + 1], u = s_warp[i - w], d = s_warp[i + w], here = s_warp[i];
            if ((double)nc_addf(nc_addf(nc_addf(nc_addf(l, r), u), d), here) < -9999.9) continue;   // a neighbour fell outside
            const double g0 = nc_mul(0.25, nc_add((double)(r - l), (double)tjac[2 * i]));
            const double g1 = nc_mul(0.25, nc_add((double)(d - u), (double)tjac[2 * i + 1]));
            const double J[4] = {g0, g1, nc_add(nc_mul((double)-(y - icy), g0), nc_mul((double)(x - icx), g1)), 1.0};
            const double diff = nc_add((double)(here - tgt[i]), moff);
            cnt++;
            acc[14] += diff * diff;
#pragma unroll
            for (int k = 0; k < 4; k++) acc[k] += diff * J[k];
            acc[4] += J[0] * J[0];
            acc[5] += J[1] * J[0];
            acc[6] += J[1] * J[1];
            acc[7] += J[2] * J[0];
            acc[8] += J[2] * J[1];
            acc[9] += J[2] * J[2];
            acc[10] += J[0];
            acc[11] += J[1];
            acc[12] += J[2];
            acc[13] += 1.0;
        }
        // lanes, then waves, in a fixed order: a rerun gives the same bits
#pragma unroll
        for (int k = 0; k < 15; k++) acc[k] = wave_sum_f64(acc[k]);
        cnt = wave_sum_i32(cnt);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 15; k++) s_red[tid >> 6][k] = acc[k];
            s_cnt[tid >> 6] = cnt;
        }
        __syncthreads();
        if (tid == 0) {
            double tot[15];
            for (int k = 0; k < 15; k++) {
                tot[k] = s_red[0][k];
                for (int wv = 1; wv < SBI_THREADS / 64; wv++) tot[k] += s_red[wv][k];
            }
            n_used = 0;
            for (int wv = 0; wv < SBI_THREADS / 64; wv++) n_used += s_cnt[wv];
            score = tot[14];
            double m4[4][4], upd[4];
            const double b4[4] = {tot[0], tot[1], tot[2], tot[3]};
            int v = 4;
            for (int j = 0; j < 4; j++)
                for (int i = 0; i <= j; i++) m4[j][i] = m4[i][j] = tot[v++];
            // se2CtoC = se2CtoC * (-update[0:2], SO2::exp(-update[2])); dMeanOffset -= update[3] — on copies: a pivot that is not
            // strictly positive (a blank frame, a warp that left no pixel) or a step that is not finite (a tiny pivot: a nearly
            // blank frame) ends the iteration, and the SE2 of the previous iteration stands
            bool ok = sbi_ldlt_solve<4>(m4, b4, upd);
            double n[4] = {0, 0, 0, 0}, nt[2] = {0, 0}, nm = 0;
            if (ok) {
                const double th = -upd[2], cs = cos(th), sn = sin(th);
                const double ux = -upd[0], uy = -upd[1];
                n[0] = R2[0] * cs + R2[1] * sn, n[1] = R2[0] * -sn + R2[1] * cs;
                n[2] = R2[2] * cs + R2[3] * sn, n[3] = R2[2] * -sn + R2[3] * cs;
                nt[0] = t2[0] + (R2[0] * ux + R2[1] * uy);
                nt[1] = t2[1] + (R2[2] * ux + R2[3] * uy);
                nm = mean_offset - upd[3];
                ok = isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]) && isfinite(n[3]) && isfinite(nt[0]) && isfinite(nt[1]) && isfinite(nm);
            }
            if (!ok) {
                degenerate = 1;
                s_walk.stop = 1;
            } else {
                for (int i = 0; i < 4; i++) R2[i] = n[i];
                t2[0] = nt[0], t2[1] = nt[1];
                mean_offset = nm;
                done = it + 1;
            }
        }
        __syncthreads();
        const int stop = s_walk.stop;
        __syncthreads();   // (thread 0 writes s_walk again at the top of the next iteration)
        if (stop) break;
    }
    if (tid == 0) {
        ptam_sbi_alignment o;
        for (int i = 0; i < 4; i++) o.se2_rot[i] = R2[i];
        o.se2_trans[0] = t2[0];
        o.se2_trans[1] = t2[1];
        o.score = score;
        o.mean_offset = mean_offset;
        sbi_se3_from_se2(g.cam, w, h, R2, t2, o.rotation);
        o.iterations_done = done;
        o.n_used = n_used;
        o.degenerate = degenerate;
        o.pad_ = 0;
        if (rec) {
            // the frame's prediction (src/Tracker.cc:1013-1029 with mbUseSBIInit) where the rotation is: into the frame's pose for
            // the PVS pass, and with the alignment into the frame's host-mapped block.  No sequence word of its own: the frame's
            // last kernel, later on this queue, publishes one, and the fence below is passed before this kernel ends.
            double pose[12];
            motion_predict_sbi_hd(rec->velocity, rec->start_pose, o.rotation, pose);
            for (int i = 0; i < 12; i++) rec->pose_out[i] = pose[i];
            *rec->h_align = o;
            for (int i = 0; i < 12; i++) rec->h_pose_in[i] = pose[i];
            __threadfence_system();
            return;
        }
        if (rr) {
            // mse3Best = rotation * se3CfromW(best) in ptam_relocalise's operation order, never contracted: the host's bits.  The pose
            // goes where the frame's PVS pass reads it, the verdict into the frame's gate (the TrackMap kernels behind this launch
            // read it at their start) and everything into the frame's host-mapped block, which the frame's last kernel publishes.
            const double* K = rr->bank_poses + (size_t)best * 12;
            const double* R = o.rotation;
            double pose[12];   // (unrolled: a dynamically indexed local array is scratch memory)
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++)
                    pose[3 * i + j] = nc_add(nc_add(nc_mul(R[3 * i], K[j]), nc_mul(R[3 * i + 1], K[3 + j])), nc_mul(R[3 * i + 2], K[6 + j]));
                pose[9 + i] = nc_add(nc_add(nc_mul(R[3 * i], K[9]), nc_mul(R[3 * i + 1], K[10])), nc_mul(R[3 * i + 2], K[11]));
            }
            const int good = o.score < rr->max_score ? 1 : 0;
            ptam_reloc_result* out = rr->h_reloc;
            out->best = best;
            out->good = good;
            out->best_ssd = best_ssd;
            out->align = o;
#pragma unroll
            for (int i = 0; i < 12; i++) out->pose[i] = pose[i];
            if (good) {
#pragma unroll
                for (int i = 0; i < 12; i++) rr->pose_out[i] = pose[i];
            }
            *rr->gate = good;
            __threadfence_system();
            return;
        }
        g.out->a = o;
        g.out->best = best;
        g.out->pad_ = 0;
        g.out->best_ssd = best_ssd;
        __threadfence_system();
        *(volatile unsigned long long*)&g.out->seq = g.seq;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
struct SbiImage {   // one image's three device arrays
    uint8_t* small;
    float* tmpl;
    float* jacs;
};
struct SbiGeom {
    int fw, fh, w3, h3, w, h;
};

struct ptam_sbi {
    ptam_ctx* ctx;
    SbiGeom g;
    void* block;
    SbiImage im;
    int made;
};
struct ptam_sbi_bank {
    ptam_ctx* ctx;
    SbiGeom g;
    void* block;
    SbiImage im;   // entry 0; entry i follows n pixels (2 n for the Jacobians) further on
    double* ssd;   // [capacity]
    const uint8_t** l3_list;   // [capacity]: the level-3 images of a batch that is being added
    int capacity, count;
    // se3CfromW of the entries (ptam_sbi_bank_set_poses): on the device for mse3Best, and the host's mirror of it
    double* d_poses;                // [capacity][12]
    std::vector<double> h_poses;    // [capacity][12]
    std::vector<double> h_campos;   // [capacity][3]: the camera positions -R^T t of the mirror (the closest-keyframe walk reads these)
    std::vector<char> pose_set;     // [capacity]
    // where the entries came from.  blur: of the first entry made since the bank was empty (0: empty).  taken: the entries are a
    // snapshot's keyframes [0, count) of map (map_id, epoch), last taken at (snap_uid, snap_generation) — ptam_sbi_bank_take_keyframes
    double blur;
    int taken;
    long long snap_uid, snap_generation, map_id, epoch;
};
struct ptam_rotation_estimator {
    ptam_ctx* ctx;
    ptam_sbi* slot[2];
    int last;         // slot of mpSBILastFrame; -1 after a reset
    int pending;      // the slot the last step made, committed by sbi_estimator_commit
    double blur;
};

static int sbi_geom(int fw, int fh, SbiGeom* g) {
    ARG_TRY(fw > 0 && fh > 0);
    g->fw = fw, g->fh = fh;
    g->w3 = fw / 8, g->h3 = fh / 8;   // three halfSamples, each size / 2 by integer division
    g->w = g->w3 / 2, g->h = g->h3 / 2;
    ARG_TRY(g->w >= 3 && g->h >= 3);   // an interior to align on
    if (g->w > SBI_MAX_SIDE || g->h > SBI_MAX_SIDE || g->w * g->h > SBI_MAX_PIXELS) {
        ptam_set_error("a SmallBlurryImage of %d x %d is above the limit of %d pixels, %d a side", g->w, g->h, SBI_MAX_PIXELS, SBI_MAX_SIDE);
        return PTAM_E_LIMIT;
    }
    return PTAM_OK;
}

static size_t sbi_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// n images' arrays in one device block: small | tmpl | jacs
static int sbi_alloc(const SbiGeom& g, int n_images, size_t extra, void** block, SbiImage* im, void** extra_out) {
    const size_t n = (size_t)g.w * g.h * n_images;
    const size_t o_t = sbi_up256(n), o_j = o_t + sbi_up256(n * 4), o_x = o_j + sbi_up256(n * 8);
    HIP_TRY(hipMalloc(block, o_x + extra));
    im->small = (uint8_t*)*block;
    im->tmpl = (float*)((char*)*block + o_t);
    im->jacs = (float*)((char*)*block + o_j);
    if (extra_out) *extra_out = (char*)*block + o_x;
    return PTAM_OK;
}

static int sbi_check_kf(const ptam_ctx* ctx, const SbiGeom& g, const ptam_kf* kf) {
    ARG_TRY(kf && kf->device == ctx->device && kf->L.w[3] == g.w3 && kf->L.h[3] == g.h3);
    return PTAM_OK;
}

// exp(-i^2 / 2 sigma^2), normalised to sum 1
static void sbi_make_weights(double blur, SbiMakeArgs* a) {
    a->k = (int)std::ceil(3.0 * blur);
    double sum = 0.0;
    for (int i = -a->k; i <= a->k; i++) sum += (a->wt[i + a->k] = std::exp(-(double)(i * i) / (2.0 * blur * blur)));
    for (int i = 0; i <= 2 * a->k; i++) a->wt[i] /= sum;
    for (int i = 2 * a->k + 1; i <= 2 * SBI_MAX_TAPS; i++) a->wt[i] = 0.0;
}
// camera.SetImageSize(mirSize) + RefreshParams (src/ATANCamera.cc:21-40): focal and centre scale with the size
static DevCam sbi_camera(const ptam_ctx* ctx, const SbiGeom& g) {
    const ptam_cam_params& p = ctx->params;
    DevCam c = ctx->cam;
    c.width = g.w, c.height = g.h;
    c.fx = g.w * p.fx, c.fy = g.h * p.fy;
    c.cx = g.w * p.cx - 0.5, c.cy = g.h * p.cy - 0.5;
    c.inv_fx = 1.0 / c.fx, c.inv_fy = 1.0 / c.fy;
    return c;
}

// one launch for n images: image b from kf (n == 1) or from d_list[b], into im's arrays b images further on
static int sbi_launch_make(ptam_ctx* ctx, const SbiGeom& g, const ptam_kf* kf, double blur, const SbiImage& im, int n = 1,
                           const uint8_t* const* d_list = nullptr) {
    if (kf)
        if (int rc = sbi_check_kf(ctx, g, kf)) return rc;
    ARG_TRY(blur > 0.0 && blur <= 5.0);
    SbiMakeArgs a;
    a.l3 = kf ? kf->L.im[3] : nullptr;
    a.l3_list = d_list;
    a.recs = nullptr;
    a.w3 = g.w3, a.w = g.w, a.h = g.h;
    a.small = im.small, a.tmpl = im.tmpl, a.jacs = im.jacs;
    sbi_make_weights(blur, &a);
    if (ctx->halfsample == PTAM_HALFSAMPLE_T)
        hipLaunchKernelGGL(sbi_make_kernel<PTAM_HALFSAMPLE_T>, dim3(n), dim3(SBI_THREADS), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(sbi_make_kernel<PTAM_HALFSAMPLE_R>, dim3(n), dim3(SBI_THREADS), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

// the align launch and its mapped wait; bank (nullable): the target is the bank's nearest entry (its SSDs are on the queue already)
static int sbi_align(ptam_ctx* ctx, const SbiGeom& g, const float* cur, const SbiImage& target, const ptam_sbi_bank* bank, int iterations,
                     size_t pin_offset, SbiOut* result) {
    ARG_TRY(iterations >= 1 && iterations <= SBI_MAX_ITERATIONS);
    void* hp;
    if (int rc = ctx_pinned(ctx, pin_offset + sizeof(SbiOut), &hp)) return rc;
    SbiAlignArgs a;
    a.cur = cur;
    a.tgt_tmpl = target.tmpl, a.tgt_jacs = target.jacs;
    a.ssd = bank ? bank->ssd : nullptr;
    a.count = bank ? bank->count : 0;
    a.w = g.w, a.h = g.h, a.iterations = iterations;
    a.cam = sbi_camera(ctx, g);
    a.out = (SbiOut*)((char*)ctx->d_pinned + pin_offset);
    a.recs = nullptr;
    a.det_items = nullptr, a.det_stride = a.det_off = 0, a.det_blocks = a.n_align = 0;
    a.rrecs = nullptr, a.n_est = 0;
    a.seq = ++ctx->pose_seq;
    volatile SbiOut* h_out = (volatile SbiOut*)((char*)hp + pin_offset);
    h_out->seq = 0;   // (the staging buffer is shared: no stale sequence numbers)
    hipLaunchKernelGGL(sbi_align_kernel, dim3(1), dim3(SBI_THREADS), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if (int rc = ptam_wait_mapped(ctx->stream, "the SmallBlurryImage alignment", [&] { return h_out->seq == a.seq; })) return rc;
    std::memcpy(result, (const void*)h_out, sizeof *result);
    return PTAM_OK;
}

void sbi_preload_kernels() {
    ptam_preload((const void*)sbi_make_kernel<PTAM_HALFSAMPLE_R>);
    ptam_preload((const void*)sbi_make_kernel<PTAM_HALFSAMPLE_T>);
    ptam_preload((const void*)sbi_ssd_kernel);
    ptam_preload((const void*)sbi_ssd_batch_kernel);
    ptam_preload((const void*)sbi_align_kernel);
    ptam_preload((const void*)sbi_take_kernel);
}

int sbi_estimator_step(ptam_rotation_estimator* e, const ptam_kf* kf, ptam_sbi_alignment* out) {
    ARG_TRY(e && kf && out);
    HIP_TRY(hipSetDevice(e->ctx->device));
    const int cur = e->last < 0 ? 0 : 1 - e->last;
    ptam_sbi* c = e->slot[cur];
    if (int rc = sbi_launch_make(e->ctx, c->g, kf, e->blur, c->im)) return rc;
    SbiOut r;
    if (int rc = sbi_align(e->ctx, c->g, c->im.tmpl, e->slot[e->last < 0 ? cur : e->last]->im, nullptr, 6, 0, &r)) return rc;
    e->pending = cur;
    *out = r.a;
    return PTAM_OK;
}
void sbi_estimator_commit(ptam_rotation_estimator* e) {
    if (e->pending >= 0) e->last = e->pending;
    e->pending = -1;
}
ptam_ctx* sbi_estimator_ctx(const ptam_rotation_estimator* e) { return e->ctx; }

// ---- the estimators' steps of a batch of frames: sbi_estimator_step's two launches, once for all frames ----
int sbi_batch_rec(ptam_rotation_estimator* e, const ptam_kf* kf, SbiBatchRec* rec) {
    const int cur = e->last < 0 ? 0 : 1 - e->last;
    const ptam_sbi *c = e->slot[cur], *tgt = e->slot[e->last < 0 ? cur : e->last];
    if (int rc = sbi_check_kf(e->ctx, c->g, kf)) return rc;
    rec->l3 = kf->L.im[3];
    rec->small = c->im.small, rec->tmpl = c->im.tmpl, rec->jacs = c->im.jacs;
    rec->tgt_tmpl = tgt->im.tmpl, rec->tgt_jacs = tgt->im.jacs;
    e->pending = cur;
    return PTAM_OK;
}
void sbi_estimator_rollback(ptam_rotation_estimator* e) { e->pending = -1; }
bool sbi_estimators_alike(const ptam_rotation_estimator* a, const ptam_rotation_estimator* b) {
    return a->blur == b->blur && a->slot[0]->g.fw == b->slot[0]->g.fw && a->slot[0]->g.fh == b->slot[0]->g.fh;
}
// the make launch for n records: image b from record b's level 3 into record b's three arrays
static int sbi_make_recs(const ptam_ctx* ctx, const SbiGeom& g, double blur, int n, const SbiBatchRec* d_recs, hipStream_t st) {
    SbiMakeArgs a;
    a.l3 = nullptr, a.l3_list = nullptr, a.recs = d_recs;
    a.w3 = g.w3, a.w = g.w, a.h = g.h;
    a.small = nullptr, a.tmpl = nullptr, a.jacs = nullptr;
    sbi_make_weights(blur, &a);
    if (ctx->halfsample == PTAM_HALFSAMPLE_T)
        hipLaunchKernelGGL(sbi_make_kernel<PTAM_HALFSAMPLE_T>, dim3(n), dim3(SBI_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL(sbi_make_kernel<PTAM_HALFSAMPLE_R>, dim3(n), dim3(SBI_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
// the align launch: n_est estimator workgroups, n_reloc relocaliser workgroups, then the detection's
static int sbi_align_recs(const ptam_ctx* ctx, const SbiGeom& g, int n_est, const SbiBatchRec* d_recs, int n_reloc, const SbiRelocRec* d_rrecs,
                          hipStream_t st, int nb_detect, const KfLevels* L, const void* det_items, size_t det_stride, size_t det_off) {
    SbiAlignArgs a;
    a.cur = a.tgt_tmpl = a.tgt_jacs = nullptr;
    a.ssd = nullptr;
    a.count = 0;
    a.w = g.w, a.h = g.h, a.iterations = 6;   // (sbi_estimator_step's and ptam_relocalise's)
    a.cam = sbi_camera(ctx, g);
    a.out = nullptr;
    a.seq = 0;
    a.recs = d_recs;
    a.det_items = nb_detect > 0 ? (const char*)det_items : nullptr;
    a.det_stride = det_stride, a.det_off = det_off;
    a.det_blocks = nb_detect > 0 ? fast_detect_tall_blocks(*L) : 0;
    a.n_align = n_est + n_reloc;
    a.rrecs = n_reloc > 0 ? d_rrecs : nullptr, a.n_est = n_est;
    hipLaunchKernelGGL(sbi_align_kernel, dim3(a.n_align + nb_detect * a.det_blocks), dim3(SBI_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
int sbi_batch_launch_make(const ptam_rotation_estimator* lead, int n, const SbiBatchRec* d_recs, hipStream_t st) {
    return sbi_make_recs(lead->ctx, lead->slot[0]->g, lead->blur, n, d_recs, st);
}
int sbi_batch_launch_align(const ptam_rotation_estimator* lead, int n, const SbiBatchRec* d_recs, hipStream_t st, int nb_detect, const KfLevels* L,
                           const void* det_items, size_t det_stride, size_t det_off) {
    return sbi_align_recs(lead->ctx, lead->slot[0]->g, n, d_recs, 0, nullptr, st, nb_detect, L, det_items, det_stride, det_off);
}

// ---- the recovering cameras of a batch (ptam_track_frames_recover_batch) ----
int sbi_reloc_check(const ptam_sbi_bank* b, const ptam_sbi* scratch, int device, const ptam_kf* kf) {
    ARG_TRY(b && scratch);
    ARG_TRY(b->ctx->device == device && scratch->ctx->device == device);
    ARG_TRY(scratch->g.fw == b->g.fw && scratch->g.fh == b->g.fh);
    if (int rc = sbi_check_kf(b->ctx, b->g, kf)) return rc;
    if (b->count < 1) {
        ptam_set_error("a recovering camera's bank is empty");
        return PTAM_E_STATE;
    }
    for (int i = 0; i < b->count; i++)
        if (!b->pose_set[(size_t)i]) {
            ptam_set_error("the pose of bank entry %d was never set (ptam_sbi_bank_set_poses)", i);
            return PTAM_E_STATE;
        }
    return PTAM_OK;
}
void sbi_reloc_rec(const ptam_sbi_bank* b, const ptam_sbi* scratch, const ptam_kf* kf, SbiBatchRec* mk, SbiRelocRec* rec) {
    mk->l3 = kf->L.im[3];
    mk->small = scratch->im.small, mk->tmpl = scratch->im.tmpl, mk->jacs = scratch->im.jacs;
    rec->cur = scratch->im.tmpl;
    rec->bank_tmpl = b->im.tmpl, rec->bank_jacs = b->im.jacs;
    rec->bank_poses = b->d_poses;
    rec->count = b->count;
}
void sbi_reloc_commit(ptam_sbi* scratch) { scratch->made = 1; }
ptam_ctx* sbi_bank_ctx(const ptam_sbi_bank* b) { return b->ctx; }
const double* sbi_bank_camera_positions(const ptam_sbi_bank* b, int* count) {
    *count = b->count;
    for (int i = 0; i < b->count; i++)
        if (!b->pose_set[(size_t)i]) return nullptr;
    return b->h_campos.data();
}
int sbi_reloc_launch_make(ptam_ctx* ctx, const ptam_sbi_bank* b, double blur, int n, const SbiBatchRec* d_recs, hipStream_t st) {
    ARG_TRY(blur > 0.0 && blur <= 5.0);
    return sbi_make_recs(ctx, b->g, blur, n, d_recs, st);
}
int sbi_reloc_launch_ssd(const ptam_sbi_bank* b, int n, int max_count, const SbiRelocRec* d_rrecs, hipStream_t st) {
    hipLaunchKernelGGL(sbi_ssd_batch_kernel, dim3(max_count, n), dim3(SBI_THREADS), 0, st, d_rrecs, b->g.w * b->g.h);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
int sbi_recover_launch_align(ptam_ctx* ctx, const ptam_sbi_bank* b, int n_est, const SbiBatchRec* d_recs, int n_reloc, const SbiRelocRec* d_rrecs,
                             hipStream_t st, int nb_detect, const KfLevels* L, const void* det_items, size_t det_stride, size_t det_off) {
    return sbi_align_recs(ctx, b->g, n_est, d_recs, n_reloc, d_rrecs, st, nb_detect, L, det_items, det_stride, det_off);
}
bool sbi_estimator_fits_bank(const ptam_rotation_estimator* e, const ptam_sbi_bank* b) {
    return e->slot[0]->g.fw == b->g.fw && e->slot[0]->g.fh == b->g.fh;
}

// ---- the map's keyframes through a ptam_map_snapshot: the slots' keyframe sections and the bank's take ----
// A slot's section is a bank's block (sbi_alloc) with the pose table behind it; sbi_geom of the snapshot's frame size gives the
// image size, so a slot's entry i and a bank's entry i lie at the same offsets.
static bool sbi_snapshot_kf_state(ptam_map_snapshot* snap, int* kf_max, double* blur, bool* writing) {
    std::lock_guard<std::mutex> lk(snap->slots.mu);   // (enable writes the two under the same mutex)
    if (kf_max) *kf_max = snap->kf_max;
    if (blur) *blur = snap->kf_blur;
    if (writing) *writing = snap->slots.writing != SnapSlots::NEVER;
    return snap->kf_max > 0;
}
bool sbi_snapshot_kf_enabled(ptam_map_snapshot* snap) { return sbi_snapshot_kf_state(snap, nullptr, nullptr, nullptr); }

int sbi_snapshot_kf_check(ptam_map_snapshot* snap, int n_kf, const ptam_kf* const* kfs) {
    int kf_max = 0;
    if (!sbi_snapshot_kf_state(snap, &kf_max, nullptr, nullptr)) return PTAM_OK;
    if (n_kf > kf_max) {
        ptam_set_error("ptam_rmap_publish: the map has %d keyframes, the snapshot's keyframe section room for %d", n_kf, kf_max);
        return PTAM_E_LIMIT;
    }
    SbiGeom g;
    if (int rc = sbi_geom(snap->width, snap->height, &g)) return rc;
    for (int k = 0; k < n_kf; k++) ARG_TRY(kfs[k] && kfs[k]->L.w[3] == g.w3 && kfs[k]->L.h[3] == g.h3);
    return PTAM_OK;
}

int sbi_snapshot_kf_first_missing(const ptam_map_snapshot* snap, int s, long long map_id, long long epoch, int n_kf) {
    const SnapSlot& sl = snap->slot[s];
    return sl.kf_map_id == map_id && sl.kf_epoch == epoch ? std::min(sl.kf_n, n_kf) : 0;
}

int sbi_snapshot_kf_enqueue(ptam_ctx* ctx, ptam_map_snapshot* snap, int s, int n_kf, const double* d_poses, int first, const uint8_t* const* d_l3) {
    SnapSlot& sl = snap->slot[s];
    SbiGeom g;
    if (int rc = sbi_geom(snap->width, snap->height, &g)) return rc;
    if (n_kf > 0) HIP_TRY(hipMemcpyAsync(sl.kf_poses, d_poses, (size_t)n_kf * 96, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_kf > first) {
        const size_t px = (size_t)g.w * g.h, i = (size_t)first;
        const SbiImage im = {sl.kf_small + i * px, sl.kf_tmpl + i * px, sl.kf_jacs + i * 2 * px};
        if (int rc = sbi_launch_make(ctx, g, nullptr, snap->kf_blur, im, n_kf - first, d_l3)) return rc;
    }
    return PTAM_OK;
}

void sbi_snapshot_kf_stamp(ptam_map_snapshot* snap, int s, int n_kf, int first, long long map_id, long long epoch, long long generation) {
    SnapSlot& sl = snap->slot[s];
    sl.kf_n = n_kf;
    sl.kf_made = n_kf - first;
    sl.kf_map_id = map_id;
    sl.kf_epoch = epoch;
    sl.kf_generation = generation;
}

static int sbi_bank_not_taken(const ptam_sbi_bank* b) {
    if (b->taken) {
        ptam_set_error("the bank's entries are a snapshot's keyframes (ptam_sbi_bank_take_keyframes): ptam_sbi_bank_clear before adding by hand");
        return PTAM_E_STATE;
    }
    return PTAM_OK;
}

extern "C" {

int ptam_sbi_create(ptam_ctx* ctx, int frame_w, int frame_h, ptam_sbi** out) {
    ARG_TRY(ctx && out);
    SbiGeom g;
    if (int rc = sbi_geom(frame_w, frame_h, &g)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_sbi* s = new ptam_sbi();
    s->ctx = ctx, s->g = g, s->made = 0;
    if (int rc = sbi_alloc(g, 1, 0, &s->block, &s->im, nullptr)) {
        delete s;
        return rc;
    }
    *out = s;
    return PTAM_OK;
}

int ptam_sbi_destroy(ptam_sbi* s) {
    if (!s) return PTAM_OK;
    hipSetDevice(s->ctx->device);
    ptam_stream_wait(s->ctx->stream);
    hipFree(s->block);
    delete s;
    return PTAM_OK;
}

int ptam_sbi_make(ptam_sbi* s, const ptam_kf* kf, double blur) {
    ARG_TRY(s && kf);
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (int rc = sbi_launch_make(s->ctx, s->g, kf, blur, s->im)) return rc;
    s->made = 1;
    return PTAM_OK;
}

int ptam_sbi_size(const ptam_sbi* s, int* w, int* h) {
    ARG_TRY(s && w && h);
    *w = s->g.w, *h = s->g.h;
    return PTAM_OK;
}

int ptam_sbi_read(ptam_sbi* s, uint8_t* small, float* tmpl, float* jacs) {
    ARG_TRY(s);
    if (!s->made) {
        ptam_set_error("ptam_sbi_read before ptam_sbi_make");
        return PTAM_E_STATE;
    }
    HIP_TRY(hipSetDevice(s->ctx->device));
    const size_t n = (size_t)s->g.w * s->g.h;
    hipStream_t st = s->ctx->stream;
    if (small) HIP_TRY(hipMemcpyAsync(small, s->im.small, n, hipMemcpyDeviceToHost, st));
    if (tmpl) HIP_TRY(hipMemcpyAsync(tmpl, s->im.tmpl, n * 4, hipMemcpyDeviceToHost, st));
    if (jacs) HIP_TRY(hipMemcpyAsync(jacs, s->im.jacs, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    return PTAM_OK;
}

int ptam_sbi_calc_rotation(ptam_sbi* current, const ptam_sbi* target, int iterations, ptam_sbi_alignment* out) {
    ARG_TRY(current && target && out);
    ARG_TRY(current->ctx == target->ctx && current->g.w == target->g.w && current->g.h == target->g.h);
    if (!current->made || !target->made) {
        ptam_set_error("ptam_sbi_calc_rotation before ptam_sbi_make of both images");
        return PTAM_E_STATE;
    }
    HIP_TRY(hipSetDevice(current->ctx->device));
    SbiOut r;
    if (int rc = sbi_align(current->ctx, current->g, current->im.tmpl, target->im, nullptr, iterations, 0, &r)) return rc;
    *out = r.a;
    return PTAM_OK;
}

int ptam_sbi_bank_create(ptam_ctx* ctx, int frame_w, int frame_h, int capacity, ptam_sbi_bank** out) {
    ARG_TRY(ctx && out && capacity >= 1 && capacity <= 65535);
    SbiGeom g;
    if (int rc = sbi_geom(frame_w, frame_h, &g)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_sbi_bank* b = new ptam_sbi_bank();
    b->ctx = ctx, b->g = g, b->capacity = capacity, b->count = 0;
    b->blur = 0.0, b->taken = 0;
    b->snap_uid = b->snap_generation = b->map_id = b->epoch = 0;
    void* x;
    if (int rc = sbi_alloc(g, capacity, (size_t)capacity * (16 + 96), &b->block, &b->im, &x)) {
        delete b;
        return rc;
    }
    b->ssd = (double*)x;
    b->l3_list = (const uint8_t**)(b->ssd + capacity);
    b->d_poses = (double*)((char*)x + (size_t)capacity * 16);
    b->h_poses.assign((size_t)capacity * 12, 0.0);
    b->h_campos.assign((size_t)capacity * 3, 0.0);
    b->pose_set.assign((size_t)capacity, 0);
    *out = b;
    return PTAM_OK;
}

int ptam_sbi_bank_destroy(ptam_sbi_bank* b) {
    if (!b) return PTAM_OK;
    hipSetDevice(b->ctx->device);
    ptam_stream_wait(b->ctx->stream);
    hipFree(b->block);
    delete b;
    return PTAM_OK;
}

int ptam_sbi_bank_add(ptam_sbi_bank* b, const ptam_kf* kf, double blur, int* index) {
    ARG_TRY(b && kf);
    if (int rc = sbi_bank_not_taken(b)) return rc;
    if (b->count >= b->capacity) {
        ptam_set_error("the SmallBlurryImage bank is full (%d entries)", b->capacity);
        return PTAM_E_LIMIT;
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    const size_t n = (size_t)b->g.w * b->g.h, i = (size_t)b->count;
    const SbiImage im = {b->im.small + i * n, b->im.tmpl + i * n, b->im.jacs + i * 2 * n};
    if (int rc = sbi_launch_make(b->ctx, b->g, kf, blur, im)) return rc;
    if (index) *index = b->count;
    if (b->count == 0) b->blur = blur;
    b->count++;
    return PTAM_OK;
}

int ptam_sbi_bank_add_batch(ptam_sbi_bank* b, int n, const ptam_kf* const* kfs, double blur, int* first_index) {
    ARG_TRY(b && kfs && n >= 1);
    if (int rc = sbi_bank_not_taken(b)) return rc;
    if (n > b->capacity - b->count) {
        ptam_set_error("the SmallBlurryImage bank has room for %d more entries, not %d", b->capacity - b->count, n);
        return PTAM_E_LIMIT;
    }
    std::vector<const uint8_t*> l3((size_t)n);
    for (int i = 0; i < n; i++) {
        if (int rc = sbi_check_kf(b->ctx, b->g, kfs[i])) return rc;
        l3[(size_t)i] = kfs[i]->L.im[3];
    }
    HIP_TRY(hipSetDevice(b->ctx->device));
    // (pageable source: the runtime has staged it when the call returns)
    HIP_TRY(hipMemcpyAsync(b->l3_list + b->count, l3.data(), (size_t)n * sizeof(l3[0]), hipMemcpyHostToDevice, b->ctx->stream));
    const size_t px = (size_t)b->g.w * b->g.h, i = (size_t)b->count;
    const SbiImage im = {b->im.small + i * px, b->im.tmpl + i * px, b->im.jacs + i * 2 * px};
    if (int rc = sbi_launch_make(b->ctx, b->g, nullptr, blur, im, n, b->l3_list + b->count)) return rc;
    if (first_index) *first_index = b->count;
    if (b->count == 0) b->blur = blur;
    b->count += n;
    return PTAM_OK;
}

int ptam_sbi_bank_count(const ptam_sbi_bank* b, int* n) {
    ARG_TRY(b && n);
    *n = b->count;
    return PTAM_OK;
}

int ptam_sbi_bank_set_poses(ptam_sbi_bank* b, int first, int n, const double* poses12) {
    ARG_TRY(b && poses12 && first >= 0 && n >= 1 && n <= b->count && first <= b->count - n);
    HIP_TRY(hipSetDevice(b->ctx->device));
    double* h = b->h_poses.data() + (size_t)first * 12;
    // (the mirror is the copy's source and lives as long as the bank; a second set of the same entries waits for the first copy)
    for (int i = first; i < first + n; i++)
        if (b->pose_set[(size_t)i]) {
            HIP_TRY(ptam_stream_wait(b->ctx->stream));
            break;
        }
    std::memcpy(h, poses12, (size_t)n * 96);
    HIP_TRY(hipMemcpyAsync(b->d_poses + (size_t)first * 12, h, (size_t)n * 96, hipMemcpyHostToDevice, b->ctx->stream));
    for (int i = first; i < first + n; i++) {
        b->pose_set[(size_t)i] = 1;
        const double* p = b->h_poses.data() + (size_t)i * 12;   // se3CfromW.inverse().get_translation(), src/MapMaker.cc:698
        for (int k = 0; k < 3; k++) b->h_campos[(size_t)i * 3 + k] = -(p[k] * p[9] + p[3 + k] * p[10] + p[6 + k] * p[11]);
    }
    return PTAM_OK;
}

int ptam_sbi_bank_poses(const ptam_sbi_bank* b, int first, int n, double* poses_out12) {
    ARG_TRY(b && poses_out12 && first >= 0 && n >= 1 && n <= b->count && first <= b->count - n);
    for (int i = first; i < first + n; i++)
        if (!b->pose_set[(size_t)i]) {
            ptam_set_error("the pose of bank entry %d was never set", i);
            return PTAM_E_STATE;
        }
    std::memcpy(poses_out12, b->h_poses.data() + (size_t)first * 12, (size_t)n * 96);
    return PTAM_OK;
}

int ptam_sbi_bank_read(ptam_sbi_bank* b, int index, uint8_t* small, float* tmpl, float* jacs) {
    ARG_TRY(b && index >= 0 && index < b->count);
    HIP_TRY(hipSetDevice(b->ctx->device));
    const size_t n = (size_t)b->g.w * b->g.h, i = (size_t)index;
    hipStream_t st = b->ctx->stream;
    if (small) HIP_TRY(hipMemcpyAsync(small, b->im.small + i * n, n, hipMemcpyDeviceToHost, st));
    if (tmpl) HIP_TRY(hipMemcpyAsync(tmpl, b->im.tmpl + i * n, n * 4, hipMemcpyDeviceToHost, st));
    if (jacs) HIP_TRY(hipMemcpyAsync(jacs, b->im.jacs + i * 2 * n, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    return PTAM_OK;
}

int ptam_sbi_bank_clear(ptam_sbi_bank* b) {
    ARG_TRY(b);
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(ptam_stream_wait(b->ctx->stream));   // (a pending copy from the mirror, a launch that reads the entries)
    b->count = 0;
    b->blur = 0.0, b->taken = 0;
    b->snap_uid = b->snap_generation = b->map_id = b->epoch = 0;
    std::fill(b->pose_set.begin(), b->pose_set.end(), 0);
    return PTAM_OK;
}

int ptam_snapshot_keyframes_enable(ptam_map_snapshot* snap, int max_keyframes, double blur) {
    ARG_TRY(snap && max_keyframes >= 1 && max_keyframes <= 65535 && blur > 0.0 && blur <= 5.0);
    SbiGeom g;
    if (int rc = sbi_geom(snap->width, snap->height, &g)) return rc;
    bool writing = false;
    if (sbi_snapshot_kf_state(snap, nullptr, nullptr, &writing)) {
        ptam_set_error("ptam_snapshot_keyframes_enable: the snapshot's keyframe section is enabled already");
        return PTAM_E_STATE;
    }
    if (writing) {
        ptam_set_error("ptam_snapshot_keyframes_enable: a publish into this snapshot is under way");
        return PTAM_E_STATE;
    }
    HIP_TRY(hipSetDevice(snap->device));
    int rc = PTAM_OK;
    for (int k = 0; k < SnapSlots::SLOTS && !rc; k++) {
        SnapSlot& sl = snap->slot[k];
        SbiImage im;
        void* x;
        rc = sbi_alloc(g, max_keyframes, (size_t)max_keyframes * 96, &sl.kf_block, &im, &x);
        if (rc) break;
        sl.kf_small = im.small, sl.kf_tmpl = im.tmpl, sl.kf_jacs = im.jacs;
        sl.kf_poses = (double*)x;
        sl.kf_n = sl.kf_made = 0;
        sl.kf_map_id = sl.kf_epoch = sl.kf_generation = 0;
    }
    if (rc) {
        for (int k = 0; k < SnapSlots::SLOTS; k++) {
            if (snap->slot[k].kf_block) (void)hipFree(snap->slot[k].kf_block);
            snap->slot[k].kf_block = nullptr;
        }
        return rc;
    }
    std::lock_guard<std::mutex> lk(snap->slots.mu);
    snap->kf_max = max_keyframes;
    snap->kf_blur = blur;
    return PTAM_OK;
}

int ptam_snapshot_keyframes_info(ptam_map_snapshot* snap, ptam_snapshot_keyframes_info_t* out) {
    ARG_TRY(snap && out);
    ptam_snapshot_keyframes_info_t r = {};
    int kf_max = 0;
    double blur = 0.0;
    if (sbi_snapshot_kf_state(snap, &kf_max, &blur, nullptr)) {
        SbiGeom g;
        if (int rc = sbi_geom(snap->width, snap->height, &g)) return rc;
        r.enabled = 1;
        r.max_keyframes = kf_max;
        r.blur = blur;
        r.sbi_w = g.w, r.sbi_h = g.h;
        long long gen = 0;
        const int k = snap->slots.begin_read(-1, &gen);   // (-1 is no generation: the current slot, held while it is read)
        if (k >= 0) {
            const SnapSlot& sl = snap->slot[k];
            r.generation = sl.generation;
            if (sl.kf_generation == sl.generation) {
                r.map_id = sl.kf_map_id;
                r.epoch = sl.kf_epoch;
                r.n_kf = sl.kf_n;
                r.n_made = sl.kf_made;
            }
            snap->slots.end_read(k);
        }
    }
    *out = r;
    return PTAM_OK;
}

int ptam_sbi_bank_take_keyframes(ptam_sbi_bank* b, ptam_map_snapshot* snap, ptam_keyframes_take_result* res) {
    ARG_TRY(b && snap && res);
    double blur = 0.0;
    if (!sbi_snapshot_kf_state(snap, nullptr, &blur, nullptr)) {
        ptam_set_error("ptam_sbi_bank_take_keyframes: the snapshot's keyframe section is not enabled (ptam_snapshot_keyframes_enable)");
        return PTAM_E_STATE;
    }
    ARG_TRY(snap->device == b->ctx->device);
    ARG_TRY(snap->width == b->g.fw && snap->height == b->g.fh);
    if (b->count > 0 && !b->taken && b->blur != blur) {
        ptam_set_error("bad argument: ptam_sbi_bank_take_keyframes: the bank's entries were added with blur %g, the snapshot's are made with %g", b->blur,
                       blur);
        return PTAM_E_ARG;
    }
    ptam_keyframes_take_result r = {};
    long long gen = 0;
    const int k = snap->slots.begin_read(b->taken && b->snap_uid == snap->uid ? b->snap_generation : -1, &gen);
    if (k == SnapSlots::NEVER) {
        ptam_set_error("bad argument: ptam_sbi_bank_take_keyframes: nothing has been published into the snapshot");
        return PTAM_E_ARG;
    }
    if (k == SnapSlots::UNCHANGED) {   // the per-frame poll
        r.n_kf = b->count;
        r.generation = gen;
        r.map_id = b->map_id;
        *res = r;
        return PTAM_OK;
    }
    const SnapSlot& sl = snap->slot[k];   // ours until end_read: the publisher leaves it alone
    const int n = sl.kf_n;
    const long long map_id = sl.kf_map_id, epoch = sl.kf_epoch, generation = sl.generation;
    if (sl.kf_generation != sl.generation) {
        snap->slots.end_read(k);
        ptam_set_error("bad argument: ptam_sbi_bank_take_keyframes: nothing has been published into the snapshot since its keyframe section was enabled");
        return PTAM_E_ARG;
    }
    if (n > b->capacity) {
        snap->slots.end_read(k);
        ptam_set_error("ptam_sbi_bank_take_keyframes: the snapshot holds %d keyframes, the bank %d at most", n, b->capacity);
        return PTAM_E_LIMIT;
    }
    // a keyframe's image never changes: the entries the bank holds of this map stay, the others are copied
    const int first = b->taken && b->snap_uid == snap->uid && b->map_id == map_id && b->epoch == epoch && b->count <= n ? b->count : 0;
    const size_t px = (size_t)b->g.w * b->g.h;
    hipStream_t st = b->ctx->stream;
    int rc = hipSetDevice(b->ctx->device) == hipSuccess ? PTAM_OK : PTAM_E_HIP;
    // (the mirror may be the source of a pending ptam_sbi_bank_set_poses copy: as there, it is waited for before it is overwritten)
    if (!rc && ptam_stream_wait(st) != hipSuccess) rc = PTAM_E_HIP;
    if (!rc && n > 0) {
        SbiTakeArgs a;
        a.s_small = sl.kf_small, a.s_tmpl = sl.kf_tmpl, a.s_jacs = (const float2*)sl.kf_jacs, a.s_poses = sl.kf_poses;
        a.d_small = b->im.small, a.d_tmpl = b->im.tmpl, a.d_jacs = (float2*)b->im.jacs, a.d_poses = b->d_poses;
        a.px_first = (long long)(first * px);
        a.px_count = (long long)((size_t)(n - first) * px);
        a.n_pose = 12 * n;
        const long long threads = std::max(a.px_count, (long long)a.n_pose);
        hipLaunchKernelGGL(sbi_take_kernel, dim3((unsigned)std::min((threads + 255) / 256, 4096ll)), dim3(256), 0, st, a);
        if (hipGetLastError() != hipSuccess) rc = PTAM_E_HIP;
        if (!rc && hipMemcpyAsync(b->h_poses.data(), sl.kf_poses, (size_t)n * 96, hipMemcpyDeviceToHost, st) != hipSuccess) rc = PTAM_E_HIP;
        if (!rc && ptam_stream_wait(st) != hipSuccess) rc = PTAM_E_HIP;   // the call's one wait: the slot has been read
    }
    snap->slots.end_read(k);
    if (rc) {
        ptam_set_error("ptam_sbi_bank_take_keyframes: the copy failed: %s", hipGetErrorString(hipGetLastError()));
        return rc;
    }
    for (int i = 0; i < n; i++) {
        b->pose_set[(size_t)i] = 1;
        const double* p = b->h_poses.data() + (size_t)i * 12;   // se3CfromW.inverse().get_translation(), src/MapMaker.cc:698
        for (int j = 0; j < 3; j++) b->h_campos[(size_t)i * 3 + j] = -(p[j] * p[9] + p[3 + j] * p[10] + p[6 + j] * p[11]);
    }
    for (int i = n; i < b->capacity; i++) b->pose_set[(size_t)i] = 0;
    b->count = n;
    b->blur = blur;
    b->taken = 1;
    b->snap_uid = snap->uid, b->snap_generation = generation;
    b->map_id = map_id, b->epoch = epoch;
    r.changed = 1;
    r.n_kf = n;
    r.n_new = n - first;
    r.link_bytes = 96 * n;
    r.generation = generation;
    r.map_id = map_id;
    *res = r;
    return PTAM_OK;
}

int ptam_relocalise(ptam_sbi_bank* b, ptam_sbi* scratch, const ptam_kf* current, const double* kf_poses12, double blur, double max_score,
                    ptam_reloc_result* out, double* ssd_out) {
    ARG_TRY(b && scratch && current && kf_poses12 && out);
    ARG_TRY(scratch->ctx == b->ctx && scratch->g.w == b->g.w && scratch->g.h == b->g.h);
    if (b->count < 1) {
        ptam_set_error("ptam_relocalise on an empty bank");
        return PTAM_E_STATE;
    }
    ptam_ctx* ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t pin_ssd = sbi_up256((size_t)b->count * 8);
    void* hp;
    if (int rc = ctx_pinned(ctx, pin_ssd + sizeof(SbiOut), &hp)) return rc;   // (before the launches: growing it waits for the queue)
    if (int rc = sbi_launch_make(ctx, scratch->g, current, blur, scratch->im)) return rc;
    scratch->made = 1;
    hipLaunchKernelGGL(sbi_ssd_kernel, dim3(b->count), dim3(SBI_THREADS), 0, ctx->stream, (const float*)scratch->im.tmpl,
                       (const float*)b->im.tmpl, b->g.w * b->g.h, b->ssd, (double*)ctx->d_pinned);
    HIP_TRY(hipGetLastError());
    SbiOut r;
    if (int rc = sbi_align(ctx, b->g, scratch->im.tmpl, b->im, b, 6, pin_ssd, &r)) return rc;
    if (ssd_out) std::memcpy(ssd_out, hp, (size_t)b->count * 8);
    out->best = r.best;
    out->best_ssd = r.best_ssd;
    out->align = r.a;
    // mse3Best = rotation * se3CfromW(best)
    const double* K = kf_poses12 + (size_t)r.best * 12;
    const double* R = r.a.rotation;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out->pose[3 * i + j] = R[3 * i] * K[j] + R[3 * i + 1] * K[3 + j] + R[3 * i + 2] * K[6 + j];
        out->pose[9 + i] = R[3 * i] * K[9] + R[3 * i + 1] * K[10] + R[3 * i + 2] * K[11];
    }
    out->good = r.a.score < max_score ? 1 : 0;
    return PTAM_OK;
}

__global__ __launch_bounds__(256) void motion_predict_sbi_kernel(int n, const ptam_motion_model* __restrict__ models, const double* __restrict__ rot,
                                                                 double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double R[9], pose[12];
    for (int k = 0; k < 9; k++) R[k] = rot[(size_t)i * 9 + k];
    motion_predict_sbi_hd(models[i].velocity, models[i].pose, R, pose);
    for (int k = 0; k < 12; k++) out[(size_t)i * 12 + k] = pose[k];
}

int ptam_motion_predict_sbi_dev(ptam_ctx* ctx, int n, const ptam_motion_model* models, const double* rotations9, double* poses_out12) {
    ARG_TRY(ctx && n >= 1 && n <= (1 << 20) && models && rotations9 && poses_out12);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t b_m = sbi_up256((size_t)n * sizeof(ptam_motion_model)), b_r = sbi_up256((size_t)n * 72), b_o = (size_t)n * 96;
    HIP_TRY(ptam_stream_wait(ctx->stream));   // (the scratch is nobody's)
    void* sc;
    if (int rc = ctx_scratch(ctx, b_m + b_r + b_o, &sc)) return rc;
    char* b = (char*)sc;
    HIP_TRY(hipMemcpy(b, models, (size_t)n * sizeof(ptam_motion_model), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b + b_m, rotations9, (size_t)n * 72, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(motion_predict_sbi_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, (const ptam_motion_model*)b,
                       (const double*)(b + b_m), (double*)(b + b_m + b_r));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(poses_out12, b + b_m + b_r, b_o, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    return PTAM_OK;
}

int ptam_rotation_estimator_create(ptam_ctx* ctx, int frame_w, int frame_h, double blur, ptam_rotation_estimator** out) {
    ARG_TRY(ctx && out && blur > 0.0 && blur <= 5.0);
    ptam_rotation_estimator* e = new ptam_rotation_estimator();
    e->ctx = ctx, e->blur = blur, e->last = -1, e->pending = -1;
    e->slot[0] = e->slot[1] = nullptr;
    for (int i = 0; i < 2; i++)
        if (int rc = ptam_sbi_create(ctx, frame_w, frame_h, &e->slot[i])) {
            ptam_sbi_destroy(e->slot[0]);
            delete e;
            return rc;
        }
    *out = e;
    return PTAM_OK;
}

int ptam_rotation_estimator_destroy(ptam_rotation_estimator* e) {
    if (!e) return PTAM_OK;
    ptam_sbi_destroy(e->slot[0]);
    ptam_sbi_destroy(e->slot[1]);
    delete e;
    return PTAM_OK;
}

int ptam_rotation_estimator_reset(ptam_rotation_estimator* e) {
    ARG_TRY(e);
    e->last = e->pending = -1;
    return PTAM_OK;
}

}   // extern "C"
