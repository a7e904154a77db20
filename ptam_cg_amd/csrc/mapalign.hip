// mapalign.hip — the last two host stages of MapMaker::InitFromStereo on flat map tables, fp64 throughout:
//   stage (8)  ApplyGlobalTransformationToMap(CalcPlaneAligner())   src/MapMaker.cc:397, bodies :463-472 and :1100-1195
//   stage (5)  RefreshSceneDepth of every keyframe                  src/MapMaker.cc:378-380, body :1202-1219
//
//   plane_score_kernel    ONE 256-THREAD WORKGROUP PER TRIAL (:1121-1143): the plane of the trial's three points, then the points in
//                         tiles of 256 — read flat (three coalesced fp64 loads per thread) into LDS, taken from there as xyz — and
//                         the clipped distances summed per thread in index order (stride 256), over the lanes by the DPP sum of
//                         common.h, over the four waves in order through LDS.  One score per trial, no atomics.
//   plane_finish_kernel   ONE WORKGROUP, everything after the trials in the order of :1144-1194: the argmin in trial order, the
//                         inlier flags, the mean and then the covariance about it (two passes, the same fixed-order sums), and in
//                         one lane the 3x3 eigenvectors by cyclic Jacobi, the rotation and the translation.  The result goes to
//                         device memory (the next kernel reads the aligner there) and into the host-mapped result block.
//   map_apply_kernel      one thread per keyframe and per point (:463-472): pose * aligner^-1 into a second pose table (the points'
//                         threads read the old one), aligner * point in place, and with a source table MapPoint::RefreshPixelVectors
//                         (src/Map.cc:40-65) against the source keyframe's new pose, which the thread works out itself.
//   scene_depth_kernel    one workgroup per keyframe (:1202-1219): its rows of the sorted measurement table by two binary searches,
//                         the depths and their squares summed in the same fixed order, the result into the host-mapped block.
// Every dot product below is the reference's expression, left to right and without FMA contraction (the pragma after the
// includes): the sums feed comparisons — a squared distance with zero, a distance with max_dist, one score with another.
#include <cfloat>

#include "map_stage.h"
#include "map_tables_check.h"

#pragma clang fp contract(off)

namespace {

struct PlaneOut {   // what the finish kernel publishes: 256 bytes, then (device only) the n inlier bytes
    ptam_plane_info info;
    double se3[12];
};
static_assert(sizeof(PlaneOut) <= 256, "the result header is 256 bytes");

struct PlaneArgs {
    int n, trials;
    double max_dist;
    const double* pts;        // n x 3
    const int32_t* samples;   // trials x 3
    double* scores;           // trials
    int* skipped;             // trials: 1 = the triple spans no plane
    uint8_t* flags;           // n, directly behind out
    PlaneOut* out;            // device
    PlaneOut* h_out;          // the same through host-mapped memory
};

struct ApplyArgs {
    int K, N;
    const PlaneOut* plane;    // status and se3NewFromOld, on the device
    const double* poses;      // K x 12 as they came
    double* poses_new;        // K x 12
    double* pts;              // N x 3, in place
    const ptam_map_point_source* src;   // N or null
    ptam_pvs_point* pvs;                // N or null
    int pvs_stride;                     // bytes from one output row to the next (sizeof(ptam_pvs_point), or the row of a wider table)
};

struct DepthArgs {
    int K, M;
    const double* poses;
    const double* pts;
    const ptam_map_meas* meas;
    ptam_scene_depth* out;    // host-mapped
};

}   // namespace

#define ALIGN_THREADS 256
#define ALIGN_WAVES (ALIGN_THREADS / 64)

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// :1121-1130 — v3Mean and the unit normal of the plane through the trial's three points; false where the normal's squared
// length is exactly zero (`continue`)
__device__ __forceinline__ bool plane_of_triple(const double* pts, const int32_t* s, double mean[3], double nrm[3]) {
    const double *A = pts + (size_t)3 * s[0], *B = pts + (size_t)3 * s[1], *C = pts + (size_t)3 * s[2];
    double ca[3], ba[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mean[k] = 0.33333333 * ((A[k] + B[k]) + C[k]);
        ca[k] = C[k] - A[k];
        ba[k] = B[k] - A[k];
    }
    nrm[0] = ca[1] * ba[2] - ca[2] * ba[1];
    nrm[1] = ca[2] * ba[0] - ca[0] * ba[2];
    nrm[2] = ca[0] * ba[1] - ca[1] * ba[0];
    const double nn = dot3(nrm, nrm);
    if (nn == 0.0) return false;
    const double len = sqrt(nn);
#pragma unroll
    for (int k = 0; k < 3; k++) nrm[k] /= len;
    return true;
}

// :1134-1138 — |v3Diff * v3Normal|, or a negative number for a point at the mean itself (dDistSq == 0.0: `continue`)
__device__ __forceinline__ double plane_dist(const double p[3], const double mean[3], const double nrm[3]) {
    const double d[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
    if (dot3(d, d) == 0.0) return -1.0;
    return fabs(dot3(d, nrm));
}

// sums over the workgroup in a fixed order: lanes by the DPP sum, then the four waves in order
template <int K>
__device__ __forceinline__ void align_block_sum(const double v[K], double (*red)[8], double* tot, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double s = wave_sum_f64(v[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < K) tot[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}

__global__ void __launch_bounds__(ALIGN_THREADS) plane_score_kernel(PlaneArgs g) {
    __shared__ double tile[3 * ALIGN_THREADS], red[ALIGN_WAVES][8], tot[8];
    const int tid = threadIdx.x, trial = blockIdx.x, n = g.n;
    double mean[3], nrm[3];
    if (!plane_of_triple(g.pts, g.samples + 3 * trial, mean, nrm)) {   // (the same for every thread of the workgroup)
        if (tid == 0) g.scores[trial] = 0.0, g.skipped[trial] = 1;
        return;
    }
    const size_t total = (size_t)3 * n;
    double acc[1] = {0.0};
    for (int base = 0; base < n; base += ALIGN_THREADS) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const size_t f = (size_t)3 * base + j * ALIGN_THREADS + tid;
            if (f < total) tile[j * ALIGN_THREADS + tid] = g.pts[f];
        }
        __syncthreads();
        if (base + tid < n) {
            const double p[3] = {tile[3 * tid], tile[3 * tid + 1], tile[3 * tid + 2]};
            const double d = plane_dist(p, mean, nrm);
            if (!(d < 0.0)) acc[0] += d > g.max_dist ? g.max_dist : d;   // (:1140-1142)
        }
        __syncthreads();
    }
    align_block_sum<1>(acc, red, tot, tid);
    if (tid == 0) g.scores[trial] = tot[0], g.skipped[trial] = 0;
}

// eigenvalues (ascending) and the unit eigenvector of the smallest of a symmetric 3x3 matrix, by cyclic Jacobi: SymEigen<3>'s
// get_evalues() and get_evectors()[0] up to the vector's sign, which the caller fixes
__device__ void sym_eigen3_smallest(const double c[6] /* xx xy xz yy yz zz */, double ev[3], double vec[3]) {
    double A[9] = {c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
    double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = A[p * 3 + q], app = A[p * 3 + p], aqq = A[q * 3 + q];
                if (apq == 0.0 || fabs(apq) <= DBL_EPSILON * sqrt(fabs(app * aqq))) continue;
                rotated = true;
                const double z = (aqq - app) / (2.0 * apq);
                const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                const int r = 3 - p - q;   // the third index
                const double arp = A[r * 3 + p], arq = A[r * 3 + q];
                A[p * 3 + p] = app - t * apq;
                A[q * 3 + q] = aqq + t * apq;
                A[p * 3 + q] = A[q * 3 + p] = 0.0;
                A[r * 3 + p] = A[p * 3 + r] = cs * arp - sn * arq;
                A[r * 3 + q] = A[q * 3 + r] = sn * arp + cs * arq;
                for (int i = 0; i < 3; i++) {
                    const double vp = V[i * 3 + p], vq = V[i * 3 + q];
                    V[i * 3 + p] = cs * vp - sn * vq;
                    V[i * 3 + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    int k = 0;
    for (int j = 1; j < 3; j++)
        if (A[j * 4] < A[k * 4]) k = j;   // (the first of equals)
    for (int i = 0; i < 3; i++) vec[i] = V[i * 3 + k], ev[i] = A[i * 4];
    double t;
    if (ev[1] < ev[0]) t = ev[0], ev[0] = ev[1], ev[1] = t;
    if (ev[2] < ev[1]) t = ev[1], ev[1] = ev[2], ev[2] = t;
    if (ev[1] < ev[0]) t = ev[0], ev[0] = ev[1], ev[1] = t;
}

__global__ void __launch_bounds__(ALIGN_THREADS) plane_finish_kernel(PlaneArgs g) {
    __shared__ double red[ALIGN_WAVES][8], tot[8], sbest[64], s_mean[3];
    __shared__ int sbesti[64], sskip[64], s_best;
    __shared__ PlaneOut s_out;
    const int tid = threadIdx.x, lane = tid & 63, n = g.n;
    auto publish = [&](int status) {   // thread 0: the aligner is the identity unless the status is OK
        s_out.info.status = status;
        if (status != PTAM_PLANE_OK)
            for (int j = 0; j < 12; j++) s_out.se3[j] = (j < 9 && j % 4 == 0) ? 1.0 : 0.0;
        *g.out = s_out;
        *g.h_out = s_out;
    };
    if (tid == 0) {
        s_out = PlaneOut{};
        s_out.info.n_points = n;
        s_out.info.best_trial = -1;
    }
    __syncthreads();
    if (n < 10) {   // :1103-1106
        if (tid == 0) publish(PTAM_PLANE_TOO_FEW);
        return;
    }

    // ---- the best trial (:1144-1148): the strictly smaller score wins, among equal scores the lowest trial ----
    if (tid < 64) {
        double b = 9999999999999999.9;   // dBestDistSquared (:1110)
        int bi = -1, ns = 0;
        for (int k = lane; k < g.trials; k += 64) {
            if (g.skipped[k]) {
                ns++;
                continue;
            }
            const double s = g.scores[k];
            if (s < b) b = s, bi = k;
        }
        sbest[lane] = b;
        sbesti[lane] = bi;
        sskip[lane] = ns;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            for (int l = 1; l < 64; l++) {
                ns += sskip[l];
                if (sbesti[l] >= 0 && (bi < 0 || sbest[l] < b || (sbest[l] == b && sbesti[l] < bi))) b = sbest[l], bi = sbesti[l];
            }
            s_best = bi;
            s_out.info.best_trial = bi;
            s_out.info.best_score = bi >= 0 ? b : 0.0;
            s_out.info.trials_skipped = ns;
        }
    }
    __syncthreads();
    if (s_best < 0) {   // no trial assigned v3BestMean / v3BestNormal
        if (tid == 0) publish(PTAM_PLANE_DEGENERATE);
        return;
    }
    double mean[3], nrm[3];
    plane_of_triple(g.pts, g.samples + 3 * s_best, mean, nrm);   // (the expressions of the scoring kernel: the same bits)

    // ---- the inlier set (:1152-1161) and its mean (:1164-1167) ----
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += ALIGN_THREADS) {
        const double p[3] = {g.pts[(size_t)3 * i], g.pts[(size_t)3 * i + 1], g.pts[(size_t)3 * i + 2]};
        const double d = plane_dist(p, mean, nrm);
        const bool in = d >= 0.0 && d < g.max_dist;
        g.flags[i] = in ? 1 : 0;
        if (in) acc[0] += p[0], acc[1] += p[1], acc[2] += p[2], acc[3] += 1.0;   // (a count below 2^53 is exact in fp64)
    }
    align_block_sum<4>(acc, red, tot, tid);   // (its barriers also publish the flags)
    const int n_inl = (int)tot[3];
    if (n_inl == 0) {
        if (tid == 0) {
            s_out.info.n_inliers = 0;
            publish(PTAM_PLANE_DEGENERATE);
        }
        return;
    }
    if (tid == 0) {
        const double inv = 1.0 / n_inl;
        for (int k = 0; k < 3; k++) s_mean[k] = tot[k] * inv;
    }
    __syncthreads();
    const double mi[3] = {s_mean[0], s_mean[1], s_mean[2]};

    // ---- the covariance about that mean (:1169-1173) ----
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += ALIGN_THREADS) {
        if (!g.flags[i]) continue;
        const double d[3] = {g.pts[(size_t)3 * i] - mi[0], g.pts[(size_t)3 * i + 1] - mi[1], g.pts[(size_t)3 * i + 2] - mi[2]};
        acc[0] += d[0] * d[0], acc[1] += d[0] * d[1], acc[2] += d[0] * d[2];
        acc[3] += d[1] * d[1], acc[4] += d[1] * d[2], acc[5] += d[2] * d[2];
    }
    align_block_sum<6>(acc, red, tot, tid);
    if (tid != 0) return;

    // ---- the normal, the rotation and the translation (:1176-1192) ----
    double cov[6], ev[3], v[3];
    for (int k = 0; k < 6; k++) cov[k] = tot[k];
    sym_eigen3_smallest(cov, ev, v);
    if (v[2] > 0.0)
        for (int k = 0; k < 3; k++) v[k] *= -1.0;
    ptam_plane_info& info = s_out.info;
    info.n_inliers = n_inl;
    for (int k = 0; k < 3; k++) info.mean[k] = mi[k], info.normal[k] = v[k], info.eigenvalues[k] = ev[k];
    const double ex[3] = {1.0, 0.0, 0.0};
    const double along = dot3(ex, v);
    double r0[3] = {ex[0] - v[0] * along, ex[1] - v[1] * along, ex[2] - v[2] * along};
    const double len_sq = dot3(r0, r0);
    if (len_sq == 0.0) {   // the normal along x: normalize() would divide by zero
        publish(PTAM_PLANE_DEGENERATE);
        return;
    }
    const double len = sqrt(len_sq);
    for (int k = 0; k < 3; k++) r0[k] /= len;
    const double r1[3] = {v[1] * r0[2] - v[2] * r0[1], v[2] * r0[0] - v[0] * r0[2], v[0] * r0[1] - v[1] * r0[0]};   // row2 ^ row0
    double* R = s_out.se3;
    for (int k = 0; k < 3; k++) R[k] = r0[k], R[3 + k] = r1[k], R[6 + k] = v[k];
    for (int k = 0; k < 3; k++) R[9 + k] = -(dot3(R + 3 * k, mi) + 0.0);   // -(se3Aligner * mean), the translation still zero
    publish(PTAM_PLANE_OK);
}

// ---- ApplyGlobalTransformationToMap (:463-472) -----------------------------------------------------------------------------------
// se3CfromW * se3NewFromOld.inverse(): TooN's inverse is (R^T, -(R^T t)), its product (Rl Rr, tl + Rl tr)
__device__ __forceinline__ void pose_times_inverse(const double P[12], const double T[12], double O[12]) {
    double it[3];
#pragma unroll
    for (int i = 0; i < 3; i++) it[i] = -((T[i] * T[9] + T[3 + i] * T[10]) + T[6 + i] * T[11]);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) O[r * 3 + c] = (P[r * 3] * T[c * 3] + P[r * 3 + 1] * T[c * 3 + 1]) + P[r * 3 + 2] * T[c * 3 + 2];
        O[9 + r] = P[9 + r] + dot3(P + 3 * r, it);
    }
}

__global__ void __launch_bounds__(ALIGN_THREADS) map_apply_kernel(ApplyArgs a) {
    const int gid = blockIdx.x * ALIGN_THREADS + threadIdx.x;
    const int status = a.plane->info.status;
    if (status == PTAM_PLANE_DEGENERATE) return;
    const bool move = status == PTAM_PLANE_OK;   // (too few points: the reference applies the identity)
    double T[12];
#pragma unroll
    for (int j = 0; j < 12; j++) T[j] = a.plane->se3[j];
    if (gid < a.K) {
        double O[12];
        if (move)
            pose_times_inverse(a.poses + (size_t)12 * gid, T, O);
        else
            for (int j = 0; j < 12; j++) O[j] = a.poses[(size_t)12 * gid + j];
        for (int j = 0; j < 12; j++) a.poses_new[(size_t)12 * gid + j] = O[j];
        return;
    }
    const int i = gid - a.K;
    if (i >= a.N) return;
    double* w = a.pts + (size_t)3 * i;
    double p[3] = {w[0], w[1], w[2]};
    if (move) {
        const double q[3] = {p[0], p[1], p[2]};
        for (int r = 0; r < 3; r++) p[r] = w[r] = dot3(T + 3 * r, q) + T[9 + r];
    }
    if (!a.src) return;
    // MapPoint::RefreshPixelVectors (src/Map.cc:40-65) with v3Normal_NC = (0, 0, -1)
    const ptam_map_point_source s = a.src[i];
    double P[12];
    if (move)
        pose_times_inverse(a.poses + (size_t)12 * s.src_kf, T, P);
    else
        for (int j = 0; j < 12; j++) P[j] = a.poses[(size_t)12 * s.src_kf + j];
    const double cam_h = fabs(dot3(P + 6, p) + P[11]);   // dCamHeight = |v3PlanePoint_C * v3Normal_NC|
    double right[3], down[3];
    for (int k = 0; k < 3; k++) {
        const double cen = s.center_nc[k] * cam_h / fabs(s.center_nc[2]);
        right[k] = s.one_right_nc[k] * cam_h / fabs(s.one_right_nc[2]) - cen;
        down[k] = s.one_down_nc[k] * cam_h / fabs(s.one_down_nc[2]) - cen;
    }
    ptam_pvs_point o;
    for (int k = 0; k < 3; k++) {   // se3CfromW.get_rotation().inverse() * difference
        o.world[k] = p[k];
        o.pixel_right_w[k] = (P[k] * right[0] + P[3 + k] * right[1]) + P[6 + k] * right[2];
        o.pixel_down_w[k] = (P[k] * down[0] + P[3 + k] * down[1]) + P[6 + k] * down[2];
    }
    *(ptam_pvs_point*)((char*)a.pvs + (size_t)i * a.pvs_stride) = o;
}

// ---- RefreshSceneDepth (:1202-1219) for keyframe blockIdx.x ------------------------------------------------------------------------
__device__ __forceinline__ int first_row_of(const ptam_map_meas* m, int M, int kf) {   // the first row whose kf is >= kf
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (m[mid].kf < kf) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(ALIGN_THREADS) scene_depth_kernel(DepthArgs a) {
    __shared__ double red[ALIGN_WAVES][8], tot[8];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int lo = first_row_of(a.meas, a.M, k), hi = first_row_of(a.meas, a.M, k + 1);
    const double* P = a.poses + (size_t)12 * k;
    double acc[2] = {0.0, 0.0};
    for (int i = lo + tid; i < hi; i += ALIGN_THREADS) {
        const double* w = a.pts + (size_t)3 * a.meas[i].point;
        const double z = dot3(P + 6, w) + P[11];   // (se3CfromW * v3WorldPos)[2]
        acc[0] += z;
        acc[1] += z * z;
    }
    align_block_sum<2>(acc, red, tot, tid);
    if (tid != 0) return;
    const int nm = hi - lo;
    ptam_scene_depth o;
    o.n_meas = nm;
    o.pad_ = 0;
    o.depth_mean = o.depth_sigma = 0.0;
    if (nm > 0) {
        o.depth_mean = tot[0] / nm;
        const double rad = tot[1] / nm - o.depth_mean * o.depth_mean;
        o.depth_sigma = rad < 0.0 ? 0.0 : sqrt(rad);   // (a radicand that rounding made negative)
    }
    a.out[k] = o;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static inline uint64_t splitmix64_next(uint64_t& state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void plane_draw(uint64_t seed, int n, int trials, int32_t* out) {   // the draw of :1113-1119 with rand() replaced
    uint64_t state = seed;
    for (int r = 0; r < trials; r++) {
        int32_t* s = out + 3 * r;
        s[0] = (int32_t)(splitmix64_next(state) % (uint64_t)n);
        do s[1] = (int32_t)(splitmix64_next(state) % (uint64_t)n);
        while (s[1] == s[0]);
        do s[2] = (int32_t)(splitmix64_next(state) % (uint64_t)n);
        while (s[2] == s[0] || s[2] == s[1]);
    }
}

int map_plane_check(int n, const ptam_plane_opts* o) {
    ARG_TRY(o && n >= 0 && o->trials >= 1 && o->max_dist > 0.0);
    if (o->samples && n >= 10)   // (below ten points nothing is drawn, :1103-1106)
        for (int r = 0; r < o->trials; r++) {
            const int32_t* s = o->samples + 3 * r;
            for (int i = 0; i < 3; i++) ARG_TRY(s[i] >= 0 && s[i] < n);
            ARG_TRY(s[0] != s[1] && s[0] != s[2] && s[1] != s[2]);
        }
    return PTAM_OK;
}
static int plane_check(int n, const double* points3, const ptam_plane_opts* o) {
    ARG_TRY(n <= 0 || points3);
    return map_plane_check(n, o);
}
static int tables_check(int K, const double* poses, int N, const double* points3, const ptam_map_point_source* src, const ptam_pvs_point* out) {
    ARG_TRY(K >= 0 && N >= 0 && (K == 0 || poses) && (N == 0 || points3));
    ARG_TRY((src == nullptr) == (out == nullptr));
    if (src)
        for (int i = 0; i < N; i++) ARG_TRY(src[i].src_kf >= 0 && src[i].src_kf < K);
    return PTAM_OK;
}

// ---- the stage's cores: tables in device memory, launches on the stage's stream, no wait (map_stage.h) -----------------------------
void map_plane_layout(Carver& c, Carver& pin, int n, int trials, MapPlaneWork& w) {
    const size_t Nz = n > 0 ? n : 1, Tz = trials > 0 ? trials : 1;
    w.d_samples = c.piece<int32_t>(Tz * 3);
    w.scores = c.piece<double>(Tz);
    w.skipped = c.piece<int>(Tz);
    w.d_record = c.piece<char>(256 + Nz);
    w.h_samples = pin.piece<int32_t>(Tz * 3);
    w.h_record = pin.piece<char>(256);
}
int map_plane_core(MapStage& s, const MapPlaneWork& w, const ptam_plane_opts* o, int n, const double* d_points3) {
    PlaneArgs g;
    g.n = n;
    g.trials = o->trials;
    g.max_dist = o->max_dist;
    g.pts = d_points3;
    g.samples = w.d_samples;
    g.scores = w.scores;
    g.skipped = w.skipped;
    g.out = (PlaneOut*)w.d_record;
    g.flags = (uint8_t*)w.d_record + 256;
    g.h_out = s.pin_dev((PlaneOut*)w.h_record);
    if (n >= 10) {
        if (o->samples)
            std::memcpy(w.h_samples, o->samples, (size_t)o->trials * 3 * sizeof(int32_t));
        else
            plane_draw(o->seed, n, o->trials, w.h_samples);
        STAGE_TRY(s.up(w.d_samples, w.h_samples, (size_t)o->trials * 3 * sizeof(int32_t)));
        hipLaunchKernelGGL(plane_score_kernel, dim3(o->trials), dim3(ALIGN_THREADS), 0, s.st, g);
    }
    hipLaunchKernelGGL(plane_finish_kernel, dim3(1), dim3(ALIGN_THREADS), 0, s.st, g);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
void map_plane_result(const MapPlaneWork& w, ptam_plane_info* info, double se3_aligner[12]) {
    const PlaneOut* r = (const PlaneOut*)w.h_record;
    *info = r->info;
    std::memcpy(se3_aligner, r->se3, sizeof r->se3);
}
int map_record_up(MapStage& s, void* d_record, void* h_record, int status, const double se3_new_from_old[12]) {
    PlaneOut* h_out = (PlaneOut*)h_record;
    *h_out = PlaneOut{};
    h_out->info.status = status;
    std::memcpy(h_out->se3, se3_new_from_old, sizeof h_out->se3);
    return s.up(d_record, h_out, sizeof(PlaneOut));
}
// poses -> poses_new, the points in place, the pixel vectors (d_src / d_pvs nullable together) into rows pvs_stride bytes apart
int map_apply_core(MapStage& s, const void* d_record, int K, const double* d_poses, double* d_poses_new, int N, double* d_points3,
                   const ptam_map_point_source* d_src, ptam_pvs_point* d_pvs, int pvs_stride) {
    ApplyArgs a;
    a.K = K;
    a.N = N;
    a.plane = (const PlaneOut*)d_record;
    a.poses = d_poses;
    a.poses_new = d_poses_new;
    a.pts = d_points3;
    a.src = d_src;
    a.pvs = d_pvs;
    a.pvs_stride = pvs_stride;
    hipLaunchKernelGGL(map_apply_kernel, dim3((K + N + ALIGN_THREADS - 1) / ALIGN_THREADS), dim3(ALIGN_THREADS), 0, s.st, a);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}
// ptam_map_apply_global_transform's launch on tables that are in device memory.  d_record / h_record: 256 bytes each of the caller's
// stage (scratch, pinned) for the aligner's record.  Enqueues only; K + N > 0.
int map_transform_core(MapStage& s, void* d_record, void* h_record, const double se3_new_from_old[12], int K, const double* d_poses,
                       double* d_poses_new, int N, double* d_points3, const ptam_map_point_source* d_src, ptam_pvs_point* d_pvs, int pvs_stride) {
    STAGE_TRY(map_record_up(s, d_record, h_record, PTAM_PLANE_OK, se3_new_from_old));
    return map_apply_core(s, d_record, K, d_poses, d_poses_new, N, d_points3, d_src, d_pvs, pvs_stride);
}

// The three calls of stage (8) are one routine: the plane stage when `o` is given (else the aligner is se3_in), the apply stage when
// `apply`.  Arguments checked by the caller.  Uploads, up to three launches (the cores above), the copies down, one host wait.
static int align_run(ptam_ctx* ctx, const ptam_plane_opts* o, const double* se3_in, bool apply, int K, double* poses, int N, double* pts,
                     const ptam_map_point_source* src, ptam_pvs_point* pvs, double se3_out[12], ptam_plane_info* info, uint8_t* inlier_out) {
    const size_t Kz = K > 0 ? K : 1, Nz = N > 0 ? N : 1;
    MapPlaneWork w;
    double *d_pts, *d_pose, *d_pose_new;
    ptam_map_point_source* d_src;
    ptam_pvs_point* d_pvs;
    char *t_pose = nullptr, *t_pts = nullptr, *t_pvs = nullptr;   // where the tables come down, in the pinned staging
    MapStage stage(ctx);
    STAGE_TRY(stage.carve([&](Carver& c, Carver& pin) {
        map_plane_layout(c, pin, N, o ? o->trials : 0, w);
        d_pts = c.piece<double>(Nz * 3);
        d_pose = c.piece<double>(Kz * 12);
        d_pose_new = c.piece<double>(Kz * 12);
        d_src = c.piece<ptam_map_point_source>(Nz);
        d_pvs = c.piece<ptam_pvs_point>(Nz);
        if (apply) {
            t_pose = pin.piece<char>(Kz * 96);
            t_pts = pin.piece<char>(Nz * 24);
            t_pvs = pin.piece<char>(src ? Nz * sizeof(ptam_pvs_point) : 0);
        }
    }));
    hipStream_t st = stage.st;
    STAGE_TRY(stage.up(d_pts, pts, (size_t)N * 24));
    if (o)
        STAGE_TRY(map_plane_core(stage, w, o, N, d_pts));
    else   // the caller's aligner takes the plane stage's place
        STAGE_TRY(map_record_up(stage, w.d_record, w.h_record, PTAM_PLANE_OK, se3_in));
    if (apply && K + N > 0) {
        STAGE_TRY(stage.up(d_pose, poses, (size_t)K * 96));
        if (src) STAGE_TRY(stage.up(d_src, src, (size_t)N * sizeof(ptam_map_point_source)));
        STAGE_TRY(map_apply_core(stage, w.d_record, K, d_pose, d_pose_new, N, d_pts, src ? d_src : nullptr, src ? d_pvs : nullptr,
                                 (int)sizeof(ptam_pvs_point)));
    }
    // what the status decides about (the tables, the pixel vectors) comes down into the context's pinned staging and reaches the
    // caller's memory after the wait; the inlier bytes go there directly
    if (apply) {
        STAGE_TRY(stage.down(t_pose, d_pose_new, (size_t)K * 96));
        STAGE_TRY(stage.down(t_pts, d_pts, (size_t)N * 24));
        if (src) STAGE_TRY(stage.down(t_pvs, d_pvs, (size_t)N * sizeof(ptam_pvs_point)));
    }
    if (o && inlier_out && N >= 10) STAGE_TRY(stage.down(inlier_out, w.d_record + 256, (size_t)N));
    HIP_TRY(ptam_stream_wait(st));
    int status = PTAM_PLANE_OK;
    if (o) {
        map_plane_result(w, info, se3_out);
        status = info->status;
        if (inlier_out && (N < 10 || info->best_trial < 0)) std::memset(inlier_out, 0, (size_t)N);   // (no inlier pass ran)
    }
    if (apply && status == PTAM_PLANE_OK) {
        if (K > 0) std::memcpy(poses, t_pose, (size_t)K * 96);
        if (N > 0) std::memcpy(pts, t_pts, (size_t)N * 24);
    }
    if (apply && src && N > 0 && status != PTAM_PLANE_DEGENERATE) std::memcpy(pvs, t_pvs, (size_t)N * sizeof(ptam_pvs_point));
    return PTAM_OK;
}

extern "C" {

void ptam_plane_opts_default(ptam_plane_opts* o) {
    if (!o) return;
    o->max_dist = 0.05;
    o->trials = 100;
    o->seed = 0;
    o->samples = nullptr;
}

int ptam_plane_samples(uint64_t seed, int n_points, int trials, int32_t* out) {
    ARG_TRY(out && n_points >= 3 && trials >= 1);
    plane_draw(seed, n_points, trials, out);
    return PTAM_OK;
}

int ptam_calc_plane_aligner(ptam_ctx* ctx, int n_points, const double* points3, const ptam_plane_opts* opts, double se3_aligner[12],
                            ptam_plane_info* info, uint8_t* inlier_out) {
    ARG_TRY(ctx && opts && se3_aligner && info);
    if (int rc = plane_check(n_points, points3, opts)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return align_run(ctx, opts, nullptr, false, 0, nullptr, n_points, const_cast<double*>(points3), nullptr, nullptr, se3_aligner, info, inlier_out);
}

int ptam_map_apply_global_transform(ptam_ctx* ctx, const double se3_new_from_old[12], int n_kf, double* kf_poses12, int n_points,
                                    double* points3, const ptam_map_point_source* sources, ptam_pvs_point* out) {
    ARG_TRY(ctx && se3_new_from_old);
    if (int rc = tables_check(n_kf, kf_poses12, n_points, points3, sources, out)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return align_run(ctx, nullptr, se3_new_from_old, true, n_kf, kf_poses12, n_points, points3, sources, out, nullptr, nullptr, nullptr);
}

int ptam_map_align_to_plane(ptam_ctx* ctx, const ptam_plane_opts* opts, int n_kf, double* kf_poses12, int n_points, double* points3,
                            const ptam_map_point_source* sources, ptam_pvs_point* out, double se3_aligner[12], ptam_plane_info* info,
                            uint8_t* inlier_out) {
    ARG_TRY(ctx && opts && se3_aligner && info);
    if (int rc = plane_check(n_points, points3, opts)) return rc;
    if (int rc = tables_check(n_kf, kf_poses12, n_points, points3, sources, out)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return align_run(ctx, opts, nullptr, true, n_kf, kf_poses12, n_points, points3, sources, out, se3_aligner, info, inlier_out);
}

int ptam_map_scene_depth(ptam_ctx* ctx, int n_kf, const double* kf_poses12, int n_points, const double* points3, int n_meas,
                         const ptam_map_meas* meas, ptam_scene_depth* out) {
    ARG_TRY(ctx && n_kf >= 0 && n_points >= 0 && n_meas >= 0);
    ARG_TRY((n_kf == 0 || (kf_poses12 && out)) && (n_points == 0 || points3) && (n_meas == 0 || meas));
    ARG_TRY(mc_sorted_in_range(n_meas, meas, n_kf, n_points));
    if (n_kf == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    double *d_pose, *d_pts;
    ptam_map_meas* d_meas;
    ptam_scene_depth* h_out;
    MapStage s(ctx);
    STAGE_TRY(s.carve([&](Carver& c, Carver& pin) {
        d_pose = c.piece<double>((size_t)n_kf * 12);
        d_pts = c.room<double>((size_t)n_points * 3);
        d_meas = c.room<ptam_map_meas>((size_t)n_meas);
        h_out = pin.piece<ptam_scene_depth>((size_t)n_kf);   // where the kernel writes the result
    }));
    STAGE_TRY(s.up(d_pose, kf_poses12, (size_t)n_kf * 96));
    STAGE_TRY(s.up(d_pts, points3, (size_t)n_points * 24));
    STAGE_TRY(s.up(d_meas, meas, (size_t)n_meas * sizeof(ptam_map_meas)));
    return map_scene_depth_core(s, n_kf, d_pose, d_pts, n_meas, d_meas, h_out, out);
}

}   // extern "C"

// the launch and the wait of ptam_map_scene_depth on tables that are in device memory (n_kf > 0); h_out: n_kf records of the
// caller's pinned stage, which the kernel writes through their device address; out: host
int map_scene_depth_core(MapStage& s, int n_kf, const double* d_poses, const double* d_points3, int n_meas, const ptam_map_meas* d_meas,
                         ptam_scene_depth* h_out, ptam_scene_depth* out) {
    DepthArgs a;
    a.K = n_kf;
    a.M = n_meas;
    a.poses = d_poses;
    a.pts = d_points3;
    a.meas = d_meas;
    a.out = s.pin_dev(h_out);
    hipLaunchKernelGGL(scene_depth_kernel, dim3(n_kf), dim3(ALIGN_THREADS), 0, s.st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(s.st));
    std::memcpy(out, h_out, (size_t)n_kf * sizeof(ptam_scene_depth));
    return PTAM_OK;
}

void mapalign_preload_kernels() {
    ptam_preload((const void*)plane_score_kernel);
    ptam_preload((const void*)plane_finish_kernel);
    ptam_preload((const void*)map_apply_kernel);
    ptam_preload((const void*)scene_depth_kernel);
}
