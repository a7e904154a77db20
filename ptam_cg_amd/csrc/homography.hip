// homography.hip — HomographyInit::Compute (src/HomographyInit.cc) on gfx950, fp64 throughout.  Two launches:
//   homog_mlesac_kernel   ONE WAVE PER TRIAL (:195-229): the 8x9 system of the trial's four matches, one row per lane, next to the
//                         nine rows of V (wave_null_vector); the null vector is the trial's homography; then the lanes stride over
//                         all matches and the MLESAC scores are summed in a fixed order (per lane in index order, then the DPP
//                         sum of common.h).  The trial's score and its H go to the workspace.  No atomics.
//   homog_finish_kernel   ONE WORKGROUP of four waves, everything after the trials in the order of Compute (:35-63): the argmin
//                         over (score, trial) — or, below ten matches, the DLT over all of them by the same wave routine —, the
//                         inlier flags, five RefineHomographyWithInliers, DecomposeHomography, ChooseBestDecomposition.  Work
//                         per match is strided over the 256 threads and reduced wave by wave in a fixed order; what the
//                         reference does once (the 9x9 solve, the 3x3 SVD, the sorts of eight) is done by thread 0 on LDS.
// The median of the refinement is found by rank: an inlier's rank is the number of inliers ordered before it by (value, index),
// and the one of rank n / 2 is sorted[n / 2].  n^2 / 256 comparisons per thread (4 k at a thousand matches) on values every lane
// reads at the same address — exact for any n, no sort buffer, no dependence on the pose kernels' shared state.
#include "homography.h"

#include <cfloat>

namespace {

struct HomogOut {   // what comes back: 256 bytes, then the n inlier bytes
    ptam_homography_info info;
    double se3[12];
};
static_assert(sizeof(HomogOut) <= 256, "the read-back header is 256 bytes");

struct HomogArgs {
    int n, trials;
    double max_sq;
    const ptam_homography_match* m;
    const int32_t* samples;   // trials x 4
    double* scores;           // trials
    double* hs;               // trials x 9
    double* err2;             // n
    uint8_t* flags;           // n, directly behind out
    HomogOut* out;
};

struct Decomp {   // HomographyDecomposition (include/HomographyInit.h): d, v3n, se3SecondFromFirst
    double d, nrm[3], R[9], t[3];
};

}   // namespace

#define HOMOG_THREADS 256
#define HOMOG_WAVES (HOMOG_THREADS / 64)
#define HOMOG_NACC 54   // 45 entries of the upper triangle of J^T W J + 9 of J^T W e

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// dSquaredError of IsHomographyInlier / MLESACScore (:14-33)
__device__ __forceinline__ double homog_pixel_error_sq(const double H[9], const ptam_homography_match& m) {
    const double x = m.first[0], y = m.first[1];
    const double p0 = H[0] * x + H[1] * y + H[2], p1 = H[3] * x + H[4] * y + H[5], p2 = H[6] * x + H[7] * y + H[8];
    const double ex = m.second[0] - p0 / p2, ey = m.second[1] - p1 / p2;
    const double a = m.jac[0] * ex + m.jac[1] * ey, b = m.jac[2] * ex + m.jac[3] * ey;
    return a * a + b * b;
}

// one row of HomographyFromMatches' matrix (:73-101): odd = the v row
__device__ __forceinline__ void homog_dlt_row(const ptam_homography_match& m, bool odd, double a[9]) {
    const double x = m.first[0], y = m.first[1], u = odd ? m.second[1] : m.second[0];
    a[0] = odd ? 0.0 : x;
    a[1] = odd ? 0.0 : y;
    a[2] = odd ? 0.0 : 1.0;
    a[3] = odd ? x : 0.0;
    a[4] = odd ? y : 0.0;
    a[5] = odd ? 1.0 : 0.0;
    a[6] = -x * u;
    a[7] = -y * u;
    a[8] = -u;
}

// The right singular vector of the smallest singular value of a matrix of up to 32 rows and nine columns, by one wave: one-sided
// Jacobi as in mapmaker_device.h (Hestenes: column pairs are rotated until they are orthogonal), with lane r < 32 holding row r
// of the matrix (rows that do not exist are zero, which changes nothing) and lane 32 + i row i of V.  A rotation touches every
// row on its own; the three column products are sums over the matrix lanes.  Every lane returns the same h.
__device__ __forceinline__ void wave_null_vector(double a[9], int lane, double h[9]) {
    const bool is_a = lane < 32;
    if (!is_a) {
#pragma unroll
        for (int j = 0; j < 9; j++) a[j] = (lane - 32 == j) ? 1.0 : 0.0;
    }
    // A column that has become the null vector's holds rounding noise only (norm <= 8 eps |A|_F): it is never orthogonal to
    // the others to within eps of ITS norm, and rotating it on would use all 30 sweeps (four matches determine H exactly) for
    // nothing — the null vector is the same to the last digits (checked in numpy: 6 sweeps instead of 30).
    double fro = 0.0;
#pragma unroll
    for (int j = 0; j < 9; j++) fro += is_a ? a[j] * a[j] : 0.0;
    const double tiny = 64.0 * DBL_EPSILON * DBL_EPSILON * wave_sum_f64(fro);
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 8; p++)
#pragma unroll
            for (int q = p + 1; q < 9; q++) {
                const double al = wave_sum_f64(is_a ? a[p] * a[p] : 0.0), be = wave_sum_f64(is_a ? a[q] * a[q] : 0.0),
                             ga = wave_sum_f64(is_a ? a[p] * a[q] : 0.0);
                if (ga == 0.0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be) || fmin(al, be) <= tiny) continue;   // (wave-uniform)
                rotated = true;
                const double z = (be - al) / (2.0 * ga);
                const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                const double ap = a[p], aq = a[q];
                a[p] = c * ap - s * aq;
                a[q] = s * ap + c * aq;
            }
        if (!rotated) break;
    }
    double best = 0.0, col = 0.0;   // the column of V under the matrix column of least norm (the first of equals)
#pragma unroll
    for (int j = 0; j < 9; j++) {
        const double nn = wave_sum_f64(is_a ? a[j] * a[j] : 0.0);
        if (j == 0 || nn < best) best = nn, col = a[j];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = readlane_f64(col, 32 + i);
}

__global__ void __launch_bounds__(HOMOG_THREADS) homog_mlesac_kernel(HomogArgs g) {
    const int lane = threadIdx.x & 63;
    const int trial = blockIdx.x * HOMOG_WAVES + (threadIdx.x >> 6);
    if (trial >= g.trials) return;
    double a[9];
#pragma unroll
    for (int j = 0; j < 9; j++) a[j] = 0.0;
    if (lane < 8) homog_dlt_row(g.m[g.samples[trial * 4 + (lane >> 1)]], lane & 1, a);   // (indices checked on the host)
    double H[9];
    wave_null_vector(a, lane, H);
    double acc = 0.0;
    for (int i = lane; i < g.n; i += 64) {
        const double e2 = homog_pixel_error_sq(H, g.m[i]);
        acc += e2 > g.max_sq ? g.max_sq : e2;
    }
    const double score = wave_sum_f64(acc);
    if (lane == 0) {
        g.scores[trial] = score;
#pragma unroll
        for (int j = 0; j < 9; j++) g.hs[trial * 9 + j] = H[j];
    }
}

// ---- sums over the workgroup in a fixed order: lanes by the DPP sum, then the four waves in order --------------------------------
template <int K>
__device__ __forceinline__ void block_sum_f64(const double v[K], double (*red)[HOMOG_NACC], double* tot, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double s = wave_sum_f64(v[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < K) tot[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}
template <int K>
__device__ __forceinline__ void block_sum_i32(const int v[K], int (*red)[8], int* tot, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int s = wave_sum_i32(v[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < K) tot[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    __syncthreads();
}

// n (<= 8) indices into the order of a stable sort by ascending score (nScore = -nPositive): an insertion sort that moves an
// element only past strictly larger ones, which is what std::sort does below 16 elements
__device__ __forceinline__ void stable_sort_by_score(int* order, int* score, int n) {
    for (int i = 1; i < n; i++) {
        const int o = order[i], s = score[i];
        int j = i;
        for (; j > 0 && s < score[j - 1]; j--) order[j] = order[j - 1], score[j] = score[j - 1];
        order[j] = o;
        score[j] = s;
    }
}

// SVD of a 3x3 matrix by one-sided Jacobi: H = U diag(sg) V^T, sg descending (LAPACK's order)
__device__ __forceinline__ void svd3(const double H[9], double U[9], double sg[3], double V[9]) {
    double A[9];
#pragma unroll
    for (int i = 0; i < 9; i++) A[i] = H[i], V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    al += A[i * 3 + p] * A[i * 3 + p];
                    be += A[i * 3 + q] * A[i * 3 + q];
                    ga += A[i * 3 + p] * A[i * 3 + q];
                }
                if (ga == 0.0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be)) continue;
                rotated = true;
                const double z = (be - al) / (2.0 * ga);
                const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double ap = A[i * 3 + p], aq = A[i * 3 + q];
                    A[i * 3 + p] = c * ap - s * aq;
                    A[i * 3 + q] = s * ap + c * aq;
                    const double vp = V[i * 3 + p], vq = V[i * 3 + q];
                    V[i * 3 + p] = c * vp - s * vq;
                    V[i * 3 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) sg[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    auto order = [&](int p, int q) {   // columns p < q: the larger singular value first
        if (sg[p] < sg[q]) {
            double t = sg[p];
            sg[p] = sg[q], sg[q] = t;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                t = A[i * 3 + p], A[i * 3 + p] = A[i * 3 + q], A[i * 3 + q] = t;
                t = V[i * 3 + p], V[i * 3 + p] = V[i * 3 + q], V[i * 3 + q] = t;
            }
        }
    };
    order(0, 1);
    order(1, 2);
    order(0, 1);
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) U[i * 3 + j] = A[i * 3 + j] / sg[j];
    if (sg[2] == 0.0) {   // a singular H has no third column in A: the one that completes U
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}
__device__ __forceinline__ double det3(const double M[9]) {   // Tools::M3Det
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// DecomposeHomography (:232-339) by one thread: the eight solutions into dec[] (LDS) in push order; false where nCase != 1
__device__ bool homog_decompose(const double H[9], Decomp* dec) {
    double U[9], V[9], sg[3];
    svd3(H, U, sg, V);
    const double d1 = fabs(sg[0]), d2 = fabs(sg[1]), d3 = fabs(sg[2]);
    const double s = det3(U) * det3(V);
    if (!(d1 != d2 && d2 != d3)) return false;
    const double x1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), x3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    for (int k = 0; k < 8; k++) {
        const double e1 = (k & 1) ? -1.0 : 1.0, e3 = (k & 2) ? -1.0 : 1.0;
        const bool neg = k >= 4;   // Case 1, d' < 0 (:305-329)
        double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, Tp[3];
        if (!neg) {
            const double sn = (d1 - d3) * x1 * x3 * e1 * e3 / d2, cs = (d1 * x3 * x3 + d3 * x1 * x1) / d2;
            Rp[0] = cs, Rp[2] = -sn, Rp[6] = sn, Rp[8] = cs;
            Tp[0] = (d1 - d3) * x1 * e1, Tp[1] = 0.0, Tp[2] = (d1 - d3) * -x3 * e3;
        } else {
            const double sn = (d1 + d3) * x1 * x3 * e1 * e3 / d2, cs = (d3 * x1 * x1 - d1 * x3 * x3) / d2;
            Rp[0] = cs, Rp[2] = sn, Rp[4] = -1.0, Rp[6] = sn, Rp[8] = -cs;
            Tp[0] = (d1 + d3) * x1 * e1, Tp[1] = 0.0, Tp[2] = (d1 + d3) * x3 * e3;
        }
        Decomp D;
        D.d = neg ? s * -d2 : s * d2;
        const double np0 = x1 * e1, np2 = x3 * e3;   // v3np = (x1 e1, 0, x3 e3)
        double M[9];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            D.nrm[i] = V[i * 3] * np0 + V[i * 3 + 2] * np2;
            D.t[i] = U[i * 3] * Tp[0] + U[i * 3 + 2] * Tp[2];
#pragma unroll
            for (int j = 0; j < 3; j++) M[i * 3 + j] = s * (U[i * 3] * Rp[j] + U[i * 3 + 1] * Rp[3 + j] + U[i * 3 + 2] * Rp[6 + j]);
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) D.R[i * 3 + j] = M[i * 3] * V[j * 3] + M[i * 3 + 1] * V[j * 3 + 1] + M[i * 3 + 2] * V[j * 3 + 2];
        dec[k] = D;
    }
    return true;
}

// SampsonusError (:346-360) of one match under the essential matrix E
__device__ __forceinline__ double homog_sampson(const double* E, const ptam_homography_match& m) {
    const double xd = m.second[0], yd = m.second[1], x = m.first[0], y = m.first[1];
    const double f0 = E[0] * x + E[1] * y + E[2], f1 = E[3] * x + E[4] * y + E[5], f2 = E[6] * x + E[7] * y + E[8];
    const double g0 = E[0] * xd + E[3] * yd + E[6], g1 = E[1] * xd + E[4] * yd + E[7];
    const double err = xd * f0 + yd * f1 + f2;
    return err * err / ((f0 * f0 + f1 * f1) + (g0 * g0 + g1 * g1));
}

__global__ void __launch_bounds__(HOMOG_THREADS) homog_finish_kernel(HomogArgs g) {
    __shared__ double sH[9], red[HOMOG_WAVES][HOMOG_NACC], tot[HOMOG_NACC], sC[81], sx[9], sE[2][9], sbest[64], smed;
    __shared__ int sbesti[64], ired[HOMOG_WAVES][8], itot[8], order[8], score[8], s_flag[2];
    __shared__ Decomp dec[8];
    const int tid = threadIdx.x, lane = tid & 63, n = g.n;
    ptam_homography_info* info = &g.out->info;

    // ---- BestHomographyFromMatches_MLESAC (:179-230) ----
    if (tid < 64) {
        if (n < 10) {
            double a[9];
#pragma unroll
            for (int j = 0; j < 9; j++) a[j] = 0.0;
            if (lane < 2 * n) homog_dlt_row(g.m[lane >> 1], lane & 1, a);   // (2n <= 18 rows)
            double H[9];
            wave_null_vector(a, lane, H);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < 9; j++) sH[j] = H[j];
                info->best_trial = -1;
                info->best_score = 0.0;
            }
        } else {
            double b = 999999999999999999.9;   // dBestError (:192)
            int bi = -1;
            for (int k = lane; k < g.trials; k += 64) {
                const double s = g.scores[k];
                if (s < b) b = s, bi = k;
            }
            sbest[lane] = b;
            sbesti[lane] = bi;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                for (int l = 1; l < 64; l++)   // the lowest trial among the smallest scores
                    if (sbesti[l] >= 0 && (bi < 0 || sbest[l] < b || (sbest[l] == b && sbesti[l] < bi))) b = sbest[l], bi = sbesti[l];
                for (int j = 0; j < 9; j++) sH[j] = bi >= 0 ? g.hs[bi * 9 + j] : (j % 4 == 0 ? 1.0 : 0.0);   // mm3BestHomography = Identity (:191)
                info->best_trial = bi;
                info->best_score = b;
            }
        }
    }
    __syncthreads();

    // ---- the inlier set (:44-47) ----
    double H[9];
#pragma unroll
    for (int j = 0; j < 9; j++) H[j] = sH[j];
    int cnt[1] = {0};
    for (int i = tid; i < n; i += HOMOG_THREADS) {
        const bool in = homog_pixel_error_sq(H, g.m[i]) < g.max_sq;
        g.flags[i] = in ? 1 : 0;
        cnt[0] += in ? 1 : 0;
    }
    block_sum_i32<1>(cnt, ired, itot, tid);   // (its barriers also publish the flags)
    const int n_inl = itot[0];
    if (tid == 0) {
        info->n_matches = n;
        info->n_inliers = n_inl;
        info->ambiguous = 0;
        info->sampson[0] = info->sampson[1] = 0.0;
        info->status = PTAM_HOMOG_OK;
    }
    if (n_inl == 0) {
        if (tid == 0) {
            info->status = PTAM_HOMOG_NO_INLIERS;
            for (int j = 0; j < 9; j++) info->homography[j] = sH[j];
        }
        return;
    }

    // ---- five RefineHomographyWithInliers (:120-177) ----
    for (int it = 0; it < 5; it++) {
#pragma unroll
        for (int j = 0; j < 9; j++) H[j] = sH[j];
        if (tid == 0) smed = __longlong_as_double(0x7ff8000000000000ll);
        for (int i = tid; i < n; i += HOMOG_THREADS)
            if (g.flags[i]) g.err2[i] = homog_pixel_error_sq(H, g.m[i]);   // v2Error * v2Error: the same expression
        __syncthreads();
        for (int i = tid; i < n; i += HOMOG_THREADS) {   // Tukey::FindSigmaSquared's median: sorted[n / 2], by rank
            if (!g.flags[i]) continue;
            const double v = g.err2[i];
            int rank = 0;
            for (int j = 0; j < n; j++) {
                const double vj = g.err2[j];
                rank += (g.flags[j] && (vj < v || (vj == v && j < i))) ? 1 : 0;
            }
            if (rank == n_inl / 2) smed = v;
        }
        __syncthreads();
        const double sigma_sq = est_sigma_sq_from_median(PTAM_EST_TUKEY, smed, (unsigned long long)n_inl);
        double acc[HOMOG_NACC];
#pragma unroll
        for (int k = 0; k < HOMOG_NACC; k++) acc[k] = 0.0;
        for (int i = tid; i < n; i += HOMOG_THREADS) {
            if (!g.flags[i]) continue;
            const ptam_homography_match m = g.m[i];
            const double x = m.first[0], y = m.first[1];
            const double s0 = H[0] * x + H[1] * y + H[2], s1 = H[3] * x + H[4] * y + H[5], s2 = H[6] * x + H[7] * y + H[8];
            const double ex = m.second[0] - s0 / s2, ey = m.second[1] - s1 / s2;
            const double e[2] = {m.jac[0] * ex + m.jac[1] * ey, m.jac[2] * ex + m.jac[3] * ey};
            // (a zero error has the full weight: with a zero median — four matches determine H exactly, and three of their errors
            //  can round to nothing — the reference's 1 - 0 / 0 is a NaN that ends in a NaN pose; ptam_hip.h)
            const double w = g.err2[i] == 0.0 ? 1.0 : est_weight(PTAM_EST_TUKEY, g.err2[i], sigma_sq);
            const double u[3] = {x, y, 1.0}, dd = s2 * s2;
            double J[2][9];   // m2PixelProjectionJac * m29Jacobian
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double a = u[c] / s2, bx = -u[c] * s0 / dd, by = -u[c] * s1 / dd;
                J[0][c] = m.jac[0] * a;
                J[0][3 + c] = m.jac[1] * a;
                J[0][6 + c] = m.jac[0] * bx + m.jac[1] * by;
                J[1][c] = m.jac[2] * a;
                J[1][3 + c] = m.jac[3] * a;
                J[1][6 + c] = m.jac[2] * bx + m.jac[3] * by;
            }
#pragma unroll
            for (int r = 0; r < 2; r++) {   // WLS::add_mJ(e[r], J[r], w)
                int k = 0;
#pragma unroll
                for (int a = 0; a < 9; a++) {
                    const double jw = J[r][a] * w;
#pragma unroll
                    for (int b = a; b < 9; b++) acc[k++] += jw * J[r][b];
                    acc[45 + a] += e[r] * jw;
                }
            }
        }
        block_sum_f64<HOMOG_NACC>(acc, red, tot, tid);
        if (tid == 0) {   // WLS::compute: (prior + J^T W J) mu = J^T W e by L D L^T, in place in sC
            int k = 0;
            for (int a = 0; a < 9; a++)
                for (int b = a; b < 9; b++, k++) sC[a * 9 + b] = sC[b * 9 + a] = tot[k] + (a == b ? 1.0 : 0.0);
            for (int j = 0; j < 9; j++) {   // below the diagonal: L, on it: D
                double d = sC[j * 9 + j];
                for (int c = 0; c < j; c++) d -= sC[j * 9 + c] * sC[j * 9 + c] * sC[c * 9 + c];
                sC[j * 9 + j] = d;
                for (int i = j + 1; i < 9; i++) {
                    double v = sC[i * 9 + j];
                    for (int c = 0; c < j; c++) v -= sC[i * 9 + c] * sC[j * 9 + c] * sC[c * 9 + c];
                    sC[i * 9 + j] = v / d;
                }
            }
            for (int i = 0; i < 9; i++) {
                double v = tot[45 + i];
                for (int c = 0; c < i; c++) v -= sC[i * 9 + c] * sx[c];
                sx[i] = v;
            }
            for (int i = 0; i < 9; i++) sx[i] /= sC[i * 9 + i];
            for (int i = 8; i >= 0; i--) {
                double v = sx[i];
                for (int c = i + 1; c < 9; c++) v -= sC[c * 9 + i] * sx[c];
                sx[i] = v;
            }
            for (int j = 0; j < 9; j++) sH[j] += sx[j];   // mm3BestHomography += m3Update
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 9; j++) H[j] = sH[j];

    // ---- DecomposeHomography (:232-339) ----
    if (tid == 0) {
        for (int j = 0; j < 9; j++) info->homography[j] = H[j];
        s_flag[0] = homog_decompose(H, dec) ? 1 : 0;
        if (!s_flag[0]) info->status = PTAM_HOMOG_DEGENERATE;
    }
    __syncthreads();
    if (!s_flag[0]) return;

    // ---- ChooseBestDecomposition (:363-435) ----
    int c8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) c8[k] = 0;
    for (int i = tid; i < n; i += HOMOG_THREADS) {   // the first visibility count (:366-378)
        if (!g.flags[i]) continue;
        const double v = H[6] * g.m[i].first[0] + H[7] * g.m[i].first[1] + H[8];
#pragma unroll
        for (int k = 0; k < 8; k++) c8[k] += (v / dec[k].d > 0.0) ? 1 : 0;
    }
    block_sum_i32<8>(c8, ired, itot, tid);
    if (tid == 0) {
        for (int k = 0; k < 8; k++) order[k] = k, score[k] = -itot[k];
        stable_sort_by_score(order, score, 8);   // sort + resize(4)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) c8[k] = 0;
    for (int i = tid; i < n; i += HOMOG_THREADS) {   // the second (:383-395)
        if (!g.flags[i]) continue;
        const double x = g.m[i].first[0], y = g.m[i].first[1];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const Decomp& D = dec[order[k]];
            c8[k] += ((x * D.nrm[0] + y * D.nrm[1] + D.nrm[2]) / D.d > 0.0) ? 1 : 0;
        }
    }
    block_sum_i32<8>(c8, ired, itot, tid);
    if (tid == 0) {
        for (int k = 0; k < 4; k++) score[k] = -itot[k];
        stable_sort_by_score(order, score, 4);   // sort + resize(2)
        const double ratio = (double)score[1] / (double)score[0];
        s_flag[1] = ratio < 0.9 ? 0 : 1;   // (0 / 0 is not below 0.9: ambiguous, as in the reference)
        for (int k = 0; k < 2; k++) {      // m3Essential.T()[j] = t ^ R.T()[j] (:413-415)
            const Decomp& D = dec[order[k]];
            for (int j = 0; j < 3; j++) {
                sE[k][j] = D.t[1] * D.R[6 + j] - D.t[2] * D.R[3 + j];
                sE[k][3 + j] = D.t[2] * D.R[j] - D.t[0] * D.R[6 + j];
                sE[k][6 + j] = D.t[0] * D.R[3 + j] - D.t[1] * D.R[j];
            }
        }
    }
    __syncthreads();
    int chosen = order[0];
    if (s_flag[1]) {   // two-way ambiguity: the Sampson sums over all matches (:406-433)
        const double limit = g.max_sq * 4;
        double ss[2] = {0.0, 0.0};
        for (int i = tid; i < n; i += HOMOG_THREADS) {
            const ptam_homography_match m = g.m[i];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const double d = homog_sampson(sE[k], m);
                ss[k] += d > limit ? limit : d;
            }
        }
        block_sum_f64<2>(ss, red, tot, tid);
        if (!(tot[0] <= tot[1])) chosen = order[1];
        if (tid == 0) {
            info->ambiguous = 1;
            info->sampson[0] = tot[0];
            info->sampson[1] = tot[1];
        }
    }
    if (tid < 12) g.out->se3[tid] = tid < 9 ? dec[chosen].R[tid] : dec[chosen].t[tid - 9];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

static inline uint64_t splitmix64_next(uint64_t& state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void homog_draw(uint64_t seed, int n, int trials, int32_t* out) {   // the draw of :198-211 with rand() replaced
    uint64_t state = seed;
    for (int r = 0; r < trials; r++)
        for (int i = 0; i < 4; i++) {
            int32_t k;
            bool unique;
            do {
                k = (int32_t)(splitmix64_next(state) % (uint64_t)n);
                unique = true;
                for (int j = 0; j < i && unique; j++) unique = out[r * 4 + j] != k;
            } while (!unique);
            out[r * 4 + i] = k;
        }
}

int homog_check(int n, const ptam_homography_opts* o) {
    ARG_TRY(o && n >= 4 && o->trials >= 1 && o->max_pixel_error > 0.0);
    if (o->samples)
        for (int r = 0; r < o->trials; r++)
            for (int i = 0; i < 4; i++) {
                const int32_t k = o->samples[r * 4 + i];
                ARG_TRY(k >= 0 && k < n);
                for (int j = 0; j < i; j++) ARG_TRY(o->samples[r * 4 + j] != k);
            }
    return PTAM_OK;
}

namespace {
struct HomogLayout {
    size_t samples, matches, scores, hs, err2, out, total, pin_out, pin_total;
};
HomogLayout homog_layout(int n, int trials) {
    HomogLayout L;
    const size_t b_samp = up256((size_t)trials * 4 * sizeof(int32_t));
    L.samples = 0;
    L.matches = b_samp;
    L.scores = L.matches + up256((size_t)n * sizeof(ptam_homography_match));
    L.hs = L.scores + up256((size_t)trials * sizeof(double));
    L.err2 = L.hs + up256((size_t)trials * 9 * sizeof(double));
    L.out = L.err2 + up256((size_t)n * sizeof(double));
    L.total = L.out + 256 + up256((size_t)n);
    L.pin_out = b_samp;
    L.pin_total = b_samp + 256 + up256((size_t)n);
    return L;
}
}   // namespace

void homog_sizes(int n, int trials, size_t* scratch_bytes, size_t* pinned_bytes) {
    const HomogLayout L = homog_layout(n, trials);
    *scratch_bytes = L.total;
    *pinned_bytes = L.pin_total;
}

int homog_run(ptam_ctx* ctx, int n, const ptam_homography_match* d_matches, const ptam_homography_match* h_matches,
              const ptam_homography_opts* o, double se3[12], ptam_homography_info* info, uint8_t* inlier_out) {
    const HomogLayout L = homog_layout(n, o->trials);
    void *s, *hp;
    int rc = ctx_scratch(ctx, L.total, &s);
    if (rc) return rc;
    rc = ctx_pinned(ctx, L.pin_total, &hp);
    if (rc) return rc;
    char* d = (char*)s;
    HomogArgs g;
    g.n = n;
    g.trials = o->trials;
    g.max_sq = o->max_pixel_error * o->max_pixel_error;
    g.samples = (const int32_t*)(d + L.samples);
    g.scores = (double*)(d + L.scores);
    g.hs = (double*)(d + L.hs);
    g.err2 = (double*)(d + L.err2);
    g.out = (HomogOut*)(d + L.out);
    g.flags = (uint8_t*)(d + L.out + 256);
    if (d_matches)
        g.m = d_matches;
    else {   // (pageable: staged before the call returns, which is after the final wait)
        g.m = (const ptam_homography_match*)(d + L.matches);
        HIP_TRY(hipMemcpyAsync(d + L.matches, h_matches, (size_t)n * sizeof(ptam_homography_match), hipMemcpyHostToDevice, ctx->stream));
    }
    if (n >= 10) {   // (below ten matches nothing is drawn, :182-186)
        int32_t* h_samples = (int32_t*)hp;
        if (o->samples)
            std::memcpy(h_samples, o->samples, (size_t)o->trials * 4 * sizeof(int32_t));
        else
            homog_draw(o->seed, n, o->trials, h_samples);
        HIP_TRY(hipMemcpyAsync(d + L.samples, h_samples, (size_t)o->trials * 4 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(homog_mlesac_kernel, dim3((o->trials + HOMOG_WAVES - 1) / HOMOG_WAVES), dim3(HOMOG_THREADS), 0, ctx->stream, g);
    }
    hipLaunchKernelGGL(homog_finish_kernel, dim3(1), dim3(HOMOG_THREADS), 0, ctx->stream, g);
    HIP_TRY(hipGetLastError());
    char* h_out = (char*)hp + L.pin_out;
    // (the n inlier bytes come down only for the caller that asked for them)
    HIP_TRY(hipMemcpyAsync(h_out, d + L.out, 256 + (inlier_out ? (size_t)n : 0), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ptam_stream_wait(ctx->stream));
    const HomogOut* r = (const HomogOut*)h_out;
    *info = r->info;
    if (r->info.status == PTAM_HOMOG_OK) std::memcpy(se3, r->se3, sizeof r->se3);
    if (inlier_out) std::memcpy(inlier_out, h_out + 256, (size_t)n);
    return PTAM_OK;
}

extern "C" {

void ptam_homography_opts_default(ptam_homography_opts* o) {
    if (!o) return;
    o->max_pixel_error = 5.0;
    o->trials = 300;
    o->seed = 0;
    o->samples = nullptr;
}

int ptam_homography_samples(uint64_t seed, int n_matches, int trials, int32_t* out) {
    ARG_TRY(out && n_matches >= 4 && trials >= 1);
    homog_draw(seed, n_matches, trials, out);
    return PTAM_OK;
}

int ptam_homography_init(ptam_ctx* ctx, int n, const ptam_homography_match* matches, const ptam_homography_opts* opts,
                         double se3_second_from_first[12], ptam_homography_info* info, uint8_t* inlier_out) {
    ARG_TRY(ctx && matches && opts && se3_second_from_first && info);
    const int rc = homog_check(n, opts);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return homog_run(ctx, n, nullptr, matches, opts, se3_second_from_first, info, inlier_out);
}

}   // extern "C"

void homography_preload_kernels() {
    ptam_preload((const void*)homog_mlesac_kernel);
    ptam_preload((const void*)homog_finish_kernel);
}
