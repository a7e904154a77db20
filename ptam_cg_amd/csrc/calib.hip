// calib.hip — the camera calibrator's optimiser (src/CameraCalibrator.cc, src/CalibImage.cc, src/ATANCamera.cc) on gfx950, fp64.
//   calib_refresh_kernel   the base camera and its five perturbed copies (RefreshParams of params and of params + 0.001 e_i) from
//                          the parameters on the device.  After ptam_calib_reset only: every step refreshes them itself.
//   calib_guess_kernel     CalibImage::GuessInitialPose (:514-606), ONE WORKGROUP PER NEW IMAGE: UnProject of each corner, the
//                          2n x 9 DLT matrix in the handle's work area (a thread owns the rows tid, tid + 256, ...), its right
//                          null vector by one-sided Jacobi as in homography.hip (the three column products of a rotation are sums
//                          over the workgroup in a fixed order; V's nine rows live in LDS), then by thread 0 the 2x2 fix-up, the
//                          Gram-Schmidt rotation and the translation.
//   calib_step_kernel      CameraCalibrator::OptimizeOneStep (:215-269), ONE WORKGROUP PER VIEW, one launch per step:
//                            prologue   the pose update of the PREVIOUS step, delta_n = L^-T (z_n - Y_n delta_c), pose =
//                                       exp(0.1 delta_n) * pose, from what that step left in the view's record (flag APPLY)
//                            measure    CalibImage::Project (:608-648) per corner; D_n = I + sum Jp^T Jp, B_n, e_n, the view's
//                                       share of C and Jc^T e, the squared error and the count, reduced in a fixed order
//                            eliminate  D_n = L L^T, Y_n = L^-1 B_n, z_n = L^-1 e_n, S_n = Y_n^T Y_n, g_n = Y_n^T z_n
//                            last one   the workgroup that arrives last (fence, barrier, atomic add: the arrival count of
//                                       trails_compact_batch_kernel; it clears the count) sums the views' shares in a fixed
//                                       order, solves (C - sum S_n) delta_c = (Jc^T e - sum g_n), adds 0.1 delta_c to the
//                                       parameters and refreshes the six cameras.  Nobody waits for anybody.
//                          The closing launch after a call's last step is the same kernel with flag ONLY_POSE: the same code
//                          updates a pose whether a call is split or not.
//   calib_residual_kernel  what Draw3DGrid(Camera, true) projects for one image.
// The host never holds the camera between steps; K steps are K + 1 launches back to back and one wait.
#include "common.h"
#include "patch_device.h"   // cam_unproject

#include <algorithm>
#include <cfloat>

#pragma clang fp contract(off)

#define CALIB_THREADS 256
#define CALIB_WAVES (CALIB_THREADS / 64)
#define CALIB_NACC 78      // 21 D (upper) + 30 B + 6 e + 15 C (upper) + 5 Jc^T e + 1 squared error
#define CALIB_NSHARE 41    // 15 S (upper) + 5 g + 15 C (upper) + 5 Jc^T e + 1 squared error
enum { CALIB_APPLY = 1, CALIB_ONLY_POSE = 2 };

namespace {

struct CalibState {
    double params[5];
    double delta_c[5];
    int arrived, gate;   // gate: the last step had something to adjust (its updates are applied)
    DevCam cams[6];      // RefreshParams of params, then of params + 0.001 e_i
};
struct CalibView {       // what a step leaves per view
    double L[36], Y[30], z[6];
    double share[CALIB_NSHARE];
    int count, pad_;
};
struct CalibArgs {
    CalibState* state;
    double* poses;                  // 12 per image
    const ptam_calib_corner* corners;
    const int* first;               // n_images + 1
    CalibView* views;
    double* work;                   // 18 doubles per corner
    double* hist_rms;               // per step of a call
    int* hist_count;
    int* guess_status;              // per image of an add
    double width, height;
    int disable;
};

}   // namespace

// ---- sums over the workgroup in a fixed order: lanes by the DPP sum, then the four waves in order ----------------------------
template <int K>
__device__ __forceinline__ void calib_block_sum(const double* v, double (*red)[CALIB_NACC], double* tot, int tid) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        const double s = wave_sum_f64(v[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < K) tot[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}
__device__ __forceinline__ int calib_block_sum_i32(int v, int* red, int tid) {
    const int s = wave_sum_i32(v);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const int t = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return t;
}

__device__ __forceinline__ void calib_refresh(const CalibArgs& g, int tid) {   // tid < 6
    double p[5];
#pragma unroll
    for (int i = 0; i < 5; i++) p[i] = g.state->params[i] + ((tid == i + 1) ? 0.001 : 0.0);   // UpdateParams(0.001 e_i) :225-228
    g.state->cams[tid] = devcam_refresh(g.width, g.height, p[0], p[1], p[2], p[3], p[4]);
}

__global__ void __launch_bounds__(64) calib_refresh_kernel(CalibArgs g) {
    if (threadIdx.x < 6) calib_refresh(g, threadIdx.x);
}

// ---- CalibImage::GuessInitialPose ---------------------------------------------------------------------------------------------
// the singular values (descending) of a 2x2 matrix and the right singular vector of the smaller one, by one-sided Jacobi
__device__ __forceinline__ void calib_svd2(const double M[4], double sg[2], double v_small[2]) {
    double A[4] = {M[0], M[1], M[2], M[3]}, V[4] = {1.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < 30; sweep++) {
        const double al = A[0] * A[0] + A[2] * A[2], be = A[1] * A[1] + A[3] * A[3], ga = A[0] * A[1] + A[2] * A[3];
        if (ga == 0.0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be)) break;
        const double z = (be - al) / (2.0 * ga);
        const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const double ap = A[i * 2], aq = A[i * 2 + 1];
            A[i * 2] = c * ap - s * aq;
            A[i * 2 + 1] = s * ap + c * aq;
            const double vp = V[i * 2], vq = V[i * 2 + 1];
            V[i * 2] = c * vp - s * vq;
            V[i * 2 + 1] = s * vp + c * vq;
        }
    }
    const double s0 = sqrt(A[0] * A[0] + A[2] * A[2]), s1 = sqrt(A[1] * A[1] + A[3] * A[3]);
    const int small = s0 < s1 ? 0 : 1;
    sg[0] = small ? s0 : s1;
    sg[1] = small ? s1 : s0;
    v_small[0] = V[small];
    v_small[1] = V[2 + small];
}

__global__ void __launch_bounds__(CALIB_THREADS) calib_guess_kernel(CalibArgs g, int image0) {
    __shared__ double red[CALIB_WAVES][CALIB_NACC], tot[CALIB_NACC], sV[81];
    const int tid = threadIdx.x, img = image0 + blockIdx.x;
    const int first = g.first[img], n = g.first[img + 1] - first, rows = 2 * n;
    double* A = g.work + (size_t)first * 18;
    const DevCam cam = g.state->cams[0];
    for (int i = tid; i < n; i += CALIB_THREADS) {   // :522-551
        const ptam_calib_corner c = g.corners[first + i];
        double u, v;
        cam_unproject(cam, c.u, c.v, u, v);
        const double x = (double)c.gx, y = (double)c.gy;
        double* r0 = A + (size_t)(2 * i) * 9;
        r0[0] = x, r0[1] = y, r0[2] = 1.0, r0[3] = 0.0, r0[4] = 0.0, r0[5] = 0.0, r0[6] = -x * u, r0[7] = -y * u, r0[8] = -u;
        double* r1 = r0 + 9;
        r1[0] = 0.0, r1[1] = 0.0, r1[2] = 0.0, r1[3] = x, r1[4] = y, r1[5] = 1.0, r1[6] = -x * v, r1[7] = -y * v, r1[8] = -v;
    }
    if (tid < 81) sV[tid] = (tid % 10 == 0) ? 1.0 : 0.0;
    __syncthreads();
    // (from here a thread touches the rows tid, tid + 256, ... only, and thread i < 9 row i of V: the rotations need no barrier of their own)
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0.0;
    for (int r = tid; r < rows; r += CALIB_THREADS)
#pragma unroll
        for (int j = 0; j < 9; j++) acc[j] += A[(size_t)r * 9 + j] * A[(size_t)r * 9 + j];
    calib_block_sum<9>(acc, red, tot, tid);
    double fro = 0.0;
    for (int j = 0; j < 9; j++) fro += tot[j];
    const double tiny = 64.0 * DBL_EPSILON * DBL_EPSILON * fro;   // (wave_null_vector, homography.hip: a column that is rounding noise only)
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                double s3[3] = {0.0, 0.0, 0.0};
                for (int r = tid; r < rows; r += CALIB_THREADS) {
                    const double ap = A[(size_t)r * 9 + p], aq = A[(size_t)r * 9 + q];
                    s3[0] += ap * ap;
                    s3[1] += aq * aq;
                    s3[2] += ap * aq;
                }
                calib_block_sum<3>(s3, red, tot, tid);
                const double al = tot[0], be = tot[1], ga = tot[2];   // (rewritten only behind the next sum's first barrier)
                if (ga == 0.0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be) || fmin(al, be) <= tiny) continue;   // (uniform)
                rotated = true;
                const double z = (be - al) / (2.0 * ga);
                const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = tid; r < rows; r += CALIB_THREADS) {
                    const double ap = A[(size_t)r * 9 + p], aq = A[(size_t)r * 9 + q];
                    A[(size_t)r * 9 + p] = c * ap - s * aq;
                    A[(size_t)r * 9 + q] = s * ap + c * aq;
                }
                if (tid < 9) {
                    const double vp = sV[tid * 9 + p], vq = sV[tid * 9 + q];
                    sV[tid * 9 + p] = c * vp - s * vq;
                    sV[tid * 9 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
#pragma unroll
    for (int j = 0; j < 9; j++) acc[j] = 0.0;
    for (int r = tid; r < rows; r += CALIB_THREADS)
#pragma unroll
        for (int j = 0; j < 9; j++) acc[j] += A[(size_t)r * 9 + j] * A[(size_t)r * 9 + j];
    calib_block_sum<9>(acc, red, tot, tid);   // (its barriers also publish V)
    if (tid != 0) return;
    int col = 0;   // the column of V under the matrix column of least norm (the first of equals): get_VT()[8]
    for (int j = 1; j < 9; j++)
        if (tot[j] < tot[col]) col = j;
    double H[9];
    for (int i = 0; i < 9; i++) H[i] = sV[i * 9 + col];
    if (H[8] < 0.0)   // the translation's z is H[8] over two positive numbers: the sign that puts the grid in front (ptam_hip.h)
        for (int i = 0; i < 9; i++) H[i] = -H[i];
    {   // the possibly poorly conditioned top-left bit :563-583
        const double M[4] = {H[0], H[1], H[3], H[4]};
        double sg[2], vs[2];
        calib_svd2(M, sg, vs);
        for (int i = 0; i < 9; i++) H[i] = H[i] / sg[0];
        const double lam2 = sg[1] / sg[0];
        const double b1 = sqrt(1.0 - lam2 * lam2);
        const double ap0 = b1 * vs[0], ap1 = b1 * vs[1];   // v2b * VT with v2b = (0, b1)
        const double dot = H[6] * ap0 + H[7] * ap1;
        H[6] = dot > 0 ? ap0 : -ap0;
        H[7] = dot > 0 ? ap1 : -ap1;
    }
    const double mag1 = sqrt((H[0] * H[0] + H[3] * H[3]) + H[6] * H[6]);   // :591-601
    for (int i = 0; i < 9; i++) H[i] = H[i] / mag1;
    double R[9], T[3];
    const double d01 = (H[0] * H[1] + H[3] * H[4]) + H[6] * H[7];
    for (int i = 0; i < 3; i++) {
        R[i * 3] = H[i * 3];
        R[i * 3 + 1] = H[i * 3 + 1] - H[i * 3] * d01;
        T[i] = H[i * 3 + 2];
    }
    const double mag2 = sqrt((R[1] * R[1] + R[4] * R[4]) + R[7] * R[7]);
    for (int i = 0; i < 3; i++) R[i * 3 + 1] /= mag2;
    R[2] = R[3] * R[7] - R[6] * R[4];
    R[5] = R[6] * R[1] - R[0] * R[7];
    R[8] = R[0] * R[4] - R[3] * R[1];
    bool ok = T[2] != 0.0;
    for (int i = 0; i < 9; i++) ok = ok && isfinite(R[i]);
    for (int i = 0; i < 3; i++) ok = ok && isfinite(T[i]);
    double* pose = g.poses + (size_t)img * 12;
    for (int i = 0; i < 9; i++) pose[i] = R[i];
    for (int i = 0; i < 3; i++) pose[9 + i] = T[i];
    g.guess_status[blockIdx.x] = ok ? PTAM_CALIB_GUESS_OK : PTAM_CALIB_GUESS_REFUSED;
}

// ---- CalibImage::Project of one corner (:608-648); false where the reference says `continue` --------------------------------
__device__ __forceinline__ bool calib_measure(const DevCam* cams, const double* T, const ptam_calib_corner& c, double e[2],
                                              double Jp[2][6], double Jc[2][5]) {
    double X, Y, Z;
    se3_apply(T, (double)c.gx, (double)c.gy, 0.0, X, Y, Z);
    if (Z <= 0.001) return false;
    const double x = X / Z, y = Y / Z;
    double u, v, r, f;
    cam_project(cams[0], x, y, u, v, r, f);
    if (r > cams[0].max_r) return false;   // Camera.Invalid()
    e[0] = c.u - u;
    e[1] = c.v - v;
    const double iz = 1.0 / Z;
    double D[4];
    cam_derivs(cams[0], x, y, r, f, D);
#pragma unroll
    for (int dof = 0; dof < 6; dof++) {   // SE3<>::generator_field(dof, unproject(v3Cam))
        double m0 = 0.0, m1 = 0.0, m2 = 0.0;
        if (dof == 0) m0 = 1.0;
        if (dof == 1) m1 = 1.0;
        if (dof == 2) m2 = 1.0;
        if (dof == 3) m1 = -Z, m2 = Y;
        if (dof == 4) m2 = -X, m0 = Z;
        if (dof == 5) m0 = -Y, m1 = X;
        const double c0 = (m0 - X * m2 * iz) * iz, c1 = (m1 - Y * m2 * iz) * iz;
        Jp[0][dof] = D[0] * c0 + D[1] * c1;
        Jp[1][dof] = D[2] * c0 + D[3] * c1;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) {   // GetCameraParameterDerivs src/ATANCamera.cc:211-237
        if (i == 4 && cams[0].w == 0.0) {
            Jc[0][i] = 0.0;
            Jc[1][i] = 0.0;
            continue;
        }
        double ub, vb, rb, fb;
        cam_project(cams[1 + i], x, y, ub, vb, rb, fb);
        Jc[0][i] = (ub - u) / 0.001;
        Jc[1][i] = (vb - v) / 0.001;
    }
    return true;
}

__global__ void __launch_bounds__(CALIB_THREADS) calib_step_kernel(CalibArgs g, int step, int flags) {
    __shared__ double red[CALIB_WAVES][CALIB_NACC], tot[CALIB_NACC], sL[36], sY[36], sPose[12];
    __shared__ DevCam sCam[6];
    __shared__ int ired[CALIB_WAVES], s_last;
    const int tid = threadIdx.x, view = blockIdx.x, nviews = gridDim.x;
    CalibView* V = g.views + view;
    double* pose = g.poses + (size_t)view * 12;

    // ---- the previous step's pose update (:266-267) ----
    if (tid < 12) sPose[tid] = pose[tid];
    __syncthreads();
    if ((flags & CALIB_APPLY) && tid == 0 && g.state->gate) {
        double d[6];
        for (int i = 0; i < 6; i++) {
            double v = V->z[i];
            for (int k = 0; k < 5; k++) v -= V->Y[i * 5 + k] * g.state->delta_c[k];
            d[i] = v;
        }
        for (int i = 5; i >= 0; i--) {   // L^T delta = z - Y delta_c
            double v = d[i];
            for (int k = i + 1; k < 6; k++) v -= V->L[k * 6 + i] * d[k];
            d[i] = v / V->L[i * 6 + i];
        }
        for (int i = 0; i < 6; i++) d[i] *= 0.1;   // vUpdate *= 0.1 :265
        double out[12], cur[12];
        for (int i = 0; i < 12; i++) cur[i] = sPose[i];
        se3_exp_mul(d, cur, out);
        for (int i = 0; i < 12; i++) sPose[i] = out[i], pose[i] = out[i];
    }
    if (flags & CALIB_ONLY_POSE) return;
    if (tid < 6) sCam[tid] = g.state->cams[tid];
    __syncthreads();

    // ---- CalibImage::Project and the sums of :236-257 ----
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; i++) T[i] = sPose[i];
    double acc[CALIB_NACC];
#pragma unroll
    for (int k = 0; k < CALIB_NACC; k++) acc[k] = 0.0;
    int cnt = 0;
    const int first = g.first[view], n = g.first[view + 1] - first;
    for (int i = tid; i < n; i += CALIB_THREADS) {
        double e[2], Jp[2][6], Jc[2][5];
        if (!calib_measure(sCam, T, g.corners[first + i], e, Jp, Jc)) continue;
        cnt++;
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = a; b < 6; b++) acc[k++] += Jp[0][a] * Jp[0][b] + Jp[1][a] * Jp[1][b];
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
            for (int b = 0; b < 5; b++) acc[k++] += Jp[0][a] * Jc[0][b] + Jp[1][a] * Jc[1][b];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[k++] += Jp[0][a] * e[0] + Jp[1][a] * e[1];
#pragma unroll
        for (int a = 0; a < 5; a++)
#pragma unroll
            for (int b = a; b < 5; b++) acc[k++] += Jc[0][a] * Jc[0][b] + Jc[1][a] * Jc[1][b];
#pragma unroll
        for (int a = 0; a < 5; a++) acc[k++] += Jc[0][a] * e[0] + Jc[1][a] * e[1];
        acc[k++] += e[0] * e[0] + e[1] * e[1];
    }
    calib_block_sum<CALIB_NACC>(acc, red, tot, tid);
    const int count = calib_block_sum_i32(cnt, ired, tid);

    // ---- the view's block eliminated: D = L L^T, Y = L^-1 [B | e] ----
    if (tid == 0) {
        int k = 0;
        for (int a = 0; a < 6; a++)
            for (int b = a; b < 6; b++, k++) sL[a * 6 + b] = sL[b * 6 + a] = tot[k] + (a == b ? 1.0 : 0.0);   // mJTJ = Identity :223
        for (int j = 0; j < 6; j++) {
            double d = sL[j * 6 + j];
            for (int c = 0; c < j; c++) d -= sL[j * 6 + c] * sL[j * 6 + c];
            d = sqrt(d);
            sL[j * 6 + j] = d;
            for (int i = j + 1; i < 6; i++) {
                double v = sL[i * 6 + j];
                for (int c = 0; c < j; c++) v -= sL[i * 6 + c] * sL[j * 6 + c];
                sL[i * 6 + j] = v / d;
            }
        }
    }
    __syncthreads();
    if (tid < 6) {   // column tid of [B | e]: forward substitution
        double y[6];
        for (int i = 0; i < 6; i++) {
            double v = tid < 5 ? tot[21 + i * 5 + tid] : tot[51 + i];
            for (int c = 0; c < i; c++) v -= sL[i * 6 + c] * y[c];
            y[i] = v / sL[i * 6 + i];
            sY[i * 6 + tid] = y[i];
        }
    }
    __syncthreads();
    if (tid < 36) V->L[tid] = (tid % 6 <= tid / 6) ? sL[tid] : 0.0;
    if (tid < 30) V->Y[tid] = sY[(tid / 5) * 6 + tid % 5];
    if (tid < 6) V->z[tid] = sY[tid * 6 + 5];
    if (tid < 20) {   // S = Y^T Y (upper), g = Y^T z
        int a = 0, b = tid;
        if (tid < 15) {
            int rem = tid;
            while (rem >= 5 - a) rem -= 5 - a, a++;
            b = a + rem;
        } else {
            a = tid - 15;
            b = 5;
        }
        double v = 0.0;
        for (int i = 0; i < 6; i++) v += sY[i * 6 + a] * sY[i * 6 + b];
        V->share[tid] = v;
    }
    if (tid < 21) V->share[20 + tid] = tot[57 + tid];   // C (upper), Jc^T e, the squared error
    if (tid == 0) V->count = count;

    // ---- arrival: the last workgroup finishes the step ----
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const bool last = atomicAdd(&g.state->arrived, 1) == nviews - 1;
        if (last) g.state->arrived = 0;   // (for the next launch; nobody else of this one looks at it any more)
        s_last = last ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();   // (the other views' records, written before their arrival)
    double sh[CALIB_NSHARE];
#pragma unroll
    for (int k = 0; k < CALIB_NSHARE; k++) sh[k] = 0.0;
    int c_all = 0;
    for (int v = tid; v < nviews; v += CALIB_THREADS) {
        const CalibView* W = g.views + v;
#pragma unroll
        for (int k = 0; k < CALIB_NSHARE; k++) sh[k] += W->share[k];
        c_all += W->count;
    }
    calib_block_sum<CALIB_NSHARE>(sh, red, tot, tid);
    const int total = calib_block_sum_i32(c_all, ired, tid);
    if (tid == 0) {
        double A5[25], rhs[5], dc[5];
        int k = 0;
        for (int a = 0; a < 5; a++)
            for (int b = a; b < 5; b++, k++) A5[a * 5 + b] = A5[b * 5 + a] = ((a == b ? 1.0 : 0.0) + tot[20 + k]) - tot[k];
        for (int a = 0; a < 5; a++) rhs[a] = tot[35 + a] - tot[15 + a];
        for (int j = 0; j < 5; j++) {   // Cholesky, in place
            double d = A5[j * 5 + j];
            for (int c = 0; c < j; c++) d -= A5[j * 5 + c] * A5[j * 5 + c];
            d = sqrt(d);
            A5[j * 5 + j] = d;
            for (int i = j + 1; i < 5; i++) {
                double v = A5[i * 5 + j];
                for (int c = 0; c < j; c++) v -= A5[i * 5 + c] * A5[j * 5 + c];
                A5[i * 5 + j] = v / d;
            }
        }
        for (int i = 0; i < 5; i++) {
            double v = rhs[i];
            for (int c = 0; c < i; c++) v -= A5[i * 5 + c] * dc[c];
            dc[i] = v / A5[i * 5 + i];
        }
        for (int i = 4; i >= 0; i--) {
            double v = dc[i];
            for (int c = i + 1; c < 5; c++) v -= A5[c * 5 + i] * dc[c];
            dc[i] = v / A5[i * 5 + i];
        }
        g.hist_rms[step] = sqrt(tot[40] / (double)total);   // mdMeanPixelError :260, before the update
        g.hist_count[step] = total;
        g.state->gate = total > 0 ? 1 : 0;
        if (total > 0) {
            for (int i = 0; i < 5; i++) {
                g.state->delta_c[i] = dc[i];
                g.state->params[i] = g.state->params[i] + 0.1 * dc[i];   // UpdateParams(vUpdate.slice(...)) :268
            }
            if (g.disable) g.state->params[4] = 0.0;   // DisableRadialDistortion at the start of the next step :226
        }
    }
    __syncthreads();
    if (tid < 6 && g.state->gate) calib_refresh(g, tid);
}

__global__ void __launch_bounds__(CALIB_THREADS) calib_residual_kernel(CalibArgs g, int image) {
    const int first = g.first[image], n = g.first[image + 1] - first;
    const int i = blockIdx.x * CALIB_THREADS + threadIdx.x;
    if (i >= n) return;
    const ptam_calib_corner c = g.corners[first + i];
    const double* T = g.poses + (size_t)image * 12;
    double X, Y, Z, u = 0.0, v = 0.0;
    int valid = 0;
    se3_apply(T, (double)c.gx, (double)c.gy, 0.0, X, Y, Z);
    if (!(Z <= 0.001)) {
        double r, f;
        cam_project(g.state->cams[0], X / Z, Y / Z, u, v, r, f);
        valid = r > g.state->cams[0].max_r ? 0 : 1;
    }
    g.work[2 * i] = u;
    g.work[2 * i + 1] = v;
    ((int*)(g.work + 2 * (size_t)n))[i] = valid;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct ptam_calibrator {
    ptam_ctx* ctx;
    int max_images, max_corners, n_images, n_corners, disable;
    char* d_block;
    char* h_pin;   // hist_rms | hist_count | params | guess status | poses of an add
    size_t pin_rms, pin_count, pin_params, pin_status, pin_poses;
    CalibArgs g;
    std::vector<int> first;
};

static inline size_t calib_up256(size_t b) { return (b + 255) & ~(size_t)255; }

static int calib_upload_params(ptam_calibrator* h, const double p[5]) {
    hipStream_t st = h->ctx->stream;
    double* hp = (double*)(h->h_pin + h->pin_params);
    std::memcpy(hp, p, 5 * sizeof(double));
    HIP_TRY(hipMemcpyAsync(h->g.state->params, hp, 5 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(calib_refresh_kernel, dim3(1), dim3(64), 0, st, h->g);
    HIP_TRY(hipGetLastError());
    HIP_TRY(ptam_stream_wait(st));
    return PTAM_OK;
}

extern "C" {

int ptam_calib_create(ptam_ctx* ctx, int max_images, int max_corners_total, ptam_calibrator** out) {
    ARG_TRY(ctx && out);
    ARG_TRY(max_images >= 1 && max_images <= PTAM_CALIB_MAX_IMAGES && max_corners_total >= 4 && max_corners_total <= PTAM_CALIB_MAX_CORNERS);
    HIP_TRY(hipSetDevice(ctx->device));
    ptam_calibrator* h = new ptam_calibrator();
    h->ctx = ctx;
    h->max_images = max_images;
    h->max_corners = max_corners_total;
    h->n_images = h->n_corners = h->disable = 0;
    h->d_block = nullptr;
    h->h_pin = nullptr;
    h->first.assign(1, 0);
    size_t off = 0;
    auto take = [&](size_t b) {
        const size_t o = off;
        off += calib_up256(b);
        return o;
    };
    const size_t o_state = take(sizeof(CalibState)), o_poses = take((size_t)max_images * 12 * sizeof(double)),
                 o_corners = take((size_t)max_corners_total * sizeof(ptam_calib_corner)), o_first = take(((size_t)max_images + 1) * sizeof(int)),
                 o_views = take((size_t)max_images * sizeof(CalibView)), o_work = take((size_t)max_corners_total * 18 * sizeof(double)),
                 o_rms = take((size_t)PTAM_CALIB_MAX_STEPS * sizeof(double)), o_cnt = take((size_t)PTAM_CALIB_MAX_STEPS * sizeof(int)),
                 o_status = take((size_t)max_images * sizeof(int));
    if (hipMalloc(&h->d_block, off) != hipSuccess) {
        ptam_set_error("ptam_calib_create: %zu bytes of device memory", off);
        delete h;
        return PTAM_E_HIP;
    }
    h->pin_rms = 0;
    h->pin_count = h->pin_rms + calib_up256((size_t)PTAM_CALIB_MAX_STEPS * sizeof(double));
    h->pin_params = h->pin_count + calib_up256((size_t)PTAM_CALIB_MAX_STEPS * sizeof(int));
    h->pin_status = h->pin_params + 256;
    h->pin_poses = h->pin_status + calib_up256((size_t)max_images * sizeof(int));
    const size_t pin_total = h->pin_poses + calib_up256((size_t)max_images * 12 * sizeof(double));
    if (hipHostMalloc(&h->h_pin, pin_total, hipHostMallocDefault) != hipSuccess) {
        ptam_set_error("ptam_calib_create: %zu bytes of pinned memory", pin_total);
        hipFree(h->d_block);
        delete h;
        return PTAM_E_HIP;
    }
    char* d = h->d_block;
    h->g.state = (CalibState*)(d + o_state);
    h->g.poses = (double*)(d + o_poses);
    h->g.corners = (const ptam_calib_corner*)(d + o_corners);
    h->g.first = (const int*)(d + o_first);
    h->g.views = (CalibView*)(d + o_views);
    h->g.work = (double*)(d + o_work);
    h->g.hist_rms = (double*)(d + o_rms);
    h->g.hist_count = (int*)(d + o_cnt);
    h->g.guess_status = (int*)(d + o_status);
    h->g.width = ctx->params.width;
    h->g.height = ctx->params.height;
    h->g.disable = 0;
    if (hipMemsetAsync(d, 0, off, ctx->stream) != hipSuccess) {
        ptam_set_error("ptam_calib_create: hipMemsetAsync failed");
        hipHostFree(h->h_pin);
        hipFree(h->d_block);
        delete h;
        return PTAM_E_HIP;
    }
    const double def[5] = {0.5, 0.75, 0.5, 0.5, 0.1};   // ATANCamera::mvDefaultParams src/ATANCamera.cc:286
    const int rc = calib_upload_params(h, def);
    if (rc) {
        hipHostFree(h->h_pin);
        hipFree(h->d_block);
        delete h;
        return rc;
    }
    *out = h;
    return PTAM_OK;
}

int ptam_calib_destroy(ptam_calibrator* h) {
    if (!h) return PTAM_OK;
    hipSetDevice(h->ctx->device);
    ptam_stream_wait(h->ctx->stream);
    hipHostFree(h->h_pin);
    hipFree(h->d_block);
    delete h;
    return PTAM_OK;
}

int ptam_calib_reset(ptam_calibrator* h, const double* params, int disable_distortion) {
    ARG_TRY(h);
    double p[5] = {0.5, 0.75, 0.5, 0.5, 0.1};
    if (params)
        for (int i = 0; i < 5; i++) p[i] = params[i];
    for (int i = 0; i < 5; i++) ARG_TRY(std::isfinite(p[i]));
    ARG_TRY(p[0] != 0.0 && p[1] != 0.0);
    if (disable_distortion) p[4] = 0.0;   // DisableRadialDistortion :159
    HIP_TRY(hipSetDevice(h->ctx->device));
    const int rc = calib_upload_params(h, p);
    if (rc) return rc;
    h->disable = h->g.disable = disable_distortion ? 1 : 0;
    h->n_images = h->n_corners = 0;
    h->first.assign(1, 0);
    return PTAM_OK;
}

int ptam_calib_counts(ptam_calibrator* h, int32_t* n_images, int32_t* n_corners) {
    ARG_TRY(h && n_images && n_corners);
    *n_images = h->n_images;
    *n_corners = h->n_corners;
    return PTAM_OK;
}

int ptam_calib_add_images(ptam_calibrator* h, int n, const int32_t* first_corner, const ptam_calib_corner* corners, int32_t* status_out) {
    ARG_TRY(h && n >= 1 && first_corner && corners && status_out);
    ARG_TRY(first_corner[0] == 0 && n <= h->max_images - h->n_images);
    for (int k = 0; k < n; k++) ARG_TRY(first_corner[k + 1] >= first_corner[k] && first_corner[k + 1] - first_corner[k] >= 4);
    const int total = first_corner[n];
    ARG_TRY(total <= h->max_corners - h->n_corners);
    {
        std::vector<int64_t> keys;
        for (int k = 0; k < n; k++) {
            keys.clear();
            for (int i = first_corner[k]; i < first_corner[k + 1]; i++) {
                ARG_TRY(std::isfinite(corners[i].u) && std::isfinite(corners[i].v));
                keys.push_back(((int64_t)corners[i].gx << 32) | (uint32_t)corners[i].gy);
            }
            std::sort(keys.begin(), keys.end());
            ARG_TRY(std::adjacent_find(keys.begin(), keys.end()) == keys.end());   // a grid position twice in one image
        }
    }
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    std::vector<int> first(h->first);
    for (int k = 0; k < n; k++) first.push_back(h->n_corners + first_corner[k + 1]);
    ptam_calib_corner* d_corners = (ptam_calib_corner*)h->g.corners;
    int* d_first = (int*)h->g.first;
    // (pageable sources: staged before the copies return; the final wait is the call's one wait)
    HIP_TRY(hipMemcpyAsync(d_corners + h->n_corners, corners, (size_t)total * sizeof(ptam_calib_corner), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_first + h->n_images, first.data() + h->n_images, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(calib_guess_kernel, dim3(n), dim3(CALIB_THREADS), 0, st, h->g, h->n_images);
    HIP_TRY(hipGetLastError());
    int* h_status = (int*)(h->h_pin + h->pin_status);
    double* h_poses = (double*)(h->h_pin + h->pin_poses);
    HIP_TRY(hipMemcpyAsync(h_status, h->g.guess_status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_poses, h->g.poses + (size_t)h->n_images * 12, (size_t)n * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    int kept = 0;
    for (int k = 0; k < n; k++) kept += h_status[k] == PTAM_CALIB_GUESS_OK ? 1 : 0;
    if (kept < n) {   // a refused image is not added: the kept ones move up (rare; a second wait)
        std::vector<ptam_calib_corner> cc;
        std::vector<double> pp;
        std::vector<int> ff(h->first);
        for (int k = 0; k < n; k++) {
            if (h_status[k] != PTAM_CALIB_GUESS_OK) continue;
            cc.insert(cc.end(), corners + first_corner[k], corners + first_corner[k + 1]);
            pp.insert(pp.end(), h_poses + (size_t)k * 12, h_poses + (size_t)k * 12 + 12);
            ff.push_back(h->n_corners + (int)cc.size());
        }
        if (kept) {
            HIP_TRY(hipMemcpyAsync(d_corners + h->n_corners, cc.data(), cc.size() * sizeof(ptam_calib_corner), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(h->g.poses + (size_t)h->n_images * 12, pp.data(), pp.size() * sizeof(double), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_first + h->n_images, ff.data() + h->n_images, ((size_t)kept + 1) * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(ptam_stream_wait(st));
        }
        first.swap(ff);
    }
    for (int k = 0; k < n; k++) status_out[k] = h_status[k];
    h->first.swap(first);
    h->n_images += kept;
    h->n_corners = h->first.back();
    return PTAM_OK;
}

int ptam_calib_set_poses(ptam_calibrator* h, const double* poses) {
    ARG_TRY(h && poses);
    if (h->n_images == 0) {
        ptam_set_error("ptam_calib_set_poses: no images");
        return PTAM_E_STATE;
    }
    for (int i = 0; i < h->n_images * 12; i++) ARG_TRY(std::isfinite(poses[i]));
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(hipMemcpyAsync(h->g.poses, poses, (size_t)h->n_images * 12 * sizeof(double), hipMemcpyHostToDevice, h->ctx->stream));
    HIP_TRY(ptam_stream_wait(h->ctx->stream));
    return PTAM_OK;
}

int ptam_calib_read_poses(ptam_calibrator* h, double* poses) {
    ARG_TRY(h && poses);
    if (h->n_images == 0) return PTAM_OK;
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(hipMemcpyAsync(poses, h->g.poses, (size_t)h->n_images * 12 * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    HIP_TRY(ptam_stream_wait(h->ctx->stream));
    return PTAM_OK;
}

int ptam_calib_params(ptam_calibrator* h, double params[5]) {
    ARG_TRY(h && params);
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(hipMemcpyAsync(params, h->g.state->params, 5 * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    HIP_TRY(ptam_stream_wait(h->ctx->stream));
    return PTAM_OK;
}

int ptam_calib_optimize(ptam_calibrator* h, int steps, ptam_calib_result* result, double* rms_history) {
    ARG_TRY(h && result && steps >= 1 && steps <= PTAM_CALIB_MAX_STEPS);
    if (h->n_images == 0) {
        ptam_set_error("ptam_calib_optimize: no images");
        return PTAM_E_STATE;
    }
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    for (int k = 0; k < steps; k++)
        hipLaunchKernelGGL(calib_step_kernel, dim3(h->n_images), dim3(CALIB_THREADS), 0, st, h->g, k, k ? CALIB_APPLY : 0);
    hipLaunchKernelGGL(calib_step_kernel, dim3(h->n_images), dim3(CALIB_THREADS), 0, st, h->g, steps, CALIB_APPLY | CALIB_ONLY_POSE);
    HIP_TRY(hipGetLastError());
    double* h_rms = (double*)(h->h_pin + h->pin_rms);
    int* h_cnt = (int*)(h->h_pin + h->pin_count);
    double* h_par = (double*)(h->h_pin + h->pin_params);
    HIP_TRY(hipMemcpyAsync(h_rms, h->g.hist_rms, (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_cnt, h->g.hist_count, (size_t)steps * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_par, h->g.state->params, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    std::memset(result, 0, sizeof *result);
    for (int i = 0; i < 5; i++) result->params[i] = h_par[i];
    result->pixel_aspect_ratio = (h->g.height * h_par[1]) / (h->g.width * h_par[0]);   // PixelAspectRatio include/ATANCamera.h:101
    result->steps = steps;
    if (h_cnt[0] == 0) {   // nothing to adjust: every step's update was gated off on the device
        result->status = PTAM_CALIB_NO_MEASUREMENTS;
        result->n_measurements = 0;
        result->rms = 0.0;
        return PTAM_OK;
    }
    result->status = PTAM_CALIB_OK;
    result->n_measurements = h_cnt[steps - 1];
    result->rms = h_rms[steps - 1];
    if (rms_history) std::memcpy(rms_history, h_rms, (size_t)steps * sizeof(double));
    return PTAM_OK;
}

int ptam_calib_residuals(ptam_calibrator* h, int image, double* projected_uv, int32_t* valid) {
    ARG_TRY(h && projected_uv && valid && image >= 0 && image < h->n_images);
    HIP_TRY(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream;
    const int n = h->first[image + 1] - h->first[image];
    hipLaunchKernelGGL(calib_residual_kernel, dim3((n + CALIB_THREADS - 1) / CALIB_THREADS), dim3(CALIB_THREADS), 0, st, h->g, image);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(projected_uv, h->g.work, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(valid, h->g.work + 2 * (size_t)n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ptam_stream_wait(st));
    return PTAM_OK;
}

}   // extern "C"

void calib_preload_kernels() {
    ptam_preload((const void*)calib_refresh_kernel);
    ptam_preload((const void*)calib_guess_kernel);
    ptam_preload((const void*)calib_step_kernel);
    ptam_preload((const void*)calib_residual_kernel);
}
