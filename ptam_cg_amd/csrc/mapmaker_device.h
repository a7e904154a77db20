// mapmaker_device.h — the per-point geometry of the map maker, shared by the epipolar point maker (mapmaker.hip) and the stereo
// initialiser (trails.hip): Triangulate's singular vector, the rotations of a pose and the unit ray of a pixel.
#pragma once
#include <cfloat>

#include "common.h"
#include "patch_device.h"

// ---- Triangulate (:171-189): the right singular vector of the smallest singular value of A (4x4), by one-sided Jacobi on A
// itself (Hestenes): column pairs are rotated until they are orthogonal, V accumulates the rotations, and the column of V whose
// column of A has the least norm is the vector.  (Not the eigenvector of A^T A: that squares the condition number, and a
// small baseline is the ill-conditioned case.)  The sign is free: the caller projects.
__device__ __forceinline__ void smallest_right_singular_vector(double A[16], double v[4]) {
    double V[16];
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    al += A[i * 4 + p] * A[i * 4 + p];
                    be += A[i * 4 + q] * A[i * 4 + q];
                    ga += A[i * 4 + p] * A[i * 4 + q];
                }
                if (ga == 0.0 || fabs(ga) <= DBL_EPSILON * sqrt(al * be)) continue;
                rotated = true;
                const double z = (be - al) / (2.0 * ga);
                const double t = fabs(z) < 1e150 ? copysign(1.0, z) / (fabs(z) + sqrt(1.0 + z * z)) : 0.5 / z;
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double ap = A[i * 4 + p], aq = A[i * 4 + q];
                    A[i * 4 + p] = c * ap - s * aq;
                    A[i * 4 + q] = s * ap + c * aq;
                    const double vp = V[i * 4 + p], vq = V[i * 4 + q];
                    V[i * 4 + p] = c * vp - s * vq;
                    V[i * 4 + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int k = 0;
    double best = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double nn = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) nn += A[i * 4 + j] * A[i * 4 + j];
        if (j == 0 || nn < best) best = nn, k = j;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = k == 0 ? V[i * 4] : k == 1 ? V[i * 4 + 1] : k == 2 ? V[i * 4 + 2] : V[i * 4 + 3];
}

// R^T v and R v, dot products left to right like TooN's, no contraction
__device__ __forceinline__ double rt_row(const double R[9], int i, const double v[3]) {
    return nc_add(nc_add(nc_mul(R[i], v[0]), nc_mul(R[3 + i], v[1])), nc_mul(R[6 + i], v[2]));
}
__device__ __forceinline__ double r_row(const double R[9], int i, const double v[3]) {
    return nc_add(nc_add(nc_mul(R[3 * i], v[0]), nc_mul(R[3 * i + 1], v[1])), nc_mul(R[3 * i + 2], v[2]));
}
// normalize(unproject(UnProject(px))): TooN's v /= sqrt(v * v)
__device__ __forceinline__ void unit_ray(const DevCam& cam, double u, double v, double out[3]) {
    double x, y;
    cam_unproject(cam, u, v, x, y);
    const double nrm = sqrt(nc_add(nc_add(nc_mul(x, x), nc_mul(y, y)), 1.0));
    out[0] = x / nrm;
    out[1] = y / nrm;
    out[2] = 1.0 / nrm;
}
