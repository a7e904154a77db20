// kf_dist_device.h — MapMaker::KeyFrameLinearDist (src/MapMaker.cc:696-703) and the (distance, keyframe) order of
// NClosestKeyFrames / ClosestKeyFrame (:711-752) on the device, for the kernels that choose keyframes by it: mba_select_kernel
// (mapba.hip, BundleAdjustRecent's four nearest) and rm_closest_kernel (maprmap.hip, ptam_rmap_closest_keyframes).
#pragma once
#include "patch_device.h"   // nc_mul / nc_add / nc_sub

// se3CfromW.inverse().get_translation() = -(R^T t), TooN's row dot products left to right, no contraction
__device__ __forceinline__ void mba_centre(const double* P, double c[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) c[i] = -nc_add(nc_add(nc_mul(P[i], P[9]), nc_mul(P[3 + i], P[10])), nc_mul(P[6 + i], P[11]));
}

// KeyFrameLinearDist(k1, k2) with c1 = k1's centre and P2 = k2's se3CfromW: v3Diff = c2 - c1, sqrt(v3Diff * v3Diff) (:700-702)
__device__ __forceinline__ double mba_linear_dist(const double c1[3], const double* P2) {
    double c[3];
    mba_centre(P2, c);
    const double dx = nc_sub(c[0], c1[0]), dy = nc_sub(c[1], c1[1]), dz = nc_sub(c[2], c1[2]);
    return sqrt(nc_add(nc_add(nc_mul(dx, dx), nc_mul(dy, dy)), nc_mul(dz, dz)));
}

// std::pair<double, KeyFrame*>::operator< with the keyframe index in place of the pointer
__device__ __forceinline__ bool mba_pair_less(double d1, int k1, double d2, int k2) { return d1 < d2 || (!(d2 < d1) && k1 < k2); }

// the least (bd, bk) of a 1024-thread workgroup by mba_pair_less; bk < 0: the thread has none.  Thread 0 holds the result
// afterwards; s_d / s_k: 16 words of shared memory each, free again after the caller's next __syncthreads()
__device__ __forceinline__ void mba_block_least(double& bd, int& bk, double* s_d, int* s_k) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (ok >= 0 && (bk < 0 || mba_pair_less(od, ok, bd, bk))) bd = od, bk = ok;
    }
    if (lane == 0) s_d[wid] = bd, s_k[wid] = bk;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < 16; w++)
            if (s_k[w] >= 0 && (bk < 0 || mba_pair_less(s_d[w], s_k[w], bd, bk))) bd = s_d[w], bk = s_k[w];
}
