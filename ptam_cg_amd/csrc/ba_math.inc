// ba_math.inc — device helpers of the bundle kernels: histogram bins, projection (ProjectAndFindSquaredError), estimator pieces.
// Textually included by bundle.hip (one translation unit: the kernels share BaDev and the helpers of ba_math.inc).
// =================================================================================================
// device helpers
// =================================================================================================
// First-level bin of the order-statistic select: the top 16 bits of the fp64 pattern (exponent + 4
// mantissa bits = 16 sub-bins per binade) relative to 2^-24, clamped to [0, 4095] — monotone in the
// value, 256 binades wide (6e-8 .. 7e69).  A rank that lands in a clamped end bin takes the generic
// full-width radix path of select_final_kernel.
#define E2_BIN_BASE ((1023 - 24) << 4)
__device__ __forceinline__ int e2_bin(double e2) {
    const int t = (int)((unsigned long long)__double_as_longlong(e2) >> 48) - E2_BIN_BASE;
    return t < 0 ? 0 : (t > HIST_BINS - 1 ? HIST_BINS - 1 : t);
}
__device__ __forceinline__ int e2_bin2(double e2) {   // next 12 bits
    return (int)(((unsigned long long)__double_as_longlong(e2) >> 36) & (HIST_BINS - 1));
}

// Kernels of the NEXT LM step are enqueued before the host has seen the trial's outcome (the GPU would idle ~10 us
// per trial otherwise).  They carry d.guard != 0 and leave at once unless finalize_new_kernel decided on the device
// what the host is about to decide from the same numbers.
__device__ __forceinline__ int4 ba_guard_load(const BaDev& d) {   // end_step, spec_go, spec_stay, spec_seq: one scalar load
    return d.guard ? *(const int4*)&d.sc->end_step : make_int4(0, 0, 0, 0);
}
__device__ __forceinline__ bool ba_guard_blocks(const BaDev& d, const int4 f) {
    if (d.guard == 0) return false;
    if (f.w != d.guard_seq) return true;
    return d.guard == 1 ? (f.y == 0 && f.z == 0) : f.x == 0;
}
__device__ __forceinline__ bool ba_guard_stay(const BaDev& d, const int4 f) { return d.guard == 1 && f.z != 0; }   // "stay": the unchanged state again
__device__ __forceinline__ bool ba_guard_blocks(const BaDev& d) { return ba_guard_blocks(d, ba_guard_load(d)); }

// project one measurement: returns false (bad) if z <= 0  (ProjectAndFindSquaredError :164-180).
// Same arithmetic as cam_project / cam_derivs (common.h) with the divisions replaced by three
// Newton-refined reciprocals (1/z, 1/r, 1/(1+k^2 r^2)); pass 1, pass 2 and the new-error pass all
// go through this one function, so they see bit-identical projections.
struct BaProj {
    double X, Y, Z;      // v3Cam
    double x, y;         // z = 1 plane
    double u, v;         // image
    double r, ir, f;     // radius, 1/r, rtrans_factor
};
// atan for x >= 0 in ~45 VALU instructions (the library call is ~80 and sits in K7's critical VALU
// budget): argument reduction atan(x) = atan(c) + atan((x - c) / (1 + c x)) with c in {0, 1/2, 1, 3/2}
// (x >= 39/16: pi/2 - atan(1/x)) and the classic 11-term odd minimax polynomial on |t| < 7/16
// (Sun fdlibm's published coefficients); the quotient uses rcp + 2 Newton steps.  Measured against
// libm over [1e-8, 1e3]: <= 2 ulp (constants: tests/test_oracle_kat.py::test_atan_reduction_constants;
// the device code itself is covered by the BA parity tests).
// The constants come from a __constant__ table: uniform loads put them in SGPRs, which a VOP3 fp64
// instruction reads directly — as literals each use would cost two v_mov_b32 and a VGPR pair.
__constant__ double BA_ATAN_K[20] = {
    3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01,  -1.11111104054623557880e-01,
    9.09088713343650656196e-02,  -7.69187620504482999495e-02, 6.66107313738753120669e-02,  -5.83357013379057348645e-02,
    4.97687799461593236017e-02,  -3.65315727442169155270e-02, 1.62858201153657823623e-02,
    4.63647609000806093515e-01,  7.85398163397448278999e-01,  9.82793723247329054082e-01,  1.57079632679489655800e+00,
    0.4375, 0.6875, 1.1875, 2.4375, 1.5};
__device__ __forceinline__ double ba_atan_pos(double x) {
    const double* __restrict__ K = BA_ATAN_K;
    double c = 0.0, hi = 0.0;
    if (x >= K[15]) c = 0.5, hi = K[11];
    if (x >= K[16]) c = 1.0, hi = K[12];
    if (x >= K[17]) c = K[19], hi = K[13];
    double num = x - c, den = fma(c, x, 1.0);
    if (x >= K[18]) {
        num = -1.0;
        den = x;
        hi = K[14];
    }
    const double t = num * rcp_nr(den);
    const double z = t * t, w = z * z;
    // v_fma_f64 with the coefficient as an SGPR operand (left alone the compiler picks v_fmac and
    // first copies every coefficient into a VGPR pair)
#define FMA_SK(a, b, k) ({ double r_; asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r_) : "v"(a), "v"(b), "s"(k)); r_; })
    double p1 = FMA_SK(w, K[10], K[8]);   // (K[10] is copied once: two scalar operands are not encodable)
    p1 = FMA_SK(w, p1, K[6]);
    p1 = FMA_SK(w, p1, K[4]);
    p1 = FMA_SK(w, p1, K[2]);
    p1 = FMA_SK(w, p1, K[0]);
    double p2 = FMA_SK(w, K[9], K[7]);
    p2 = FMA_SK(w, p2, K[5]);
    p2 = FMA_SK(w, p2, K[3]);
    p2 = FMA_SK(w, p2, K[1]);
#undef FMA_SK
    const double s1 = z * p1, s2 = w * p2;
    return hi - (t * (s1 + s2) - t);
}
// 1/sqrt(a), a > 0: v_rsq_f64 + 2 Newton steps (<= 1 ulp)
__device__ __forceinline__ double rsq_nr(double a) {
    double y = __builtin_amdgcn_rsq(a);
    const double h = 0.5 * a;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}
__device__ __forceinline__ bool ba_project(const DevCam& cam, const double* __restrict__ T, const double* __restrict__ X,
                                           BaProj& p) {
    se3_apply(T, X[0], X[1], X[2], p.X, p.Y, p.Z);
    if (p.Z <= 0) return false;
    const double iz = rcp_nr(p.Z);
    p.x = p.X * iz;
    p.y = p.Y * iz;
    const double r2 = p.x * p.x + p.y * p.y;
    if (r2 < 1e-6 || cam.w == 0.0) {   // r < 0.001  (src/ATANCamera.h:105-111)
        p.r = r2 > 0 ? r2 * rsq_nr(r2) : 0.0;
        p.ir = 0;
        p.f = 1.0;
    } else {
        p.ir = rsq_nr(r2);
        p.r = r2 * p.ir;
        const double t = p.r * cam.two_tan;   // (negative only for a negative FOV parameter)
        p.f = cam.w_inv * copysign(ba_atan_pos(fabs(t)), t) * p.ir;
    }
    p.u = cam.cx + cam.fx * (p.f * p.x);
    p.v = cam.cy + cam.fy * (p.f * p.y);
    return true;
}
// GetProjectionDerivs (src/ATANCamera.cc:179-209): dFdx = x*g, dFdy = y*g with the common factor
// g = [ (k/w)/(1+k^2 r^2) - f ] / r^2
__device__ __forceinline__ void ba_derivs(const DevCam& cam, const BaProj& p, double D[4]) {
    const double r = p.r * cam.dist_enabled;
    double g = 0.0;
    if (!(r < 0.01)) {
        const double k = cam.two_tan;
        const double iden = rcp_nr(1 + k * k * r * r);
        g = (cam.w_inv * k * iden - p.f) * (p.ir * p.ir);
    }
    const double dx = p.x * g, dy = p.y * g;
    D[0] = cam.fx * (dx * p.x + p.f);
    D[2] = cam.fy * (dx * p.y);
    D[1] = cam.fx * (dy * p.x);
    D[3] = cam.fy * (dy * p.y + p.f);
}
// Tukey with a precomputed 1/sigma^2 (other estimators keep their general form)
__device__ __forceinline__ double ba_sqrt_weight(int est, double e2, double s2, double is2) {
    if (est == PTAM_EST_TUKEY) return e2 > s2 ? 0.0 : 1.0 - e2 * is2;
    return est_sqrt_weight(est, e2, s2);
}
// W_ij = A^T B (6x3, row-major) of one measurement K7 found alive with a free camera, from what K7 formed it from: the CURRENT
// pose and point, the measurement's record and sigma^2 — K7's expressions in K7's order (ba_jacobian.inc, the `full` branch and
// the W stores).  The point update rebuilds W with this instead of reading 144 bytes per measurement back; K7 keeps its own
// text (its register budget is tuned by hand).  A measurement K7 gave weight 0 is MS_BAD by now and never gets here.
__device__ __forceinline__ void ba_rebuild_w(const DevCam& cam, int est, const double* __restrict__ T, const double* __restrict__ Xp,
                                             double2 fo, double sn, double sigma_sq, double w18[18]) {
    BaProj pr;
    ba_project(cam, T, Xp, pr);
    const double ex = sn * (fo.x - pr.u), ey = sn * (fo.y - pr.v);
    const double w = ba_sqrt_weight(est, ex * ex + ey * ey, sigma_sq, 1.0 / sigma_sq);
    double D[4];
    ba_derivs(cam, pr, D);
    const double sw = sn * w;
    const double D0 = sw * D[0], D1 = sw * D[1], D2 = sw * D[2], D3 = sw * D[3];
    const double X = pr.X, Y = pr.Y, Z = pr.Z;
    const double iz = rcp_nr(Z);
    double B0[3], B1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double g0 = T[k], g1 = T[3 + k], g2 = T[6 + k];
        const double mx = (g0 - X * g2 * iz) * iz, my = (g1 - Y * g2 * iz) * iz;
        B0[k] = D0 * mx + D1 * my;
        B1[k] = D2 * mx + D3 * my;
    }
    const double zx = -X * iz * iz, zy = -Y * iz * iz;
    const double mxs[6] = {iz, 0, zx, zx * Y, iz * Z - zx * X, -iz * Y};
    const double mys[6] = {0, iz, zy, -iz * Z + zy * Y, -zy * X, iz * X};
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double A0 = D0 * mxs[k] + D1 * mys[k], A1 = D2 * mxs[k] + D3 * mys[k];
#pragma unroll
        for (int c = 0; c < 3; c++) w18[k * 3 + c] = A0 * B0[c] + A1 * B1[c];
    }
}
__device__ __forceinline__ double ba_objective(int est, double e2, double s2, double is2) {
    if (est == PTAM_EST_TUKEY) {
        if (e2 > s2) return 1.0;
        const double dd = 1.0 - e2 * is2;
        return 1.0 - dd * dd * dd;
    }
    return est_objective(est, e2, s2);
}
