// ba_update.inc — K10: point back-substitution, new error, finalize / purge / publish kernels (src/Bundle.cc:461-550).
// Textually included by bundle.hip (one translation unit: the kernels share BaDev and the helpers of ba_math.inc).
// =================================================================================================
// K10
// =================================================================================================
__global__ void __launch_bounds__(64) pose_update_kernel(BaDev d, int cur) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c < d.C) {
        const double* T = d.pose[cur] + 12 * c;
        double* Tn = d.pose[cur ^ 1] + 12 * c;
        const int f = d.cam_free[c];
        if (f < 0) {
#pragma unroll
            for (int i = 0; i < 12; i++) Tn[i] = T[i];
        } else {
            double mu[6], Tl[12], o[12];
#pragma unroll
            for (int i = 0; i < 6; i++) mu[i] = d.da[6 * f + i];
#pragma unroll
            for (int i = 0; i < 12; i++) Tl[i] = T[i];
            se3_exp_mul(mu, Tl, o);   // exp(da_j) * se3CfW  (:501)
#pragma unroll
            for (int i = 0; i < 12; i++) Tn[i] = o[i];
        }
    }
    if (blockIdx.x == 0) {
        double s = 0;
        for (int i = threadIdx.x; i < d.n; i += 64) s += d.da[i] * d.da[i];
        s = wave_sum_f64(s);
        if (threadIdx.x == 0) d.sumsq2[0] = s, d.sumsq2[1] = 0.0;
    }
}

// A chunk that is ONE point with more than BA_CHUNK measurements (a point seen by more than 256 keyframes): the same
// arithmetic, BA_CHUNK measurements at a time — W^T da summed per thread over its strided measurements, the threads' sums
// added in thread order by one wave (fixed order), then the new-error pass over the same strides.
template <bool LOADW>
__device__ void point_update_long(const DevCam& cam, const BaDev& d, int cur, int est, const BaChunk& ch, double (*Ts)[3], double (*wred)[2]) {
    const int tid = threadIdx.x, pp = ch.pt_begin;
    const size_t wp = w_plane(d);
    const double sig2 = d.sc->sigma_sq;
    const double Xc[3] = {d.pt[cur][(size_t)pp * 3], d.pt[cur][(size_t)pp * 3 + 1], d.pt[cur][(size_t)pp * 3 + 2]};
    double t0 = 0, t1 = 0, t2 = 0;
    for (int m = ch.m_begin + tid; m < ch.m_end; m += BA_CHUNK) {
        const int c = d.m_cam[m], f = d.cam_free[c];
        if (d.m_state[m] != MS_ALIVE || f < 0) continue;   // non-fixed, non-bad  (:469-474)
        const double* da = d.da + 6 * f;
        if (LOADW) {
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const double a0 = da[2 * h], a1 = da[2 * h + 1];
                const double2 w0 = *(const double2*)(d.W + 0 * wp + (size_t)m * 6 + 2 * h), w1 = *(const double2*)(d.W + 1 * wp + (size_t)m * 6 + 2 * h),
                              w2 = *(const double2*)(d.W + 2 * wp + (size_t)m * 6 + 2 * h);
                t0 += w0.x * a0 + w0.y * a1;
                t1 += w1.x * a0 + w1.y * a1;
                t2 += w2.x * a0 + w2.y * a1;
            }
        } else {   // W rebuilt from the current state (ba_rebuild_w), added in the same order
            double Tc[12], w[18];
#pragma unroll
            for (int i = 0; i < 12; i++) Tc[i] = d.pose[cur][12 * (size_t)c + i];
            ba_rebuild_w(cam, est, Tc, Xc, d.m_found[m], d.m_s[m], sig2, w);
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const double a0 = da[2 * h], a1 = da[2 * h + 1];
                t0 += w[(2 * h) * 3] * a0 + w[(2 * h + 1) * 3] * a1;
                t1 += w[(2 * h) * 3 + 1] * a0 + w[(2 * h + 1) * 3 + 1] * a1;
                t2 += w[(2 * h) * 3 + 2] * a0 + w[(2 * h + 1) * 3 + 2] * a1;
            }
        }
    }
    Ts[tid][0] = t0, Ts[tid][1] = t1, Ts[tid][2] = t2;
    __syncthreads();
    if (tid < 64) {
        double s0 = 0, s1 = 0, s2 = 0;
        for (int q = tid; q < BA_CHUNK; q += 64) s0 += Ts[q][0], s1 += Ts[q][1], s2 += Ts[q][2];
        s0 = wave_sum_f64(s0), s1 = wave_sum_f64(s1), s2 = wave_sum_f64(s2);
        if (tid == 0) {
            const double* eb = d.epsB + (size_t)pp * 3;
            const double* vi = d.Vinv + (size_t)pp * 9;
            const double* X = d.pt[cur] + (size_t)pp * 3;
            const double v0 = eb[0] - s0, v1 = eb[1] - s1, v2 = eb[2] - s2;
            const double d0 = vi[0] * v0 + vi[1] * v1 + vi[2] * v2, d1 = vi[3] * v0 + vi[4] * v1 + vi[5] * v2, d2 = vi[6] * v0 + vi[7] * v1 + vi[8] * v2;
            double* Xn = d.pt[cur ^ 1] + (size_t)pp * 3;
            Xn[0] = X[0] + d0, Xn[1] = X[1] + d1, Xn[2] = X[2] + d2;   // :503-504
            wred[0][0] = Xn[0], wred[0][1] = Xn[1], wred[1][0] = Xn[2], wred[1][1] = d0 * d0 + d1 * d1 + d2 * d2;
        }
    }
    __syncthreads();
    const double Xn[3] = {wred[0][0], wred[0][1], wred[1][0]};
    const double sq = wred[1][1];
    const double s2 = sig2;
    double err = 0;
    for (int m = ch.m_begin + tid; m < ch.m_end; m += BA_CHUNK) {   // FindNewError over every listed measurement (:188-207)
        if (d.m_state[m] == MS_DEAD) continue;
        BaProj pr;
        if (!ba_project(cam, d.pose[cur ^ 1] + 12 * d.m_cam[m], Xn, pr)) {
            err += 1.0;
            d.m_zbad_t[m] = 1;
        } else {
            const double2 fo = d.m_found[m];
            const double sn = d.m_s[m];
            const double ex = sn * (fo.x - pr.u), ey = sn * (fo.y - pr.v), e2n = ex * ex + ey * ey;
            err += ba_objective(est, e2n, s2, 1.0 / s2);
            d.m_e2t[m] = e2n;
            d.m_zbad_t[m] = 0;
        }
    }
    __syncthreads();   // (wred is reused below)
    err = wave_sum_f64(err);
    if ((tid & 63) == 0) wred[tid >> 6][0] = err;
    __syncthreads();
    if (tid == 0) {
        double e = 0;
        for (int i = 0; i < BA_CHUNK / 64; i++) e += wred[i][0];
        d.err_part[2 * blockIdx.x] = e;
        d.err_part[2 * blockIdx.x + 1] = sq;
    }
}

// delta b, trial points, new robust error; block owns whole points.  W_ij, which this kernel needs for sum_j W_ij^T da_j alone, is
// not read back from K7's planes (144 of the 176 bytes a measurement moved here) but rebuilt in registers from the current pose
// and point (ba_rebuild_w: ~200 fp64 instructions).  LOADW = true is the loading form, kept for comparison
// (PTAM_UPDATE_LOADS_W=1, bundle.hip).
template <bool LOADW>
__global__ void __launch_bounds__(BA_CHUNK) point_update_kernel(DevCam cam, BaDev d, int cur, int est) {
    TL_MARK(d, 11)
    __shared__ double Ts[BA_CHUNK][3];
    __shared__ double Np[BA_CHUNK][3];
    __shared__ double wred[BA_CHUNK / 64][2];
    const int tid = threadIdx.x;
    const BaChunk ch = d.chunks[blockIdx.x];
    if (ch.m_end - ch.m_begin > BA_CHUNK) {   // (uniform: a long point, alone in its chunk)
        point_update_long<LOADW>(cam, d, cur, est, ch, Ts, wred);
        return;
    }
    const int m = ch.m_begin + tid;
    const bool active = m < ch.m_end;
    // Every load of the workgroup leaves in ONE go, the small ones first: the measurement's record, the first round's per-point
    // data (V*^-1, epsB, the point — they depend on the chunk alone), then (LOADW) W, 144 of the ~190 bytes per measurement, and
    // behind it what hangs on the record: the camera's update and — for the rebuilt W — its current pose and the measurement's
    // own point, or (LOADW) its trial pose (cache hits).  Issued phase by phase (record -> free index -> update; the per-point
    // data after the first barrier; the pose after the second) each phase was a round trip queued behind the W stream of the
    // ~1 000 co-resident workgroups: 13 us for 47 MB.
    const int mc = min(m, d.M - 1);
    const int st = active ? (int)d.m_state[mc] : (int)MS_DEAD;
    const int c = d.m_cam[mc], p = d.m_pt[mc];
    const int f = d.m_fidx[mc];   // (= cam_free[c], bundle.hip)
    const double s2 = d.sc->sigma_sq;
    const double2 fo = d.m_found[mc];
    const double sn = d.m_s[mc];
    const int npts = ch.pt_end - ch.pt_begin;
    const int pi0 = tid >> 3, sub = tid & 7;
    const bool on0 = pi0 < npts;
    const int pp0 = ch.pt_begin + (on0 ? pi0 : 0);
    const int rq0 = d.rowptr[pp0], rq1 = d.rowptr[pp0 + 1];
    double vi[9], x[3], eb[3];
    {
        const double* Vi = d.Vinv + (size_t)pp0 * 9;
        const double* X = d.pt[cur] + (size_t)pp0 * 3;
        const double* E = d.epsB + (size_t)pp0 * 3;
#pragma unroll
        for (int i = 0; i < 9; i++) vi[i] = Vi[i];
#pragma unroll
        for (int i = 0; i < 3; i++) x[i] = X[i], eb[i] = E[i];
    }
    double w[18];   // row-major 6x3 again, from the three coordinate planes (bundle.h)
    if (LOADW) {
        const size_t wp = w_plane(d);
#pragma unroll
        for (int c3 = 0; c3 < 3; c3++)
#pragma unroll
            for (int h = 0; h < 3; h++) {
                const double2 t = *(const double2*)(d.W + c3 * wp + (size_t)mc * 6 + 2 * h);
                w[(2 * h) * 3 + c3] = t.x;
                w[(2 * h + 1) * 3 + c3] = t.y;
            }
    }
    double da[6], T[12], Tc[12], xm[3];
    {
        const double2* dq = (const double2*)(d.da + 6 * (size_t)max(f, 0));   // (48-byte pitch: 16-byte aligned)
        const double2* Tq = (const double2*)(d.pose[cur ^ 1] + 12 * (size_t)c);
        if (!LOADW) {
            const double2* Cq = (const double2*)(d.pose[cur] + 12 * (size_t)c);
            const double* Xm = d.pt[cur] + (size_t)p * 3;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double2 t = Cq[i];
                Tc[2 * i] = t.x, Tc[2 * i + 1] = t.y;
            }
#pragma unroll
            for (int i = 0; i < 3; i++) xm[i] = Xm[i];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double2 t = dq[i];
            da[2 * i] = t.x, da[2 * i + 1] = t.y;
        }
        if (LOADW) {
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double2 t = Tq[i];
                T[2 * i] = t.x, T[2 * i + 1] = t.y;
            }
        }
    }
    double t0 = 0, t1 = 0, t2 = 0;
    if (st == MS_ALIVE && f >= 0) {   // non-fixed, non-bad  (:469-474)
        if (!LOADW) ba_rebuild_w(cam, est, Tc, xm, fo, sn, s2, w);
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const double a = da[r];
            t0 += w[r * 3] * a;
            t1 += w[r * 3 + 1] * a;
            t2 += w[r * 3 + 2] * a;
        }
    }
    if (!LOADW) {
        // (the trial pose is needed behind the second barrier only: asked for here, where the current pose's registers are
        //  free again, the kernel keeps its 128 VGPRs and four workgroups a CU; the two barriers and the per-point sums cover it)
        const double2* Tq = (const double2*)(d.pose[cur ^ 1] + 12 * (size_t)c);
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double2 t = Tq[i];
            T[2 * i] = t.x, T[2 * i + 1] = t.y;
        }
    }
    Ts[tid][0] = t0;
    Ts[tid][1] = t1;
    Ts[tid][2] = t2;
    __syncthreads();
    // per point: eight threads add strided slices of its measurements' terms, the slices meet in a fixed order (DPP)
    double sq = 0;
    for (int base = 0; base < npts; base += BA_CHUNK / 8) {
        const int pi = base + pi0;
        const bool on = pi < npts;
        const int pp = ch.pt_begin + (on ? pi : 0);
        int r0 = rq0 - ch.m_begin, r1 = on0 ? rq1 - ch.m_begin : r0;
        if (base != 0) {   // (more than 32 points in the chunk: further rounds fetch theirs here)
            r0 = d.rowptr[pp] - ch.m_begin, r1 = on ? d.rowptr[pp + 1] - ch.m_begin : r0;
            const double* Vi = d.Vinv + (size_t)pp * 9;
            const double* X = d.pt[cur] + (size_t)pp * 3;
            const double* E = d.epsB + (size_t)pp * 3;
#pragma unroll
            for (int i = 0; i < 9; i++) vi[i] = Vi[i];
#pragma unroll
            for (int i = 0; i < 3; i++) x[i] = X[i], eb[i] = E[i];
        }
        const double e0 = eb[0], e1 = eb[1], e2 = eb[2];
        double s0 = 0, s1 = 0, s2 = 0;
        for (int rr = r0 + sub; rr < r1; rr += 8) {
            s0 += Ts[rr][0];
            s1 += Ts[rr][1];
            s2 += Ts[rr][2];
        }
        s0 += dpp_row_shr_f64<1>(s0), s1 += dpp_row_shr_f64<1>(s1), s2 += dpp_row_shr_f64<1>(s2);
        s0 += dpp_row_shr_f64<2>(s0), s1 += dpp_row_shr_f64<2>(s1), s2 += dpp_row_shr_f64<2>(s2);
        s0 += dpp_row_shr_f64<4>(s0), s1 += dpp_row_shr_f64<4>(s1), s2 += dpp_row_shr_f64<4>(s2);
        if (on && sub == 7) {   // (lane 7 of the group holds the sum of its eight slices)
            const double v0 = e0 - s0, v1 = e1 - s1, v2 = e2 - s2;
            const double d0 = vi[0] * v0 + vi[1] * v1 + vi[2] * v2;
            const double d1 = vi[3] * v0 + vi[4] * v1 + vi[5] * v2;
            const double d2 = vi[6] * v0 + vi[7] * v1 + vi[8] * v2;
            sq += d0 * d0 + d1 * d1 + d2 * d2;
            const double n0 = x[0] + d0, n1 = x[1] + d1, n2 = x[2] + d2;   // :503-504
            double* Xn = d.pt[cur ^ 1] + (size_t)pp * 3;
            Xn[0] = n0;
            Xn[1] = n1;
            Xn[2] = n2;
            Np[pi][0] = n0;
            Np[pi][1] = n1;
            Np[pi][2] = n2;
        }
    }
    __syncthreads();
    double err = 0;
    if (active && st != MS_DEAD) {   // FindNewError over every listed measurement (:188-207)
        const double* X = Np[p - ch.pt_begin];
        BaProj pr;
        if (!ba_project(cam, T, X, pr)) {
            err = 1.0;
            d.m_zbad_t[m] = 1;
        } else {
            const double ex = sn * (fo.x - pr.u), ey = sn * (fo.y - pr.v);
            const double e2n = ex * ex + ey * ey;
            err = ba_objective(est, e2n, s2, 1.0 / s2);
            // if this trial is accepted, these ARE pass 1's results of the next LM step (same poses,
            // points and projection code): keep them so that the next step can skip its projection pass
            d.m_e2t[m] = e2n;
            d.m_zbad_t[m] = 0;
        }
    }
    err = wave_sum_f64(err);
    sq = wave_sum_f64(sq);
    if ((tid & 63) == 0) {
        wred[tid >> 6][0] = err;
        wred[tid >> 6][1] = sq;
    }
    __syncthreads();
    if (tid == 0) {
        double e = 0, s = 0;
        for (int i = 0; i < BA_CHUNK / 64; i++) {
            e += wred[i][0];
            s += wred[i][1];
        }
        d.err_part[2 * blockIdx.x] = e;
        d.err_part[2 * blockIdx.x + 1] = s;
    }
}

// The trial's outcome from the point update's per-chunk sums: new error, |db|^2, and the host's decision (src/Bundle.cc:338,
// :488-490, :518-533) taken on the device as well, for the kernels that were enqueued before the host has seen it.  One workgroup of
// 256 threads; fixed assignment + fixed combine order: the same bits in every workgroup that calls it.
struct BaDecision {
    double new_err, sumsq_pt, sumsq_cam;
    int end_step, go, stay;
};
__device__ __forceinline__ BaDecision ba_decide(const BaDev& d, double conv_limit, int last_allowed) {
    __shared__ double w[4][2];
    double e = 0, s = 0;
    // (what the decision needs leaves now, with the sums' loads: asked for after the reduction it was one more round trip on the chain)
    const double ce_pre = d.sc->cur_err, sq0_pre = d.sumsq2[0], sq1_pre = d.sumsq2[1];
    const int fault_pre = d.sc->solve_fault;
    // (four blocks' sums per thread and round, loaded before they are added — same order of additions: a pair per round is a
    //  round trip per pair, twelve in a row at 3 000 blocks)
    for (int base = 0; base < d.n_chunks; base += 1024) {
        double2 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *(const double2*)&d.err_part[2 * min(base + u * 256 + (int)threadIdx.x, d.n_chunks - 1)];
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (base + u * 256 + (int)threadIdx.x < d.n_chunks) {
                e += v[u].x;
                s += v[u].y;
            }
    }
    e = wave_sum_f64(e);
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) {
        w[threadIdx.x >> 6][0] = e;
        w[threadIdx.x >> 6][1] = s;
    }
    __syncthreads();
    BaDecision r;
    r.new_err = w[0][0] + w[1][0] + w[2][0] + w[3][0];
    r.sumsq_pt = w[0][1] + w[1][1] + w[2][1] + w[3][1];
    r.sumsq_cam = sq0_pre + sq1_pre;   // |da|^2, left in two parts by the backward substitution (solve.hip)
    const double ne = r.new_err, ce = ce_pre;
    const bool conv = r.sumsq_cam + r.sumsq_pt < conv_limit;
    const bool end_step = !(ne > ce) || conv || last_allowed != 0;
    // (a void solve — the persistent factorisation gave up a wait, solve.hip — decides nothing: the guarded kernels behind
    //  this one leave at once, the host repeats the trial)
    const bool ok = fault_pre == 0;
    r.end_step = (ok && end_step) ? 1 : 0;
    r.go = (ok && end_step && ne < ce && !conv && last_allowed == 0) ? 1 : 0;
    r.stay = (ok && end_step && !(ne < ce) && !conv && last_allowed == 0) ? 1 : 0;
    return r;
}
// ... written to the scalar block and, on single-device runs, published to the host from here (publish_scalars_kernel's job, one
// launch less per trial): by ONE workgroup
__device__ __forceinline__ void ba_decision_out(const BaDev& d, const BaDecision& r, ulonglong2* host_slots, unsigned long long seq) {
    if (threadIdx.x == 0) {
        d.sc->new_err = r.new_err;
        d.sc->sumsq_pt = r.sumsq_pt;
        d.sc->sumsq_cam = r.sumsq_cam;
        d.sc->spec_seq = (int)seq;
        d.sc->end_step = r.end_step;
        d.sc->spec_go = r.go;
        d.sc->spec_stay = r.stay;
    }
    if (host_slots) {
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x < sizeof(BaScalars) / 8)
            host_slots[threadIdx.x] = make_ulonglong2(((const volatile unsigned long long*)d.sc)[threadIdx.x], seq);
    }
}
__global__ void __launch_bounds__(256) finalize_new_kernel(BaDev d, double conv_limit, int last_allowed, ulonglong2* host_slots,
                                                            unsigned long long seq) {
    TL_MARK(d, 12)
    const BaDecision r = ba_decide(d, conv_limit, last_allowed);
    ba_decision_out(d, r, host_slots, seq);
}

// The trial's decision AND the next step's first launch in one: every workgroup works the decision out for itself (the same sums in
// the same order: the same bits), workgroup 0 writes it down and publishes the trial's scalars to the host, and all of them go on
// with what purge_pass1_kernel does behind that decision — the purge that closes the step and, from an accepted trial, pass 1 out
// of the trial's errors.  One dependent launch (finalize_new_kernel: 4.5 us, of which ~0.3 are work) less per trial; the
// redundant sums are 16 KB of loads per workgroup.  (The purge appends to the outlier list while workgroup 0 publishes: the
// host takes the list's length at the previous step's end from n_outliers_pub, which the last select left behind — bundle.h.)
__global__ void __launch_bounds__(256) purge_pass1_decide_kernel(BaDev d, double conv_limit, int last_allowed, ulonglong2* host_slots,
                                                                  unsigned long long seq) {
    TL_MARK(d, 1)
    const BaDecision r = ba_decide(d, conv_limit, last_allowed);
    if (blockIdx.x == 0) ba_decision_out(d, r, host_slots, seq);
    if (!r.end_step) return;
    const bool go = r.go != 0, stay = r.stay != 0;
    __shared__ unsigned hist[HIST_BINS];
    if (go || stay) hist_clear(hist);
    pass1_adopt<true>(d, go, go || stay, hist, stay);
    if (go || stay) hist_flush(d, hist);
}

// erase bad measurements, append to the outlier list (:536-547)
__global__ void __launch_bounds__(256) purge_kernel(BaDev d) {
    TL_MARK(d, 15)
    if (ba_guard_blocks(d)) return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool bad = m < d.M && d.m_state[m] == MS_BAD;
    const unsigned long long mask = __ballot(bad);
    if (mask == 0) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(&d.sc->n_outliers, __popcll(mask));   // one atomic per wave
    base = __shfl(base, 0, 64);
    if (bad) {
        d.outliers[base + __popcll(mask & ((1ull << lane) - 1ull))] = d.m_orig[m];
        d.m_state[m] = MS_DEAD;
    }
}

// The host's per-trial decision needs the scalars: they are written into host-mapped memory as
// (word, sequence) pairs, one 16-byte store per lane, and the host spins until every pair carries the
// expected sequence number — no system-scope fence on the device, no D2H copy + stream synchronise
// (~30 us of idle GPU per trial) on the host.
// Results leave the device through kernels too: poses, points and the outlier indices are stored straight into the
// context's host-mapped staging buffer, and a second (stream-ordered) launch stamps a sequence word the host spins on.
// The copy engine + hipStreamSynchronize pair this replaces slept on an interrupt and, about one Compute() in eight,
// took 7 ms instead of 70 us to wake up (PTAM_DEBUG_STALL: "compute total" against "compute loop").
__global__ void __launch_bounds__(256) readback_kernel(const double* __restrict__ pose, size_t n_pose, const double* __restrict__ pts,
                                                       size_t n_pts, const int* __restrict__ out, size_t n_out, double* __restrict__ h_pose,
                                                       double* __restrict__ h_pts, int* __restrict__ h_out) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = i0; i < n_pose; i += stride) h_pose[i] = pose[i];
    for (size_t i = i0; i < n_pts; i += stride) h_pts[i] = pts[i];
    for (size_t i = i0; i < n_out; i += stride) h_out[i] = out[i];
}
__global__ void stamp_kernel(volatile unsigned long long* slot, unsigned long long seq) { *slot = seq; }

#define MBOX_WORDS (sizeof(BaScalars) / 8)
static_assert(sizeof(BaScalars) % 8 == 0 && MBOX_WORDS <= 64, "published as 64-bit words by one wave");
__global__ void __launch_bounds__(64) publish_scalars_kernel(const BaScalars* sc, ulonglong2* host_slots, unsigned long long seq) {
    const unsigned i = threadIdx.x;
    if (i < MBOX_WORDS) host_slots[i] = make_ulonglong2(((const unsigned long long*)sc)[i], seq);
}

__global__ void set_scalars_kernel(BaDev d, double cur_err, int n_bad) {
    d.sc->cur_err = cur_err;
    d.sc->n_bad = n_bad;
}
__global__ void set_new_kernel(BaDev d, double new_err, double sumsq_pt) {
    d.sc->new_err = new_err;
    d.sc->sumsq_pt = sumsq_pt;
}
// sharded mode: the scalars that ride through an all-reduce.  which = 0: (current error, bad count) behind S|E;
// which = 1: (new error, |delta b|^2) at the end of a trial, plus THIS rank's abort flag as sampled by the host when
// the trial was enqueued — the sum makes the abort decision unanimous (every rank reads the same value with the
// trial's scalars and leaves the LM loops at the same trial; a rank-local test would strand the others in a collective)
__global__ void pack2_kernel(const BaScalars* sc, double* out, int which, int abort_local) {
    if (which == 0) {
        out[0] = sc->cur_err;
        out[1] = (double)sc->n_bad;
    } else {
        out[0] = sc->new_err;
        out[1] = sc->sumsq_pt;
        out[2] = abort_local ? 1.0 : 0.0;
        out[3] = sc->solve_fault ? 1.0 : 0.0;   // (a rank's void solve is every rank's: they repeat the trial together)
    }
}
__global__ void unpack2_kernel(BaScalars* sc, const double* in, int which) {
    if (which == 0) {
        sc->cur_err = in[0];
        sc->n_bad = (int)(in[1] + 0.5);
    } else {
        sc->new_err = in[0];
        sc->sumsq_pt = in[1];
        sc->abort_any = in[2] > 0.5 ? 1 : 0;
        sc->solve_fault = in[3] > 0.5 ? 1 : 0;
    }
}
__global__ void place_keys_kernel(const double* __restrict__ src, int n, double* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
