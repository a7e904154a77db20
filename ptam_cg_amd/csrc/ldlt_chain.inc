// ldlt_chain.inc — K9 as ONE persistent launch (solve.hip): the camera system's LDL^T with forward substitution, the
// chain through the pivot blocks on one workgroup that never waits for a kernel boundary, the rest of the matrix on one
// workgroup per block row, the right-hand side on one more.  (`Cholesky<>(mS).backsub(vE)`, src/Bundle.cc:457-458.)
//
// Why: a step of the launch-per-block-column form costs 8.3 us of which the factorisation of the 32x32 pivot block is ~4;
// the rest is the dependent launch (2.3 us), the first global loads of a fresh workgroup (1.5 us: the data was written by
// other CUs a moment ago) and the closing products.  Here:
//   role 0, the CHAIN: for k = 0, 1, ...: factor A_kk on the matrix cores (ldlt_factor2.inc; the carried identity
//     gives Lkk^-T); store Lkk^-T and D_k; then row k+1's LAST step, which is the chain's own: X = A(k+1,k) Lkk^-T,
//     L(k+1,k) = X D^-1 (stored), A(k+1,k+1) -= X L^T, the flags F[k] and XF[k+1][k] — and on with block k+1.  NOTHING
//     else is on the chain: what row k+1's worker left of A(k+1,k), A(k+1,k+1) is fetched into LDS WHILE block k is being
//     factored, by the two waves that have no quadrant left after column 15, and the right-hand side is somebody else's.
//   role r-1, ROW WORKER of block row r >= 2: keeps the row's in-band tiles A(r, j0..r) in LDS.  Up-looking: for every
//     pivot block m <= r-2 in the band, as soon as F[m] is up: L(r,m) = A(r,m) Lmm^-T D_m^-1 (stored, flag XF[r][m]),
//     and A(r,j) -= X(r,m) L(j,m)^T for j = m+1..r, L(j,m) being the rows above's (their flags; all polled, then all
//     fetched, then all multiplied) or its own.  After m = r-2 the tiles (r,r-1), (r,r) go back to S for the chain (RF[r]).
//   last role, the RIGHT-HAND SIDE: b in LDS; for m = 0, 1, ...: F[m] up -> z_m = (Lmm^-T)^T b_m (stored: d.y), then
//     b_j -= L(j,m) z_m for the rows below as their XF[j][m] come up.  It follows the factorisation at a distance of one
//     hop and ends ~1 us after the chain; on the chain the same work cost ~0.5 us PER BLOCK.
//   behind them, systems of up to CH_FI_MAX_NB block rows (the FORWARD-INVERSE form, do_bw == 2 below): COLUMN WORKER j, one
//     per block column: the 32 identity columns of block j carried down the factorisation like the right-hand side — its
//     columns of L^-1, block row by block row, each multiplied into x_j as soon as the right-hand side has published that
//     block's w = D^-1 z.  The backward substitution — 12 us on one compute unit behind the chain at 10 block rows — is gone;
//     what follows the chain's last flag is 2.9 us: z of the last block, a hop, a tile product and a mat-vec in every column
//     worker at once, a hop, the trial poses.
// Hand-offs.  A hop "stores -> flag -> poll -> loads" costs 1.1-1.8 us with write-through (sc1) payload stores, wherever the
// two workgroups sit, and 0.7-1.0 us with plain stores when both sit on the SAME XCD — whose L2 then serves the reader's
// agent-scope loads; across XCDs plain stores are never seen (tools/pingpong).  The chain can only run ahead of its
// suppliers with the short hop (supply path: two hops + three tile products against 4.7 us per pivot block).  So the launch
// is 8 x the workgroups it needs and only blocks 0, 8, 16 ... work: block b is observed to run on XCD b % 8.  That is an
// observation, not a contract, so it is CHECKED: every working workgroup records its XCC id (hardware register), the chain
// compares them before its first publication and says in every F flag whether plain stores may be used; a launch that
// was spread over several XCDs falls back to write-through stores — slower, never stale.  Flags themselves are always
// agent-scope atomics, loads of handed-over data always agent-scope (never served by the reader's L1).  Flags are never
// cleared: a flag is up when it holds THIS solve's sequence number.  Every working workgroup of the launch is resident at
// once (at most nblk of them, 2 nblk <= 26 with column workers, 256 threads, a CU each), which the spinning relies on; a
// spin is bounded all the same and raises d.sflags[0] when it gives up (the backward kernel passes that on:
// BaScalars::solve_fault, ptam_ba_* returns PTAM_E_HIP).
struct ChainLds {
    double PF[2][2][NB][6];  // the factor loop's panel (ldlt_factor2.inc: [buffer][K | I][row][4 columns + pad])
    double T0[NB * LDP];     // Lkk^-T
    double T1[NB * LDP];     // X  (A operand of the tile products)
    double T2[NB * LDP];     // X D^-1 = L  (B operand)
    double T3[NB * LDP];     // the chain: A(k+1,k) as its worker left it, staged during the factorisation of block k
    double T4[NB * LDP];     //            A(k+1,k+1), likewise
    double iD[NB], Dv[NB], z[NB];
    double zp[8][NB];
    int one_xcd;
    int staged[2];           // T3 / T4 are filled
};
#define CH_TS (NB * LDP)   // doubles per LDS tile of a row worker
#define CH_MAX_NB 28       // block rows up to which the persistent form is used (ba_solve): every working workgroup — one per block row, up to a CU's LDS each — must be resident on ONE XCD (32 CUs)
#define CH_LDS_MAX (160 * 1024)
// dynamic LDS of a launch: the common part, then a row worker's in-band tiles (the right-hand side's vector fits in their place)
__host__ __device__ __forceinline__ size_t ch_lds_bytes(int band) { return sizeof(ChainLds) + 8 + (size_t)(band + 1) * CH_TS * sizeof(double); }
// the same when the right-hand-side workgroup also substitutes backwards (whole system in one chain): w = D^-1 z, the solution
// and CH_BW_SL fixed-order slices of the pending sums, all over the system's rows
#define CH_BW_SL 12
__host__ __device__ __forceinline__ size_t ch_lds_bytes_bw(int band, int nblk) {
    const size_t rhs = (size_t)(2 + CH_BW_SL) * nblk * NB + NB, tiles = (size_t)(band + 1) * CH_TS;
    return sizeof(ChainLds) + 8 + (rhs > tiles ? rhs : tiles) * sizeof(double);
}
// the same for the forward-inverse form (do_bw == 2): a column worker carries the block rows j .. nblk-1 of its 32 columns of L^-1,
// at most nblk tiles (L^-1 is dense below the diagonal whatever the band of L); the right-hand side needs two vectors
__host__ __device__ __forceinline__ size_t ch_lds_bytes_fi(int band, int nblk) {
    return sizeof(ChainLds) + 8 + (size_t)(band + 1 > nblk ? band + 1 : nblk) * CH_TS * sizeof(double);
}
#define CH_FI_MAX_NB 13    // block rows up to which the forward-inverse form is used: 13 tiles beside ChainLds fill a CU's LDS, and 2 x 13 working workgroups fit one XCD (32 CUs)
#define CH_BW_MAXT 9       // in-band tiles left of the diagonal up to which the right-hand-side workgroup substitutes backwards itself: two register sets of so many tiles (dense: 10 block rows = the 50-keyframe headline; beyond, ldlt_backward_kernel follows the launch)
// Looks a waiting workgroup takes before it gives up (BaDev::spin_limit; PTAM_CH_SPIN_LIMIT overrides): ~0.25 s.  A legitimate
// wait is microseconds; what a wait can run into is a partner that was never dispatched — two persistent solves on one device
// (two processes sharing a GPU), each holding part of the XCD's CUs.  The solve is then reported as void (BaScalars::solve_fault)
// and the host repeats the trial with the launch-per-block-column form, which cannot wait for anybody.  A wait also ends at
// once when ANOTHER wait of this solve has already given up (the error word carries this solve's number).

__device__ __forceinline__ double ch_ld(const double* p) {
    return __longlong_as_double(__hip_atomic_load((const long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// payload store: plain when every working workgroup sits on one XCD (its L2 serves the readers), write-through otherwise
__device__ __forceinline__ void ch_st(double* p, double v, bool one_xcd) {
    if (one_xcd)
        *p = v;   // (ordered by the asm "s_waitcnt vmcnt(0)" + memory clobber in front of every flag store; a volatile store would be sc0 sc1)
    else
        __hip_atomic_store((long long*)p, __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 16 bytes per lane at agent scope (no such atomic load in the language): an asm load the compiler does not count — the caller
// waits for it with ch_ld2_wait before it touches the value
__device__ __forceinline__ void ch_ld2_issue(double2& v, const double2* p) { asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory"); }
__device__ __forceinline__ void ch_ld2_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// a flag goes up (the caller has waited for its stores and passed a workgroup barrier): on one XCD a plain store — the word stays
// in the L2 the pollers read, an agent-scope store would send every poll to memory (2 000 cycles instead of 700)
__device__ __forceinline__ void ch_raise(unsigned* f, unsigned seq, bool one_xcd) {
    const unsigned v = (seq << 1) | (one_xcd ? 1u : 0u);
    if (one_xcd)
        // (as an instruction: a volatile C++ store came out as "flat_store_dword ... sc0 sc1" — written through to memory, and
        //  a FLAT access counts on lgkmcnt too: the chain's next LDS wait then waited for the flag to reach memory, 1 500 cycles)
        asm volatile("global_store_dword %0, %1, off" ::"v"(f), "v"(v) : "memory");
    else
        __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ch_flag(const unsigned* f) { return __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// one lane waits until the flag carries this solve's sequence number (bit 0 of a flag: "plain stores in use"); returns the flag
__device__ __forceinline__ unsigned ch_wait(const unsigned* f, unsigned seq, unsigned* err, int limit) {
    int spins = 0;
    unsigned v;
    while (((v = ch_flag(f)) >> 1) != seq) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > limit || ((spins & 255) == 0 && ch_flag(err) == seq)) {
            __hip_atomic_store(err, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
    return v;
}
// every lane with `active` waits for its own flag, the wave goes on when all are up: ONE round trip per look whatever the
// number of flags (looked at one after the other, a row worker's seven flags cost it seven round trips per step — 3 us)
__device__ __forceinline__ void ch_wait_lanes(const unsigned* f, bool active, unsigned seq, unsigned* err, int limit) {
    int spins = 0;
    for (;;) {
        const bool up = !active || (ch_flag(f) >> 1) == seq;
        if (__builtin_amdgcn_ballot_w64(!up) == 0) break;
        __builtin_amdgcn_s_sleep(1);
        if (++spins > limit || ((spins & 255) == 0 && ch_flag(err) == seq)) {
            __hip_atomic_store(err, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
}
// working workgroups of a launch: the chain, the row workers of rows 2 .. nblk-1, the right-hand side
__host__ __device__ __forceinline__ int ch_roles(int nblk) { return nblk > 2 ? nblk : 2; }
// ... and, behind them, the column workers of the forward-inverse form: one per block column
__host__ __device__ __forceinline__ int ch_roles_fi(int nblk) { return ch_roles(nblk) + nblk; }
// flag words: [0] error, then F[nblk], RF[nblk], XCC[nblk + 1], XF[nblk][band + 1], and for the forward-inverse form WF[nblk]
// (w_m = D_m^-1 z_m is published), XD[nblk] (column worker j has stored x_j), XCC2[nblk] (the column workers' XCC ids)
__host__ __device__ __forceinline__ size_t ch_flag_words(int nblk, int band) { return 2 + 6 * (size_t)nblk + (size_t)nblk * (band + 1); }

// What one chain of a launch works on.  [k0, k1): the block columns it eliminates; kr: one past the last block row that receives
// their updates (k1 when nothing below takes part: the whole system, or the middle part of a two-ended elimination, whose
// multipliers towards the two chains' columns are final; min(nblk, k1 + band) for one of the two chains themselves: the rows
// below k1 are updated and go back to S / E).  n: rows before the identity padding of the LAST block (npad: none to skip).
// A launch runs ONE chain (club 0: blocks 0, 8, 16 ... -> XCD 0) or TWO independent ones (club 1: blocks 1, 9, 17 ... -> XCD 1
// works on `b`, the bottom end of a banded system mirrored into buffers of its own: ldlt_mirror_in_kernel).
struct ChainArgs {
    double *S, *E, *L, *Dg, *y;
    unsigned* flags;
    int k0, k1, kr, n;
};
// do_bw (one chain over the WHOLE system only): no ldlt_backward_kernel behind this launch, da, the trial poses pose[cur ^ 1] and
// |da|^2 are written here.  1: the right-hand-side workgroup goes on with D^-1 and the backward substitution.  2, the
// FORWARD-INVERSE form: there is no backward pass.  x = L^-T w, w = D^-1 z, is x_j = sum_{m >= j} Y(m,j)^T w_m with Y = L^-1,
// and Y is the forward substitution of the identity — what the right-hand-side workgroup does for one column, done for the 32
// columns of block j by COLUMN WORKER j (role n_roles + j), behind the factorisation like the right-hand side and with its flags:
//   R(j) = I, R(jb) = 0 below (LDS);  for m = j, j+1, ...:  F[m] up -> Y(m,j) = (Lmm^-T)^T R(m);  XF[jb][m] up -> R(jb) -=
//   L(jb,m) Y(m,j) for the in-band rows below;  WF[m] up (the right-hand side has published w_m: d.bw_scratch) -> x_j += Y(m,j)^T w_m,
//   eight partial sums per column in registers, block rows in ascending order, added in a fixed tree at the end: the same bits
//   on every rank.  After the last block: x_j -> d.da, flag XD[j].
// The right-hand-side workgroup waits for the XD flags, takes da back into LDS and finishes as form 1 does.  What follows the
// chain's last flag is z_last, one hop, a 32x32 product and mat-vec in every column worker at once, one hop, the poses.
__global__ void __launch_bounds__(TPB, 2) ldlt_chain_kernel(BaDev d, ChainArgs a0, ChainArgs a1, int clubs, int cur, int do_bw) {
    const int club = ((int)(blockIdx.x & 7) - d.chain_xcd) & 7;   // (the bundle's XCD takes chain 0, the next one chain 1)
    if (club >= clubs) return;   // (only one or two of every eight blocks work: one XCD per chain, see above)
    const ChainArgs& a = club == 0 ? a0 : a1;
    const int k0 = a.k0, k1 = a.k1, kr = a.kr;
    const int role = blockIdx.x >> 3;
    if (role == 0 && club == 0) { TL_MARK(d, 9) }
    extern __shared__ __attribute__((aligned(16))) double ch_lds[];
    ChainLds& s = *(ChainLds*)ch_lds;
    const int band = se_band(d), nblk = d.npad / NB;
    const int n_roles = ch_roles(kr - k0);
    const int n_col = do_bw == 2 ? kr - k0 : 0;   // column workers (forward-inverse form: k0 = 0, kr = nblk)
    if (role >= n_roles + n_col) return;
    const unsigned seq = d.solve_seq;
    unsigned* const err = d.sflags;   // (one error word for the launch: the first chain's)
    unsigned* const F = a.flags + 1;
    unsigned* const RF = F + nblk;
    unsigned* const XCC = RF + nblk;
    unsigned* const XFb = XCC + nblk + 1;
    unsigned* const WF = XFb + (size_t)nblk * (band + 1);
    unsigned* const XD = WF + nblk;
    unsigned* const XCC2 = XD + nblk;
    auto XF = [&](int r, int m) { return XFb + (size_t)r * (band + 1) + (m - max(0, r - band)); };
    double* __restrict__ S = a.S;
    double* __restrict__ E = a.E;
    double* __restrict__ Lf = a.L;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int qi = w >> 1, qj = w & 1;
    const int i16 = lane & 15, m4 = lane >> 4;
    const int colq = 16 * qj + i16;   // my column of an accumulator quadrant (its rows: 16 qi + m4 + 4 v)
    // where am I: HW_REG_XCC_ID (hwreg 20, bits 3:0), recorded with the solve's sequence number
    const unsigned my_xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) & 0xf;
    if (tid == 0) __hip_atomic_store(role < n_roles ? XCC + role : XCC2 + (role - n_roles), (seq << 4) | my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // a 32x32x32 product on the matrix cores, quadrant (qi, qj):  sum_k A[16 qi + i][k] * Bt[16 qj + j][k]
    //   A operand lane (i, m) = A[16 qi + i][4 kk + m], B operand lane (j, m) = Bt[16 qj + j][4 kk + m]
    auto mma_t = [&](const double* A, const double (&bt)[NB / 4]) {
        v4f64 acc = {0, 0, 0, 0};
        const double* pa = A + (16 * qi + i16) * LDP + m4;
        double a8[NB / 4];
#pragma unroll
        for (int kk = 0; kk < NB / 4; kk++) a8[kk] = pa[4 * kk];
#pragma unroll
        for (int kk = 0; kk < NB / 4; kk++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a8[kk], bt[kk], acc, 0, 0, 0);
        return acc;
    };
#ifdef K7_TIMING   // cycle stamps of the chain's wave 3 (tools/ldlt builds only): 4 per step
    int nst_ = 0;
#define CH_STAMP() if (role == 0 && threadIdx.x == 192 && nst_ < 200) d.dbg[32 + nst_++] = (long long)__builtin_readcyclecounter();
#define CH_SEEN(t_) if (lane == 0) d.dbg[440 + k] = d.dbg[456 + k] = 100 + (t_);
#define CH_RT(slot) d.dbg[600 + (slot)] = (long long)__builtin_amdgcn_s_memrealtime();
#else
#define CH_STAMP()
#define CH_SEEN(t_)
#define CH_RT(slot)
#endif
    if (role == 0) {
        // ================================ the chain ================================
        const double e0 = m4 == 0 ? 1.0 : 0.0, e1 = m4 == 1 ? 1.0 : 0.0, e2 = m4 == 2 ? 1.0 : 0.0, e3 = m4 == 3 ? 1.0 : 0.0;
        v4f64 accK;
#pragma unroll
        for (int v = 0; v < 4; v++) {   // block (0,0): written by the previous kernel, lower triangle completed symmetrically
            const int row = 16 * qi + m4 + 4 * v;
            accK[v] = S[se_blk(k0, k0, band) + max(row, colq) * NB + min(row, colq)];
        }
        bool one_xcd = false;    // decided before the first publication
        for (int k = k0; k < k1; k++) {
            v4f64 accI;
            const int niter = (min(NB, a.n - k * NB) + 3) / 4;   // (the last block ends in identity padding: skipped)
            if (tid < NB) {
                s.iD[tid] = 1.0;
                s.Dv[tid] = 1.0;
            }
            // Row k+1's tiles as its worker left them (row 1: as the previous kernel left them) are fetched WHILE block k is
            // being factored, by the wave that has nothing left to do after column 15 (ldlt_factor2.inc: wave 0): A(r,k) into
            // T3, then A(r,r) into T4 — one poll of the worker's flag per iteration, a tile per iteration once it is up.  Its
            // waits are its own: the factorisation's waves never wait for memory.  (Polling from the working waves cost the
            // chain a round trip per poll: the compiler makes a uniform flag a scalar at once.)
            const int r = k + 1;
            const bool have_row = r < kr;
            const size_t o_rk = have_row ? se_blk(r, k, band) : 0, o_rr = have_row ? se_blk(r, r, band) : 0;
            if (tid < 2) s.staged[tid] = 0;
            int stage_state = have_row ? 0 : 2;   // wave 0: 0 = the row's flag is not up yet, 1 = its tiles are on their way, 2 = staged (or no row)
            double stg[2][NB * NB / 64];
            CH_STAMP()
            if (tid == 0) { CH_RT(4 * k + 3) }
            // Wave 0's second half: one look at the row's flag per iteration; once it is up, both tiles are requested — and written to
            // LDS in the NEXT iteration (the last one writes at once): requested and written in one iteration, the round trip made that
            // iteration ~450 cycles longer than the working waves' and they waited at its barrier.  (The registers cross the
            // iteration's barrier in wave 0's own loop now; in the round-3 loop, whose body all four waves shared, loads in flight
            // over the back edge made the compiler open EVERY wave's iteration with "s_waitcnt vmcnt(0)".)
#ifdef FL_NO_STAGE   // (tools/ldlt ablation build: wave 0 only walks through the barriers of the second half)
#define FL_STAGE_ON false
#else
#define FL_STAGE_ON true
#endif
#define FACTOR_IDLE_HOOK(t_)                                                                                         \
    if (FL_STAGE_ON && stage_state < 2) {                                                                            \
        if (stage_state == 0 && (r < k0 + 2 || (ch_flag(RF + r) >> 1) == seq)) {                                     \
            _Pragma("unroll") for (int u = 0; u < NB * NB / 64; u++) stg[0][u] = ch_ld(S + o_rk + lane + 64 * u);    \
            _Pragma("unroll") for (int u = 0; u < NB * NB / 64; u++) stg[1][u] = ch_ld(S + o_rr + lane + 64 * u);    \
            stage_state = (t_) + 1 < niter ? 1 : 3;                                                                  \
            CH_SEEN(t_)                                                                                              \
        } else if (stage_state == 1)                                                                                 \
            stage_state = 3;                                                                                         \
        if (stage_state == 3) {                                                                                      \
            _Pragma("unroll") for (int u = 0; u < NB * NB / 64; u++) {                                               \
                const int e_ = lane + 64 * u;                                                                        \
                s.T3[(e_ / NB) * LDP + e_ % NB] = stg[0][u];                                                         \
                s.T4[(e_ / NB) * LDP + e_ % NB] = stg[1][u];                                                         \
            }                                                                                                        \
            if (lane == 0) s.staged[0] = s.staged[1] = 1;                                                            \
            stage_state = 2;                                                                                         \
        }                                                                                                            \
    }
#include "ldlt_factor2.inc"
#undef FACTOR_IDLE_HOOK
            CH_STAMP()
            if (k == k0) {
                // may plain stores be used?  Every working workgroup has recorded its XCC id long ago (they start within a
                // microsecond, this is 4 us later); one that has not counts as "elsewhere".  ONE wave looks, all follow.
                if (w == 0) {   // (lane i looks at role i's word: one round trip, not one per role)
                    bool same = true;
                    for (int i = lane; i < n_roles + n_col; i += 64) same = same && ch_flag(i < n_roles ? XCC + i : XCC2 + (i - n_roles)) == ((seq << 4) | my_xcc);
                    const bool all_same = __builtin_amdgcn_ballot_w64(!same) == 0;
                    if (lane == 0) s.one_xcd = all_same;
                }
                __syncthreads();
                one_xcd = s.one_xcd != 0;
            }
            // Lkk^-T: to LDS as the TRSM's operand, to the factor buffer straight from the accumulators; D_k
            const size_t o_kk = se_blk(k, k, band);
#pragma unroll
            for (int v = 0; v < 4; v++)   // (ldlt_factor2.inc: wave 2 leaves quadrant (1,1), wave 3 the zeros of (1,0))
                s.T0[(16 * qi + m4 + 4 * v) * LDP + fl_colI] = accI[v];
            // (the global stores of a step are issued BEHIND the products they do not feed — a store instruction costs the wave ~60
            //  cycles of issue with four waves at it, and the matrix pipe is busy for 512 either way)
            auto store_diag = [&]() {
#pragma unroll
                for (int v = 0; v < 4; v++) ch_st(Lf + o_kk + (16 * qi + m4 + 4 * v) * NB + fl_colI, accI[v], one_xcd);
                if (tid < NB) ch_st(a.Dg + k * NB + tid, s.Dv[tid], one_xcd);
            };
            if (!have_row) {
                store_diag();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    ch_raise(F + k, seq, one_xcd);
                    CH_RT(200)
                }
                break;
            }
            // ---- block row k+1: its last step is mine ----
            double aop[NB / 4];
            v4f64 accN;
            if (!(s.staged[0] && s.staged[1])) {   // (written before the loop's last barrier)
                // the row's flag came too late for the idle wave (or there was no second half): all four waves fetch the two tiles now —
                // COALESCED and through the same LDS buffers (as MFMA operands straight from memory they were 16 cache lines per
                // instruction: ~2 500 cycles here against ~1 000, and a chain that missed the staging by a hair lost more than it
                // could have gained: 57.8 against 47.4 us per launch)
                if (r >= k0 + 2 && lane == 0) ch_wait(RF + r, seq, err, d.spin_limit);   // (row k0+1 has no worker: its tiles are the previous kernel's)
                double t3[NB * NB / TPB], t4[NB * NB / TPB];
#pragma unroll
                for (int u = 0; u < NB * NB / TPB; u++) t3[u] = ch_ld(S + o_rk + tid + u * TPB);
#pragma unroll
                for (int u = 0; u < NB * NB / TPB; u++) t4[u] = ch_ld(S + o_rr + tid + u * TPB);
#pragma unroll
                for (int u = 0; u < NB * NB / TPB; u++) {
                    const int e = tid + u * TPB;
                    s.T3[(e / NB) * LDP + e % NB] = t3[u];
                    s.T4[(e / NB) * LDP + e % NB] = t4[u];
                }
                __syncthreads();
            }
#pragma unroll
            for (int kk = 0; kk < NB / 4; kk++) aop[kk] = s.T3[(16 * qi + i16) * LDP + 4 * kk + m4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int row = 16 * qi + m4 + 4 * v;
                accN[v] = s.T4[max(row, colq) * LDP + min(row, colq)];
            }
            CH_STAMP()
            __syncthreads();   // (T0)
            // X = A(r,k) Lkk^-T (upper triangular: the slabs below the diagonal are zeros and ride along), L = X D^-1
            v4f64 x = {0, 0, 0, 0};
            {
                const double* pb = s.T0 + m4 * LDP + colq;
                double b8[NB / 4];
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) b8[kk] = pb[4 * kk * LDP];
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) x = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[kk], b8[kk], x, 0, 0, 0);
            }
            const double idc = s.iD[colq];
            __builtin_amdgcn_sched_barrier(0);
            store_diag();
            __builtin_amdgcn_sched_barrier(0);
            double lv[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int e = (16 * qi + m4 + 4 * v);
                lv[v] = x[v] * idc;
                s.T1[e * LDP + colq] = x[v];
                s.T2[e * LDP + colq] = lv[v];
            }
            __syncthreads();   // (T1, T2; and everybody has read iD, T0, T3, T4, staged)
            double bt[NB / 4];
#pragma unroll
            for (int kk = 0; kk < NB / 4; kk++) bt[kk] = s.T2[(16 * qj + i16) * LDP + 4 * kk + m4];
            const v4f64 upd = mma_t(s.T1, bt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < 4; v++) ch_st(Lf + o_rk + (16 * qi + m4 + 4 * v) * NB + colq, lv[v], one_xcd);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < 4; v++) accK[v] = accN[v] - upd[v];
            // everything of step k is stored: both flags go up behind ONE wait.  (Raised from inside the next factorisation
            // instead — its second iteration, when the stores have landed for certain — the wait left the chain, but the two
            // extra branches in the loop cost as much: 15.5 against 15.3 thousand cycles per step.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                ch_raise(F + k, seq, one_xcd);
                ch_raise(XF(r, k), seq, one_xcd);
                CH_RT(4 * k)
            }
            if (r == k1) {
                // my last pivot was k1 - 1: block (k1, k1) with every update of my columns goes back to S for whoever eliminates it
                // (lower triangle: the quadrants (0,0), (1,0), (1,1) — wave 1 carries none)
                if (w != 1) {
#pragma unroll
                    for (int v = 0; v < 4; v++) S[o_rr + (16 * qi + m4 + 4 * v) * NB + colq] = accK[v];
                }
                break;
            }
            CH_STAMP()
        }
        return;
    }
    if (role == n_roles - 1) {
        // ================================ the right-hand side ================================
        // b: rows [k0 * NB, kr * NB) of the vector, held RELATIVE to k0 — the buffer is the place of a row worker's tiles,
        // (band + 1) * CH_TS doubles, and only kr - k0 <= CH_MAX_NB block rows are ever needed; indexed by absolute row (rounds 2-3)
        // the middle launch of a two-ended elimination ran past it from b_start > 33 (band + 1) on: ~700 free cameras at band 1
        double* const bb = ch_lds + (sizeof(ChainLds) + 7) / 8;
        const int b0 = k0 * NB;
        for (int i = k0 * NB + tid; i < kr * NB; i += TPB) bb[i - b0] = E[i];
        __syncthreads();
        const int q = tid & (NB - 1), part = tid >> 5;   // z: column q of Lmm^-T, its rows part + 8 j
        const int row = tid >> 3, g = tid & 7;           // updates: row of a tile, its columns g + 8 jj
        for (int m = k0; m < k1; m++) {
            unsigned fv = 0;
            if (lane == 0) fv = ch_wait(F + m, seq, err, d.spin_limit);
            const bool one_xcd = (__builtin_amdgcn_readfirstlane(fv) & 1u) != 0;
            if (tid == 0 && m == k1 - 1) { CH_RT(201) }
            const size_t o_mm = se_blk(m, m, band);
            double t4[NB / 8];
#pragma unroll
            for (int j = 0; j < NB / 8; j++) t4[j] = ch_ld(Lf + o_mm + (part + 8 * j) * NB + q);
            double p = 0;
#pragma unroll
            for (int j = 0; j < NB / 8; j++) p += t4[j] * bb[m * NB - b0 + part + 8 * j];
            s.zp[part][q] = p;
            __syncthreads();
            if (tid < NB) {
                const double z = ((s.zp[0][tid] + s.zp[1][tid]) + (s.zp[2][tid] + s.zp[3][tid])) +
                                 ((s.zp[4][tid] + s.zp[5][tid]) + (s.zp[6][tid] + s.zp[7][tid]));
                s.z[tid] = z;
                if (do_bw != 2) a.y[m * NB + tid] = z;   // (read by the next kernel; the forward-inverse form has none that reads it)
                if (do_bw == 1) bb[m * NB - b0 + tid] = z / ch_ld(a.Dg + m * NB + tid);   // (b_m was consumed above: its place takes w_m = D^-1 z_m)
                if (do_bw == 2) ch_st(d.bw_scratch + m * NB + tid, z / ch_ld(a.Dg + m * NB + tid), one_xcd);   // (w_m for the column workers)
            }
            if (do_bw == 2 && w == 0) {   // (wave 0 stored w_m: its own wait orders the flag behind it)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0) {
                    ch_raise(WF + m, seq, one_xcd);
                    if (m == k1 - 1) { CH_RT(202) }
                }
            }
            __syncthreads();
            double zr[NB / 8];
#pragma unroll
            for (int jj = 0; jj < NB / 8; jj++) zr[jj] = s.z[g + 8 * jj];
            const int jhi = min(kr - 1, m + band);
            {
                const int jw = m + 1 + lane;   // lane u looks at row m+1+u's flag
                ch_wait_lanes(XF(min(jw, jhi), m), jw <= jhi && jhi > m, seq, err, d.spin_limit);
            }
            for (int jb = m + 1; jb <= jhi; jb += 4) {   // four rows at a time: loads, then sums
                const int nj = min(4, jhi - jb + 1);
                double lv[4][NB / 8];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (u < nj) {
                        const double* Lj = Lf + se_blk(jb + u, m, band) + row * NB + g;
#pragma unroll
                        for (int jj = 0; jj < NB / 8; jj++) lv[u][jj] = ch_ld(Lj + 8 * jj);
                    }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (u < nj) {
                        double sum = 0;
#pragma unroll
                        for (int jj = 0; jj < NB / 8; jj++) sum += lv[u][jj] * zr[jj];
                        sum += dpp_row_shr_f64<1>(sum);   // the 8 threads of a row are 8 consecutive lanes of a DPP row
                        sum += dpp_row_shr_f64<2>(sum);
                        sum += dpp_row_shr_f64<4>(sum);
                        if (g == 7) bb[(jb + u) * NB - b0 + row] -= sum;
                    }
            }
            __syncthreads();
        }
        for (int i = k1 * NB + tid; i < kr * NB; i += TPB) E[i] = bb[i - b0];   // (the rows below my columns: their right-hand side as it stands)
        if (!do_bw) return;
        // the trial poses exp(da_j) * se3CfW (src/Bundle.cc:496-501), |da|^2 — as ldlt_backward_kernel leaves them (xs: da in LDS)
        auto finish = [&](const double* xs, int nrow) {
            for (int c2 = tid; c2 < d.C; c2 += TPB) {
                const int f = d.cam_free[c2];
                const double* T = d.pose[cur] + 12 * c2;
                double* Tn = d.pose[cur ^ 1] + 12 * c2;
                double Tl[12], o[12];
#pragma unroll
                for (int i = 0; i < 12; i++) Tl[i] = T[i];
                if (f < 0) {
#pragma unroll
                    for (int i = 0; i < 12; i++) Tn[i] = Tl[i];
                } else {
                    double mu[6];
#pragma unroll
                    for (int i = 0; i < 6; i++) mu[i] = xs[6 * f + i];
                    se3_exp_mul(mu, Tl, o);
#pragma unroll
                    for (int i = 0; i < 12; i++) Tn[i] = o[i];
                }
            }
#ifdef K7_TIMING
            if (tid == 0) d.dbg[1398] = (long long)__builtin_readcyclecounter();
#endif
            if (tid < 64) {
                double sq = 0;
                for (int i = tid; i < min(nrow, d.n); i += 64) sq += xs[i] * xs[i];
                sq = wave_sum_f64(sq);
                if (tid == 0) {
                    d.sumsq2[0] = sq;
                    d.sumsq2[1] = 0.0;
                    // a wait of THIS solve gave up somewhere (every wait that could still give up has been passed by now): the solve is
                    // void, the host repeats the trial with the launch-per-block-column form; the word is taken down again
                    if (ch_flag(err) != 0) {
                        d.sc->solve_fault = 1;
                        __hip_atomic_store(err, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        };
        if (do_bw == 2) {
            // ================================ ... forward-inverse form: the column workers have x ================================
            // one look at all their flags per round trip, then da comes back through the L2 they stored to
            const int nrow = kr * NB;
            double* const xs = bb + nrow;
            ch_wait_lanes(XD + min(lane, kr - 1), lane < kr, seq, err, d.spin_limit);
            if (tid == 0) { CH_RT(207) }
            for (int i = tid; i < nrow; i += TPB) xs[i] = ch_ld(d.da + i);
            __syncthreads();
            finish(xs, nrow);
            if (tid == 0) { CH_RT(208) }
            return;
        }
        // ================================ ... and backwards ================================
        // L^T x = w, block by block from the last, right-looking (solve.hip: ldlt_backward_kernel is the stand-alone form): per
        // block k  x_k = Lkk^-T (w_k - pending_k), then pending_m += L(k, m)^T x_k for the in-band blocks m < k.  Everything this
        // needs is final (every flag of the launch has been seen) and in this XCD's L2.  Two things bound the pass: this ONE
        // compute unit's path to the L2 — tools/membw/l2cu: four waves pull 19 bytes per cycle with 8-byte loads, 34 with 16-byte
        // ones, and a wave is held at every load it issues; the factor is 360 KB at 50 keyframes — and the chain  pending sums
        // -> mat-vec -> products  of a block.  With all four waves doing both in turn (first form: 1.9 k cycles per block) the
        // two added up, and the pass cost what the separate kernel and its launch cost.  So the waves take ROLES:
        //   wave 0, the chain: v = w_k - pending_k, x_k = Lkk^-T v (lane (r, h): row r, columns 16 h ..: 16 products, the halves
        //     met through LDS); it issues no global load at all;
        //   waves 1..3, the tiles: wave t takes tiles t-1, t+2, t+5 of a block row, a WHOLE tile per wave, eight 16-byte loads per
        //     lane (lane (g, p): rows g, g + 4, ... of the column pair p), requested at the top of the block — in flight under
        //     wave 0's chain —, multiplied when x_k is there and added into ITS slice of the pending sums (one per wave and lane
        //     group: twelve slices, one writer per slot, block rows in descending order, summed in fixed order by wave 0 — the same
        //     bits on every rank); the last of them also brings the NEXT block's Lkk^-T into LDS (coalesced; as "row r,
        //     columns 16 h .." straight from memory a request touched 64 cache lines).
        // Two barriers per block: x_k there | pending sums complete.  The 16-byte loads are `global_load_dwordx4 ... sc1` (ch_ld2_issue):
        // like ch_ld they bypass this compute unit's L1 — which may still hold the previous solve's factor — and are served by the
        // L2 the writers stored to (or, when the launch was spread over several XCDs and the writers wrote through, by memory); no
        // fence is needed or issued.  (Plain loads behind an L1 invalidate were 3x slower on lines another CU had just written.)
        {
            const int nrow = kr * NB;
            double* const xs = bb + nrow;
            double* const pend = xs + nrow;   // [CH_BW_SL][nrow]
            for (int i = tid; i < CH_BW_SL * nrow; i += TPB) pend[i] = 0.0;
            const int hh = lane >> 5, c32 = lane & (NB - 1);   // wave 0: row c32, column half hh
            const int g4 = lane >> 4, cp = lane & 15;           // tile waves: rows g4 + 4 u, columns 2 cp, 2 cp + 1
            constexpr int TW = 3;   // tiles per tile wave and block row
            static_assert(3 * TW >= CH_BW_MAXT, "three tile waves cover a block row");
            static_assert(CH_BW_SL == 12, "a slice per tile wave and lane group");
            const int tw = w - 1;
            double* const dstage0 = s.T1;   // (T1 .. T4: 4 224 doubles, the forward pass is done with them): two staging areas, pitch 34
            static_assert(4 * NB * LDP >= 2 * NB * 34, "the diagonal tiles' staging areas");
            // (the three tile waves share it — requests u = tw, tw + 3, tw + 6 of its eight: all on one wave, beside that wave's
            //  three tiles, the compiler ran out of registers and fetched the tile one request after the other: 4 400 cycles per block)
            auto stage_diag = [&](int k) {   // (tile waves) Lkk^-T -> LDS
                const double2* dk = (const double2*)(Lf + se_blk(k, k, band)) + lane;
                double2 dq[3];
#pragma unroll
                for (int i = 0; i < 3; i++)
                    if (tw + 3 * i < NB / 4) ch_ld2_issue(dq[i], dk + 64 * (tw + 3 * i));
                ch_ld2_wait();   // (and with it every tile request of this wave: they were issued before)
                double* const ds = dstage0 + (k & 1) * (NB * 34);
#pragma unroll
                for (int i = 0; i < 3; i++)
                    if (tw + 3 * i < NB / 4) *(double2*)(ds + (4 * (tw + 3 * i) + g4) * 34 + 2 * cp) = dq[i];
            };
            if (w > 0) stage_diag(kr - 1);
            __syncthreads();   // (the zeros are written, the first diagonal tile is staged)
#ifdef K7_TIMING
#define BWI_STAMP(i_) if (lane == 0 && w < 2) d.dbg[1400 + 8 * k + 4 * w + (i_)] = (long long)__builtin_readcyclecounter();
            if (tid == 0) d.dbg[1399] = (long long)__builtin_readcyclecounter();
#else
#define BWI_STAMP(i_)
#endif
#pragma unroll 1
            for (int k = kr - 1; k >= 0; k--) {
                const int jb0 = max(0, k - band), nt = k - jb0;
                BWI_STAMP(0)
                double2 lt[TW][NB / 4];
                if (w == 0) {
                    // ---- the chain ----
                    const double* pk = pend + k * NB + c32;
                    const double v = bb[k * NB + c32] - ((((pk[0] + pk[nrow]) + (pk[2 * nrow] + pk[3 * nrow])) + ((pk[4 * nrow] + pk[5 * nrow]) + (pk[6 * nrow] + pk[7 * nrow]))) +
                                                         ((pk[8 * nrow] + pk[9 * nrow]) + (pk[10 * nrow] + pk[11 * nrow])));
                    if (hh == 0) s.z[c32] = v;
                    // (LDS operations of one wave are executed in order: the wave reads what it wrote without a barrier; the fence keeps
                    //  the compiler from moving the reads up)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    // (every operand fetched unconditionally, THEN the triangle's selects: with the loads inside the conditionals the
                    //  compiler made sixteen exec-masked LDS round trips of them — 2 000 cycles per block)
                    double tk[NB / 2], zk[NB / 2];
#pragma unroll
                    for (int u = 0; u < NB / 2; u++) tk[u] = dstage0[(k & 1) * (NB * 34) + c32 * 34 + 16 * hh + u], zk[u] = s.z[16 * hh + u];
                    double p4[4] = {0, 0, 0, 0};   // (four partial sums: sixteen dependent additions were 250 cycles of the chain)
#pragma unroll
                    for (int u = 0; u < NB / 2; u++) p4[u & 3] += (16 * hh + u >= c32) ? tk[u] * zk[u] : 0.0;   // upper triangular
                    const double p = (p4[0] + p4[1]) + (p4[2] + p4[3]);
                    // the two column halves of a row sit in lanes r and r + 32: v_permlane32_swap hands the upper half's sums down
                    // (through LDS it was one more round trip on the chain)
                    const unsigned long long pb_ = (unsigned long long)__double_as_longlong(p);
                    const auto lo_ = __builtin_amdgcn_permlane32_swap((unsigned)pb_, (unsigned)pb_, false, false);
                    const auto hi_ = __builtin_amdgcn_permlane32_swap((unsigned)(pb_ >> 32), (unsigned)(pb_ >> 32), false, false);
                    const double p_up = __longlong_as_double((long long)(((unsigned long long)hi_[1] << 32) | lo_[1]));   // lanes 0..31: the sum of lane + 32
                    if (hh == 0) xs[k * NB + c32] = p + p_up;
                    BWI_STAMP(1)
                } else {
                    // ---- the tiles: block row k requested now, under wave 0's chain ----
                    const double2* src = (const double2*)(Lf + se_blk(k, jb0, band)) + lane;
#pragma unroll
                    for (int i = 0; i < TW; i++)
                        if (tw + 3 * i < nt) {
#pragma unroll
                            for (int u = 0; u < NB / 4; u++) ch_ld2_issue(lt[i][u], src + (size_t)(tw + 3 * i) * (NB * NB / 2) + 64 * u);
                        }
                    if (k > 0)
                        stage_diag(k - 1);
                    else
                        ch_ld2_wait();
                }
                BWI_STAMP(2)
                __syncthreads();   // x_k is there
                BWI_STAMP(3)
                if (w > 0) {
                    double xv[NB / 4];
#pragma unroll
                    for (int u = 0; u < NB / 4; u++) xv[u] = xs[k * NB + 4 * u + g4];
                    double* const pslot = pend + (4 * tw + g4) * nrow + jb0 * NB + 2 * cp;
#pragma unroll
                    for (int i = 0; i < TW; i++)
                        if (tw + 3 * i < nt) {
                            double a0 = 0, a1 = 0;
#pragma unroll
                            for (int u = 0; u < NB / 4; u++) a0 += lt[i][u].x * xv[u], a1 += lt[i][u].y * xv[u];
                            // (the only writer of its slots; as LDS adds without return: a read-modify-write in registers is a round trip per tile)
                            __hip_atomic_fetch_add(pslot + (tw + 3 * i) * NB, a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_add(pslot + (tw + 3 * i) * NB + 1, a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                }
                __syncthreads();   // the pending sums of block k - 1 are complete
            }
            __syncthreads();
            for (int i = tid; i < nrow; i += TPB) d.da[i] = xs[i];
            finish(xs, nrow);
        }
        return;
    }
    if (role >= n_roles) {
        // ================================ column worker (forward-inverse form) ================================
        const int j = role - n_roles;   // my block column: the 32 columns of L^-1 below and including block j
        double* const Rt = ch_lds + (sizeof(ChainLds) + 7) / 8;   // R(jb), jb = j .. kr-1: tile jb - j
        for (int e = tid; e < (kr - j) * CH_TS; e += TPB) Rt[e] = 0.0;
        __syncthreads();
        if (tid < NB) Rt[tid * LDP + tid] = 1.0;
        __syncthreads();
        const int c32 = tid & (NB - 1), part = tid >> 5;   // x_j: column c32 of Y(m,j), its rows part + 8 jj
        double xp = 0;
        bool one_xcd = false;
        for (int m = j; m < kr; m++) {
            unsigned fv = 0;
            if (lane == 0) fv = ch_wait(F + m, seq, err, d.spin_limit);
            one_xcd = (__builtin_amdgcn_readfirstlane(fv) & 1u) != 0;
            if (tid == 0 && j == 0 && m == kr - 1) { CH_RT(203) }
            // Y(m,j) = Lmm^-1 R(m): the stored Lmm^-T transposed as the A operand, straight from memory (16 doubles of 4 rows per request)
            {
                const double* Tm = Lf + se_blk(m, m, band) + m4 * NB + 16 * qi + i16;
                const double* Rm = Rt + (m - j) * CH_TS + m4 * LDP + colq;
                double a8[NB / 4], b8[NB / 4];
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) a8[kk] = ch_ld(Tm + 4 * kk * NB);
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) b8[kk] = Rm[4 * kk * LDP];
                v4f64 y = {0, 0, 0, 0};
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) y = __builtin_amdgcn_mfma_f64_16x16x4f64(a8[kk], b8[kk], y, 0, 0, 0);
#pragma unroll
                for (int v = 0; v < 4; v++) s.T2[(16 * qi + m4 + 4 * v) * LDP + colq] = y[v];
            }
            __syncthreads();   // (Y(m,j) is in T2)
            if (tid == 0 && j == 0 && m == kr - 1) { CH_RT(204) }
            // R(jb) -= L(jb,m) Y(m,j) for the in-band rows below: all their flags in one look per round trip, the tiles COALESCED and
            // through LDS, three per round, the next round's loads in flight under this round's products (as a row worker does)
            const int jhi = min(kr - 1, m + band);
            if (jhi > m) {
                {
                    const int jw = m + 1 + lane;   // lane u looks at row m+1+u's flag
                    ch_wait_lanes(XF(min(jw, jhi), m), jw <= jhi, seq, err, d.spin_limit);
                }
                double bt[NB / 4];   // B operand: Bt[c][k] = Y[k][c]
#pragma unroll
                for (int kk = 0; kk < NB / 4; kk++) bt[kk] = s.T2[(4 * kk + m4) * LDP + colq];
                constexpr int RT = 3;
                double* const stage[RT] = {s.T0, s.T3, s.T4};
                auto issue = [&](int jb, double (&pr)[RT][NB * NB / TPB]) {
#pragma unroll
                    for (int u = 0; u < RT; u++)
                        if (jb + u <= jhi) {
                            const double* src = Lf + se_blk(jb + u, m, band) + tid;
#pragma unroll
                            for (int i = 0; i < NB * NB / TPB; i++) pr[u][i] = ch_ld(src + TPB * i);
                        }
                };
                auto round = [&](int jb, const double (&now)[RT][NB * NB / TPB], double (&nxt)[RT][NB * NB / TPB]) {
                    if (jb + RT <= jhi) issue(jb + RT, nxt);
#pragma unroll
                    for (int u = 0; u < RT; u++)
                        if (jb + u <= jhi) {
#pragma unroll
                            for (int i = 0; i < NB * NB / TPB; i++) {
                                const int e = tid + TPB * i;
                                stage[u][(e / NB) * LDP + e % NB] = now[u][i];
                            }
                        }
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < RT; u++)
                        if (jb + u <= jhi) {
                            const v4f64 upd = mma_t(stage[u], bt);
                            double* rj = Rt + (jb + u - j) * CH_TS + (16 * qi + m4) * LDP + colq;
#pragma unroll
                            for (int v = 0; v < 4; v++) rj[4 * v * LDP] -= upd[v];
                        }
                    __syncthreads();   // (the stage is rewritten by the next round; R(m+1) is complete for the next step)
                };
                double pa[RT][NB * NB / TPB], pb[RT][NB * NB / TPB];   // (ping-pong)
                issue(m + 1, pa);
                for (int jb = m + 1; jb <= jhi; jb += 2 * RT) {
                    round(jb, pa, pb);
                    if (jb + RT <= jhi) round(jb + RT, pb, pa);
                }
            }
            // x_j += Y(m,j)^T w_m
            if (lane == 0) (void)ch_wait(WF + m, seq, err, d.spin_limit);
            if (tid == 0 && j == 0 && m == kr - 1) { CH_RT(205) }
            double wv[NB / 8];
#pragma unroll
            for (int jj = 0; jj < NB / 8; jj++) wv[jj] = ch_ld(d.bw_scratch + m * NB + part + 8 * jj);
#pragma unroll
            for (int jj = 0; jj < NB / 8; jj++) xp += s.T2[(part + 8 * jj) * LDP + c32] * wv[jj];
            __syncthreads();   // (T2 is rewritten by the next step)
        }
        s.zp[part][c32] = xp;
        __syncthreads();
        if (w == 0) {
            if (tid < NB)
                ch_st(d.da + j * NB + tid,
                      ((s.zp[0][tid] + s.zp[1][tid]) + (s.zp[2][tid] + s.zp[3][tid])) + ((s.zp[4][tid] + s.zp[5][tid]) + (s.zp[6][tid] + s.zp[7][tid])), one_xcd);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (wave 0 stored x_j: its own wait orders the flag behind it)
            if (lane == 0) {
                ch_raise(XD + j, seq, one_xcd);
                if (j == 0) { CH_RT(206) }
            }
        }
        return;
    }
    // ================================ row worker ================================
    const int r = k0 + role + 1;
    if (r >= kr) return;
    const int j0 = max(k0, r - band), nt = r - j0 + 1;
    double* const tiles = ch_lds + (sizeof(ChainLds) + 7) / 8;
    for (int t = 0; t < nt; t++) {
        const size_t o = se_blk(r, j0 + t, band);
        double v4[NB * NB / TPB];
#pragma unroll
        for (int u = 0; u < NB * NB / TPB; u++) v4[u] = S[o + tid + u * TPB];
#pragma unroll
        for (int u = 0; u < NB * NB / TPB; u++) {
            const int e = tid + u * TPB;
            tiles[t * CH_TS + (e / NB) * LDP + e % NB] = v4[u];
        }
    }
    __syncthreads();
    bool one_xcd = false, stored_direct = false;
    const int m_last = min(r - 2, k1 - 1);   // (a row below k1: every pivot of the launch that reaches it)
    for (int m = j0; m <= m_last; m++) {
        // F[m]: Lmm^-T, D_m and L(m+1, m) are stored
        unsigned fv = 0;
        if (lane == 0) fv = ch_wait(F + m, seq, err, d.spin_limit);
        one_xcd = (__builtin_amdgcn_readfirstlane(fv) & 1u) != 0;
        if (tid == 0 && m == r - 2) { CH_RT(4 * m + 1) }
        if (tid == 0 && r == k1 - 1) { CH_RT(100 + 4 * m) }
        const size_t o_mm = se_blk(m, m, band), o_rm = se_blk(r, m, band);
        // every operand that only depends on F[m] requested at once: Lmm^-T, D_m, and the chain's L(m+1, m)
        // (L(m+1, m) COALESCED and through LDS like the other rows' tiles: as a B operand straight from memory — 4 doubles of 16 rows
        //  per instruction, 16 cache lines — it was 512 line requests per workgroup, ~0.7 us of the 1.4 this phase took)
        double lm[NB / 4], ln[NB * NB / TPB];
#pragma unroll
        for (int kk = 0; kk < NB / 4; kk++) lm[kk] = ch_ld(Lf + o_mm + (4 * kk + m4) * NB + colq);
        const double dgc = ch_ld(a.Dg + m * NB + colq);
        {
            const double* Lj = Lf + se_blk(m + 1, m, band) + tid;
#pragma unroll
            for (int i = 0; i < NB * NB / TPB; i++) ln[i] = ch_ld(Lj + TPB * i);
        }
        // X(r,m) = A(r,m) Lmm^-T, L = X D^-1
        const double* tA = tiles + (m - j0) * CH_TS + (16 * qi + i16) * LDP + m4;
        double a8[NB / 4];
#pragma unroll
        for (int kk = 0; kk < NB / 4; kk++) a8[kk] = tA[4 * kk];
        v4f64 x = {0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < NB / 4; kk++) x = __builtin_amdgcn_mfma_f64_16x16x4f64(a8[kk], lm[kk], x, 0, 0, 0);
        const double idc = fast_rcp(dgc);   // (the chain's own D^-1, bit for bit: same function of the same D)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int e = (16 * qi + m4 + 4 * v);
            const double l = x[v] * idc;
            ch_st(Lf + o_rm + e * NB + colq, l, one_xcd);
            s.T1[e * LDP + colq] = x[v];
            s.T2[e * LDP + colq] = l;
        }
#pragma unroll
        for (int i = 0; i < NB * NB / TPB; i++) {
            const int e = tid + TPB * i;
            s.T3[(e / NB) * LDP + e % NB] = ln[i];
        }
        // (the row's LAST pivot — the step the chain waits for: its stores are waited for together with the tiles that go back to
        //  S, below, and XF goes up with RF: one drain of the store queue instead of two on the chain's supply path)
        const bool last_pivot = m == m_last;
        if (!last_pivot) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0 && !last_pivot) ch_raise(XF(r, m), seq, one_xcd);
        if (tid == 0 && r == k1 - 1) { CH_RT(100 + 4 * m + 1) }
        // my row's tiles right of column m: (r, m+1) with the chain's L(m+1, m) — here already —, (r, r) with my own L,
        // the others with the rows above's: their flags first (all of them), then their tiles (all in flight), then the products
        // (to_S: the row's last pivot — the two tiles the chain is waiting for go to S straight from the registers, the first one's
        //  stores drain under the second one's product; through the LDS copy after the loop they were another round trip later)
        const bool to_S = last_pivot && m == r - 2;
        auto update = [&](int j, const double (&bt)[NB / 4]) {
            const v4f64 upd = mma_t(s.T1, bt);
            double* tj = tiles + (j - j0) * CH_TS + (16 * qi + m4) * LDP + colq;
            double* gj = S + se_blk(r, j, band) + (16 * qi + m4) * NB + colq;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const double nv = tj[4 * v * LDP] - upd[v];
                tj[4 * v * LDP] = nv;
                if (to_S) ch_st(gj + 4 * v * NB, nv, one_xcd);
            }
        };
        stored_direct = to_S;
        {
            double bt1[NB / 4];
#pragma unroll
            for (int kk = 0; kk < NB / 4; kk++) bt1[kk] = s.T3[(16 * qj + i16) * LDP + 4 * kk + m4];
            update(m + 1, bt1);
        }
        {
            double btr[NB / 4];
#pragma unroll
            for (int kk = 0; kk < NB / 4; kk++) btr[kk] = s.T2[(16 * qj + i16) * LDP + 4 * kk + m4];
            update(r, btr);
        }
        if (tid == 0 && r == k1 - 1) { CH_RT(100 + 4 * m + 2) }
        {
            const int jw = m + 2 + lane;   // lane u looks at row m+2+u's flag
            ch_wait_lanes(XF(min(jw, nblk - 1), m), jw < r, seq, err, d.spin_limit);
        }
        // The rows above's tiles L(j,m), three per round: fetched COALESCED (thread t takes elements t, t+256, ...: 32 cache lines
        // per tile and workgroup; as B operands straight from memory — 4 doubles of 16 rows per instruction — every tile cost
        // 512 requests and ~2 500 cycles, the last rows' workers fell 5 us behind the chain), laid out in LDS (the chain's
        // buffers T0 / T3 / T4, unused by a worker), and the NEXT round's loads are in flight while this round is multiplied.
        {
            constexpr int RT = 3;
            double* const stage[RT] = {s.T0, s.T3, s.T4};
            auto issue = [&](int jb, double (&pr)[RT][NB * NB / TPB]) {
#pragma unroll
                for (int u = 0; u < RT; u++)
                    if (jb + u < r) {
                        const double* src = Lf + se_blk(jb + u, m, band) + tid;
#pragma unroll
                        for (int i = 0; i < NB * NB / TPB; i++) pr[u][i] = ch_ld(src + TPB * i);
                    }
            };
            auto round = [&](int jb, const double (&cur)[RT][NB * NB / TPB], double (&nxt)[RT][NB * NB / TPB]) {
                if (jb + RT < r) issue(jb + RT, nxt);
#pragma unroll
                for (int u = 0; u < RT; u++)
                    if (jb + u < r) {
#pragma unroll
                        for (int i = 0; i < NB * NB / TPB; i++) {
                            const int e = tid + TPB * i;
                            stage[u][(e / NB) * LDP + e % NB] = cur[u][i];
                        }
                    }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < RT; u++)
                    if (jb + u < r) {
                        double bt[NB / 4];
#pragma unroll
                        for (int kk = 0; kk < NB / 4; kk++) bt[kk] = stage[u][(16 * qj + i16) * LDP + 4 * kk + m4];
                        update(jb + u, bt);
                    }
                __syncthreads();   // (the stage is rewritten by the next round)
            };
            double pa[RT][NB * NB / TPB], pb[RT][NB * NB / TPB];   // (ping-pong)
            if (m + 2 < r) {
                issue(m + 2, pa);
                __syncthreads();   // (T3 held L(m+1, m): every wave has taken its operand before a round stages a tile there)
            }
            for (int jb = m + 2; jb < r; jb += 2 * RT) {
                round(jb, pa, pb);
                if (jb + RT < r) round(jb + RT, pb, pa);
            }
        }
        __syncthreads();
        if (tid == 0 && r == k1 - 1) { CH_RT(100 + 4 * m + 3) }
    }
    // what is left of the row goes back to S, in place: the tiles right of my last pivot — (r, r-1) and (r, r) for the chain, which
    // does the row's last step (flag RF[r]); for a row below k1 + 1 every tile from column k1 on, for the launch that comes next
    {
        const int jf = max(j0, min(r - 1, k1));
        if (m_last < j0) one_xcd = false;   // (no step of this row was mine: the mode has not reached me through a flag — write-through is always right)
        for (int j = jf; j <= r && !stored_direct; j++) {
            const size_t o = se_blk(r, j, band);
            const double* tj = tiles + (j - j0) * CH_TS;
#pragma unroll
            for (int e = tid; e < NB * NB; e += TPB) ch_st(S + o + e, tj[(e / NB) * LDP + e % NB], one_xcd);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            if (m_last >= j0) ch_raise(XF(r, m_last), seq, one_xcd);
            ch_raise(RF + r, seq, one_xcd);
            CH_RT(4 * (r - 2) + 2)
        }
    }
}

// ---- the bottom end of a banded system for the second chain of a two-ended elimination ----
// Eliminating block columns nblk-1, nblk-2, ... upwards is eliminating 0, 1, ... downwards in MIRRORED coordinates: block b' =
// nblk-1-b, row r' = 31-r inside a block, i.e. the matrix J S J.  ldlt_mirror_in_kernel lays the block rows 0' .. kr'-1 of
// J S J (and of J E) out in buffers of their own, in the same banded tile layout, so that the second chain is the SAME code on
// other pointers; ldlt_mirror_out_kernel puts its results where the per-launch form (ldlt_step_body.inc, mirrored branch) puts
// them and the backward substitution expects them: Lkk^-T, D, z in the chain's order at the block's natural place, the
// multiplier block of rows i' for pivot k' as d.L(k, i)[q'][31 - r'], and the updated tiles / right-hand side of the rows
// beyond the chain's columns back into S / E.  One workgroup per (block row b', slot of its band).
__global__ void __launch_bounds__(TPB) ldlt_mirror_in_kernel(BaDev d, int kr) {
    const int band = se_band(d), nblk = d.npad / NB;
    const int bi = blockIdx.x / (band + 1), jo = blockIdx.x % (band + 1), bj = bi - band + jo;   // logical tile (bi', bj')
    if (bi >= kr || bj < 0) return;
    const double* __restrict__ src = d.SE + se_blk(nblk - 1 - bj, nblk - 1 - bi, band);
    double* __restrict__ dst = d.SE2 + se_blk(bi, bj, band);
    // (every load of the thread first, then its stores: as one loop — whose stores may alias the next load as far as the compiler
    //  knew — the tile was four dependent round trips)
    double v[NB * NB / TPB];
#pragma unroll
    for (int i = 0; i < NB * NB / TPB; i++) v[i] = src[threadIdx.x + TPB * i];
#pragma unroll
    for (int i = 0; i < NB * NB / TPB; i++) {
        const int e = threadIdx.x + TPB * i;
        const int a = e / NB, b = e % NB;   // physical element [a][b] = logical [31 - b][31 - a]
        dst[(NB - 1 - b) * NB + (NB - 1 - a)] = v[i];
    }
    if (bi == bj && threadIdx.x < NB)
        d.SE2[se_size(nblk, band) + bi * NB + threadIdx.x] = se_E(d)[(nblk - 1 - bi) * NB + NB - 1 - threadIdx.x];
}
__global__ void __launch_bounds__(TPB) ldlt_mirror_out_kernel(BaDev d, int k1, int kr) {
    const int band = se_band(d), nblk = d.npad / NB;
    const int bi = blockIdx.x / (band + 1), jo = blockIdx.x % (band + 1), bj = bi - band + jo;   // logical tile (bi', bj')
    if (bi >= kr || bj < 0) return;
    const int pi = nblk - 1 - bi, pj = nblk - 1 - bj;   // natural block indices: pj >= pi
    const int tid = threadIdx.x;
    if (bj < k1) {
        // a tile of the factor
        const double* __restrict__ src = d.L2 + se_blk(bi, bj, band);
        double v[NB * NB / TPB];   // (loads first, then stores: see ldlt_mirror_in_kernel)
#pragma unroll
        for (int i = 0; i < NB * NB / TPB; i++) v[i] = src[tid + TPB * i];
        if (bi == bj) {
            double* __restrict__ dst = d.L + se_blk(pi, pi, band);
#pragma unroll
            for (int i = 0; i < NB * NB / TPB; i++) dst[tid + TPB * i] = v[i];
            if (tid < NB) {
                d.Dg[pi * NB + tid] = d.Dg2[bi * NB + tid];
                d.y[pi * NB + tid] = d.y2[bi * NB + tid];
            }
        } else {
            double* __restrict__ dst = d.L + se_blk(pj, pi, band);   // the stored block (k, i) of pivot k = pj and row block i = pi
#pragma unroll
            for (int i = 0; i < NB * NB / TPB; i++) {
                const int e = tid + TPB * i;
                const int r = e / NB, q = e % NB;   // logical L(i', k')[r'][q']
                dst[q * NB + (NB - 1 - r)] = v[i];
            }
        }
    } else {
        // a tile below the chain's columns, with their updates: back to S
        const double* __restrict__ src = d.SE2 + se_blk(bi, bj, band);
        double* __restrict__ dst = d.SE + se_blk(pj, pi, band);
        double v[NB * NB / TPB];
#pragma unroll
        for (int i = 0; i < NB * NB / TPB; i++) v[i] = src[tid + TPB * i];
#pragma unroll
        for (int i = 0; i < NB * NB / TPB; i++) {
            const int e = tid + TPB * i;
            const int r = e / NB, c = e % NB;
            dst[(NB - 1 - c) * NB + (NB - 1 - r)] = v[i];
        }
        if (bi == bj && tid < NB) se_E(d)[pi * NB + NB - 1 - tid] = d.SE2[se_size(nblk, band) + bi * NB + tid];
    }
}
