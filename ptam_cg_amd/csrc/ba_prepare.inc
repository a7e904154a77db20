// ba_prepare.inc — the bundle's index structures built ON THE DEVICE (Bundle::Compute's GenerateMeasLUTs + GenerateOffDiagScripts,
// src/Bundle.cc:116-123, :558-599, run inside every Compute() of a freshly constructed Bundle, src/MapMaker.cc:840).
//
// The host uploads the measurements as they were added (insertion order) and keeps two O(points) / O(tile pairs) jobs: the greedy
// cut of the point list into chunks and the order of the tile pairs.  Everything that walks measurements or Schur entries is here:
//   phase 1   count per point (atomics) -> scan (points with a live measurement get dense ids, rowptr) -> scatter into the points'
//             buckets -> rank inside the bucket by (free cameras by free index, then fixed cameras): the point-major sorted arrays,
//             duplicates detected -> per point: the Schur tiles it touches (records, 2-bit codes, entry count, model cost) ->
//             scan: entry / cost prefix, the 8 XCD point ranges of equal cost -> per (XCD, tile pair): entries per fragment pattern
//   readback  a few scalars + rowptr + the dense point ids (sizes of the work lists: the host carves their memory)
//   phase 2   per XCD: bucket offsets, run lists, the budget search (256 budgets per round, one lane each) and the final greedy
//             cut (ba_split.h) -> per (XCD, tile pair): the entries placed in (pattern, point) order -> slots, block order,
//             workgroup heads.
// Every placement is by RANK, never by arrival order: the lists are the same from run to run (deterministic mode relies on it).
#include "ba_split.h"

struct PrepScalars {
    int P;             // points with a live measurement
    int M;             // live measurements
    int band;          // block bandwidth of S
    int tband;         // tile bandwidth: max over points of (last - first touched tile)
    int dup;           // duplicated (point, camera) measurements seen
    int n_xp;          // non-empty (XCD range, tile pair) lists
    int by_products;   // order of the pairs in a list: by fragment products (1) or natural (0)
    int n_schur_wg, n_segs, n_slots;
    int bad;           // a list outgrew its bound (internal error)
    int pad_;
    unsigned long long dup_key;   // the smallest duplicated (point << 32 | camera)
    long long n_entries;
    long long cost_total;
    int bound[12];     // point ranges of the 8 XCD lists (bound[8] = P)
    long long t_cut[8];
    int n_cuts[8], n_wgs[8];
    long long stamp[8][8];   // -DPREP_STAMPS builds: phases of prep_split_kernel per XCD list (100 MHz ticks)
};

struct PrepDev {
    int C, F, P_all, Mall, M;
    int n_tiles, n_pairs, nw;   // nw: 64-bit words of tile codes per point (32 tiles each)
    int cap_pl, cap_cut;        // per XCD: pairs (and 1/16 of the runs) a list may hold, segments it may be cut into
    // raw input (insertion order): chunks of MS_CH measurements, each [cam | point | found | sigma^2] (MeasStore, bundle.hip)
    const char* r_base;
    const uint8_t* r_dead;      // null: no measurement was erased
    const double* pts_raw;
    // temporaries
    int* cnt;                   // [P_all] live measurements per point
    int* start;                 // [P_all + 1]
    int* dense_of;              // [P_all]
    int* pt_orig;               // [P_all] dense id -> original id
    int* arr;                   // [Mall] arrival index inside the point's bucket
    int* tmp_i;                 // [M] bucket slot -> insertion index
    int* tmp_key;               // [M]            -> sort key of its camera
    int4* ptile;                // [M] per point, at rowptr[p] + j: j-th touched tile {tile, first measurement, slot offsets 0-3, 4-7}
    unsigned long long* tcode;  // [P_all][nw] 2 bits per tile: bit 0 a camera in slots 0..5, bit 1 in slots 5..7
    int* kp;                    // [P_all] touched tiles
    int* costp;                 // [P_all] model cost of the point's entries
    long long* ent_pre;         // [P_all + 1] entries of the points before
    long long* cost_pre;        // [P_all + 1]
    int* hist;                  // [8][n_pairs][16]
    int* ebase;                 // [8][n_pairs][16] first entry of the bucket in s_entries
    const int* pair_order;      // [2][n_pairs] natural | by fragment products
    // phase 2 (work-list block)
    int* run_cnt;               // [8][16 cap_pl]
    int* run_cost;
    int* pl_pair;               // [8][cap_pl]
    int* pl_n;
    int* pl_run0;               // [8][cap_pl + 1]
    int* pl_e0;                 // [8][cap_pl] first entry of the pair in this list
    int* pl_e;                  // [8][cap_pl + 1] entries of the list before the pair
    long long* pl_h;            // [8][cap_pl + 1] H at the pair's start (ba_split.h: the even split)
    int* cut_pair;              // [8][cap_cut]
    int* cut_e0;
    int* cut_e1;
    int* cut_wg;
    int* wg_first;              // [8][slots + 1]
    int* cpx;                   // [n_pairs * 8 + 1] segments per (pair, XCD) -> slot bases
    int* pair_first;            // [n_pairs * 8] first cut of the pair in the XCD's list
    int* wseg_tmp;              // [8 slots + 1]
    int4* rec;                  // [8][512][cap_cut] the cut every lane of the budget search makes (null: too many segments to keep)
    PrepScalars* ps;
    // host-mapped read-back area (zero-copy stores): [PrepScalars | rowptr (P_all + 1) | pt_orig (P_all)]
    PrepScalars* h_ps;
    int* h_rowptr;
    int* h_pt_orig;
};

// (the raw measurement chunks, MS_CH / ms_cam ..., are laid out in bundle.h)

__device__ __forceinline__ void prep_pair_ab(int pr, int& a, int& b) {
    a = (int)((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= pr) a++;
    while (a * (a + 1) / 2 > pr) a--;
    b = pr - a * (a + 1) / 2;
}
__device__ __forceinline__ int prep_code(const PrepDev& q, int p, int t) {
    return (int)((q.tcode[(size_t)p * q.nw + (t >> 5)] >> (2 * (t & 31))) & 3ull);
}
__device__ __forceinline__ int prep_code_of(unsigned o0, unsigned o1) {
    const int s01 = (o0 != 0xffffffffu) || ((o1 & 0xffffu) != 0xffffu);   // slots 0..5
    const int s2 = (o1 >> 8) != 0xffffffu;                                 // slots 5..7
    return s01 | (s2 << 1);
}

// exclusive scan of one 64-bit value per thread over a workgroup of NT threads (a multiple of 64): inclusive scan of the wave by
// shuffles, the waves' totals through LDS (lds: NT / 64 words); *total gets the sum.  One barrier pair.
template <int NT>
__device__ __forceinline__ long long prep_block_scan(long long v, long long* lds, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long x = __shfl_up(inc, off);
        if (lane >= off) inc += x;
    }
    __syncthreads();   // (the previous scan's totals have been read)
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const long long x = lds[w];
        base += w < wave ? x : 0;
        tot += x;
    }
    if (total) *total = tot;
    return base + inc - v;
}

// ---- phase 1 -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) prep_count_kernel(PrepDev q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.Mall) return;
    if (q.r_dead && q.r_dead[i]) return;
    q.arr[i] = atomicAdd(&q.cnt[ms_pt(q.r_base, i)], 1);
}

// one workgroup: bucket starts, dense point ids (the points that HAVE a live measurement, in their original order), rowptr.
// Tiles of 4096 points, four consecutive ones per thread (coalesced 16-byte accesses), both counts in one 64-bit scan.
__global__ void __launch_bounds__(1024) prep_scan_points_kernel(PrepDev q, BaDev d) {
    __shared__ long long lds[16];
    const int t = threadIdx.x;
    long long carry = 0;   // (points with a measurement) << 32 | measurements
    auto load4 = [&](int p, int* v) {
        v[0] = v[1] = v[2] = v[3] = 0;
        if (p + 3 < q.P_all) {
            const int4 w = *(const int4*)(q.cnt + p);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        } else
            for (int i = 0; i < 4; i++)
                if (p + i < q.P_all) v[i] = q.cnt[p + i];
    };
    int nxt[4];
    load4(4 * t, nxt);
    for (int base = 0; base < q.P_all; base += 4096) {
        const int p = base + 4 * t;
        int v[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
        if (base + 4096 < q.P_all) load4(p + 4096, nxt);   // (the next tile's counts are on their way while this one is scanned)
        const int c = v[0] + v[1] + v[2] + v[3], nz = (v[0] > 0) + (v[1] > 0) + (v[2] > 0) + (v[3] > 0);
        long long tot;
        const long long ex = prep_block_scan<1024>(((long long)nz << 32) | (long long)c, lds, &tot) + carry;
        int cb = (int)(ex & 0xffffffffll), nb = (int)(ex >> 32);
        int st[4], dn[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            st[i] = cb;
            dn[i] = v[i] > 0 ? nb : -1;
            if (v[i] > 0) {
                q.pt_orig[nb] = p + i;
                d.rowptr[nb] = cb;
                nb++;
            }
            cb += v[i];
        }
        if (p + 3 < q.P_all) {
            *(int4*)(q.start + p) = make_int4(st[0], st[1], st[2], st[3]);
            *(int4*)(q.dense_of + p) = make_int4(dn[0], dn[1], dn[2], dn[3]);
        } else
            for (int i = 0; i < 4; i++)
                if (p + i < q.P_all) q.start[p + i] = st[i], q.dense_of[p + i] = dn[i];
        carry += tot;
    }
    if (t == 0) {
        const int P = (int)(carry >> 32), M = (int)(carry & 0xffffffffll);
        q.start[q.P_all] = M;
        d.rowptr[P] = M;
        q.ps->P = P;
        q.ps->M = M;
    }
}

__global__ void __launch_bounds__(256) prep_scatter_kernel(PrepDev q, const int* __restrict__ cam_free) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.Mall) return;
    if (q.r_dead && q.r_dead[i]) return;
    const int p = ms_pt(q.r_base, i), c = ms_cam(q.r_base, i), f = cam_free[c];
    const int slot = q.start[p] + q.arr[i];
    q.tmp_i[slot] = i;
    q.tmp_key[slot] = f >= 0 ? f : q.F + c;   // the free cameras first, by free index, then the fixed ones
}

// The position of a measurement inside its point's run is its RANK by key (keys are unique inside a point unless a (point, camera)
// pair was measured twice — refused, as the round-1 host path did): the sorted arrays do not depend on the arrival order of
// the atomics above.
// (Side jobs of this wide launch, one stride loop each: the dense points' positions gathered, rowptr and the dense ids copied to the
//  host-mapped area — a single workgroup doing them was most of 0.3 ms at 50 000 points.)
__global__ void __launch_bounds__(256) prep_rank_kernel(PrepDev q, BaDev d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    {
        const int P = q.ps->P, nthr = gridDim.x * 256;
        for (int i = j; i < 3 * P; i += nthr) {
            const int qd = i / 3, k = i - 3 * qd;
            d.pt[0][i] = q.pts_raw[(size_t)3 * q.pt_orig[qd] + k];
        }
        for (int i = j; i <= P; i += nthr) q.h_rowptr[i] = d.rowptr[i];
        for (int i = j; i < P; i += nthr) q.h_pt_orig[i] = q.pt_orig[i];
    }
    if (j >= q.M) return;
    const int i = q.tmp_i[j], k = q.tmp_key[j];
    const int p = ms_pt(q.r_base, i);
    const int s0 = q.start[p], s1 = q.start[p + 1];
    int rank = 0;
    bool dup = false;
    for (int l = s0; l < s1; l++) {
        const int kl = q.tmp_key[l];
        rank += kl < k;
        dup = dup || (kl == k && l != j);
    }
    const int dst = s0 + rank, c = ms_cam(q.r_base, i);
    d.m_cam[dst] = c;
    d.m_pt[dst] = q.dense_of[p];
    d.m_orig[dst] = i;
    d.m_fidx[dst] = k < q.F ? k : -1;
    d.m_found[dst] = ms_found(q.r_base, i);
    d.m_s[dst] = sqrt(1.0 / ms_sig(q.r_base, i));   // dSqrtInvNoise src/Bundle.cc:91
    if (dup) {
        atomicAdd(&q.ps->dup, 1);
        atomicMin(&q.ps->dup_key, ((unsigned long long)(unsigned)p << 32) | (unsigned)c);
    }
}

// Per point: the Schur tiles it touches.  Its free cameras come first and ascending, so a tile's measurements are consecutive:
// record j = {tile, first measurement, per camera slot the offset of that camera's measurement from the first (0xff: none)}.
__global__ void __launch_bounds__(64) prep_tiles_kernel(PrepDev q, BaDev d, int cost_model) {
    const int qd = blockIdx.x * 64 + threadIdx.x;
    const int P = q.ps->P;
    int band = 0, tband = 0;
    if (qd < P) {
        const int i0 = d.rowptr[qd], i1 = d.rowptr[qd + 1];
        int j = 0, last = -1, first_i = 0, lo = -1, hi = -1, widx = -1;
        unsigned o0 = 0xffffffffu, o1 = 0xffffffffu;
        unsigned long long word = 0;
        // (the first eight records also stay in registers for the cost loop below: read back from memory, a point's 28 pairs were
        //  56 dependent loads)
        int rt[8], rcode[8];
        auto flush = [&]() {
            q.ptile[i0 + j - 1] = make_int4(last, first_i, (int)o0, (int)o1);
            const int code = prep_code_of(o0, o1);
#pragma unroll
            for (int u = 0; u < 8; u++)   // (a select per slot: a register array takes no dynamic index)
                if (u == j - 1) rt[u] = last, rcode[u] = code;
            const int wi = last >> 5;
            if (wi != widx) {
                if (widx >= 0) q.tcode[(size_t)qd * q.nw + widx] = word;
                word = 0;
                widx = wi;
            }
            word |= (unsigned long long)code << (2 * (last & 31));
        };
        bool done = false;
        // eight measurements per round trip (requested unconditionally, clamped): one after the other the walk was a chain of
        // ~50 dependent loads per point
        for (int ib = i0; ib < i1 && !done; ib += 8) {
            int fv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) fv[u] = d.m_fidx[min(ib + u, i1 - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = ib + u, f = fv[u];
                if (done || i >= i1) continue;
                if (f < 0) {   // (the fixed cameras' measurements come last)
                    done = true;
                    continue;
                }
                const int t = f >> 3, slot = f & 7;
                if (t != last) {
                    if (last >= 0) flush();
                    j++;
                    last = t;
                    first_i = i;
                    o0 = o1 = 0xffffffffu;
                }
                const unsigned off = (unsigned)(i - first_i), sh = 8 * (slot & 3);
                if (slot < 4)
                    o0 = (o0 & ~(0xffu << sh)) | (off << sh);
                else
                    o1 = (o1 & ~(0xffu << sh)) | (off << sh);
                if (lo < 0) lo = f;
                hi = f;
            }
        }
        if (last >= 0) {
            flush();
            q.tcode[(size_t)qd * q.nw + widx] = word;
        }
        q.kp[qd] = j;
        int cost = 0;
        if (j <= 8) {
#pragma unroll
            for (int ia = 0; ia < 8; ia++)
#pragma unroll
                for (int ib = 0; ib <= ia; ib++)
                    if (ia < j) cost += split_entry_cost(q.F, rt[ia], rt[ib], rcode[ia] | (rcode[ib] << 2), cost_model);
        } else
            for (int ia = 0; ia < j; ia++) {
                const int4 ra = q.ptile[i0 + ia];
                const int ca = prep_code_of((unsigned)ra.z, (unsigned)ra.w);
                for (int ib = 0; ib <= ia; ib++) {
                    const int4 rb = q.ptile[i0 + ib];
                    const int cb = prep_code_of((unsigned)rb.z, (unsigned)rb.w);
                    cost += split_entry_cost(q.F, ra.x, rb.x, ca | (cb << 2), cost_model);
                }
            }
        q.costp[qd] = cost;
        if (hi >= 0) {
            band = (6 * hi + 5) / SOLVE_NB - (6 * lo) / SOLVE_NB;
            tband = (hi >> 3) - (lo >> 3);
        }
    }
    // block bandwidth of the camera system: S_jk != 0 only if cameras j, k share a point
    for (int off = 32; off > 0; off >>= 1) {
        band = max(band, __shfl_xor(band, off));
        tband = max(tband, __shfl_xor(tband, off));
    }
    if (threadIdx.x == 0) {
        if (band > 0) atomicMax(&q.ps->band, band);
        if (tband > 0) atomicMax(&q.ps->tband, tband);
    }
}

// one workgroup: entry / cost prefix over the points (tiles of 1024, coalesced), the XCD point ranges of equal cost, totals
__global__ void __launch_bounds__(1024) prep_scan_cost_kernel(PrepDev q, int min_seg, int slots) {
    __shared__ long long lds[16];
    const int t = threadIdx.x;
    const int P = q.ps->P;
    long long carry_e = 0, carry_c = 0;
    // tiles of 4096 points, four consecutive ones per thread; the next tile's values are requested before this one is scanned
    auto load4 = [&](int p, int* k, int* c) {
        for (int i = 0; i < 4; i++) k[i] = c[i] = 0;
        if (p + 3 < P) {
            const int4 a = *(const int4*)(q.kp + p), b = *(const int4*)(q.costp + p);
            k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w;
            c[0] = b.x, c[1] = b.y, c[2] = b.z, c[3] = b.w;
        } else
            for (int i = 0; i < 4; i++)
                if (p + i < P) k[i] = q.kp[p + i], c[i] = q.costp[p + i];
    };
    int nk[4], nc[4];
    load4(4 * t, nk, nc);
    for (int base = 0; base < P; base += 4096) {
        const int p = base + 4 * t;
        int k[4], cc[4];
        for (int i = 0; i < 4; i++) k[i] = nk[i], cc[i] = nc[i];
        if (base + 4096 < P) load4(p + 4096, nk, nc);
        long long e4[4], e = 0, c = 0;
        for (int i = 0; i < 4; i++) {
            e4[i] = (long long)k[i] * (k[i] + 1) / 2;
            e += e4[i];
            c += cc[i];
        }
        long long te, tc;
        long long eb = prep_block_scan<1024>(e, lds, &te) + carry_e;
        long long cb = prep_block_scan<1024>(c, lds, &tc) + carry_c;
        for (int i = 0; i < 4; i++)
            if (p + i < P) {
                q.ent_pre[p + i] = eb;
                q.cost_pre[p + i] = cb;
                eb += e4[i];
                cb += cc[i];
            }
        carry_e += te;
        carry_c += tc;
    }
    const long long tot_e = carry_e, tot_c = carry_c;
    if (t == 0) {
        q.ent_pre[P] = tot_e;
        q.cost_pre[P] = tot_c;
        q.ps->n_entries = tot_e;
        q.ps->cost_total = tot_c;
        // pairs ordered by their fragment products only where both slots of the CUs are in use (bundle.hip)
        q.ps->by_products = (tot_e / 8 / (4 * min_seg) >= slots) ? 1 : 0;
        q.ps->bound[0] = 0;
        q.ps->bound[8] = P;
    }
    __threadfence_block();
    __syncthreads();
    if (t >= 1 && t < 8) {
        // first point index whose prefix cost reaches t eighths of the total
        const double target = (double)tot_c * t / 8;
        int lo = 0, hi = P + 1;   // lower_bound over cost_pre[0 .. P]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)q.cost_pre[mid] < target)
                lo = mid + 1;
            else
                hi = mid;
        }
        q.ps->bound[t] = min(lo, P);
    }
}

// grid (tile pair, XCD range): how many points of the range touch both tiles, per fragment pattern
__global__ void __launch_bounds__(256) prep_hist_kernel(PrepDev q) {
    const int pr = blockIdx.x, x = blockIdx.y;
    int a, b;
    prep_pair_ab(pr, a, b);
    if (a - b > q.ps->tband) return;   // (the table was cleared)
    __shared__ int h[16];
    if (threadIdx.x < 16) h[threadIdx.x] = 0;
    __syncthreads();
    const int p0 = q.ps->bound[x], p1 = q.ps->bound[x + 1];
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        const int ca = prep_code(q, p, a), cb = a == b ? ca : prep_code(q, p, b);
        if (ca && cb) atomicAdd(&h[ca | (cb << 2)], 1);
    }
    __syncthreads();
    if (threadIdx.x < 16) q.hist[((size_t)x * q.n_pairs + pr) * 16 + threadIdx.x] = h[threadIdx.x];
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < 16; i++) tot += h[i];
        if (tot > 0) atomicAdd(&q.ps->n_xp, 1);
    }
}

// the scalars and the two small tables the host needs go to host-mapped memory; the stamp tells the host they are there
__global__ void prep_publish_kernel(PrepDev q, volatile unsigned long long* stamp, unsigned long long seq) {
    if (threadIdx.x == 0) {
        *q.h_ps = *q.ps;
        __threadfence_system();
        *stamp = seq;
    }
}

// ---- phase 2 -------------------------------------------------------------------------------------------------------------------
// The budget search and the cut of one XCD list (the second half of prep_split_kernel), for lists in LDS or in global memory.
// an XCD list in LDS, with the reciprocals of the runs' costs
typedef const int __attribute__((address_space(3)))* lds_cptr;
typedef const double __attribute__((address_space(3)))* lds_dptr;
typedef const long long __attribute__((address_space(3)))* lds_lptr;
struct SplitRunsLds : SplitRunsT<lds_cptr, lds_lptr> {
    lds_dptr run_inv;
};
__device__ __forceinline__ int split_quot(const SplitRunsLds& R, int i, int n) {   // floor(n / cost), 0 <= n < 2^31
    const int c = R.run_cost[i];
    int q = (int)((double)n * R.run_inv[i]);   // (off by one at most: the product is within 2^-20 of the quotient)
    const int r = n - q * c;
    q += r >= c ? 1 : (r < 0 ? -1 : 0);
    return q;
}

#ifdef PREP_STAMPS
#define PSTAMP(i) { if (threadIdx.x == 0) { q.ps->stamp[x][i] = (long long)__builtin_amdgcn_s_memrealtime(); if (i == 2 || i == 4) q.ps->stamp[x][6 + (i == 4)] = (long long)__builtin_amdgcn_s_memtime(); } }
#else
#define PSTAMP(i) {}
#endif
template <class RUNS>
__device__ __forceinline__ void prep_split_search(const PrepDev& q, const SplitCfg& cfg, const RUNS& R, int x, int np, long long ent_x, long long cost_x,
                                                  const int* g_pl_pair, const int* g_pl_e0, long long* lds, int* s_jmin) {
    const int tid = threadIdx.x;
    // ---- the budget: the smallest T for which the fill needs no more than n_wg workgroups, for two workgroup counts when the
    // XCD's work does not fill both slots of its CUs (one workgroup per CU, or as many as the entries allow).  One lane per
    // budget, 256 budgets per search and round; every lane RECORDS the cut its budget makes (q.rec: 16 bytes per segment), so
    // the winner's cut is there when the search ends — a fill is a serial walk of ~150 steps, and a second one for the final
    // cut was a third of this kernel.
    const int n_wg_max = (int)max(1ll, min((long long)cfg.slots, ent_x / (4 * cfg.min_seg)));
    const int grp = tid >> 8, j = tid & 255;
    const int n_wg = grp == 0 ? n_wg_max : cfg.n_first;
    const bool two = n_wg_max > cfg.n_first;
    SplitBracket br = split_bracket_begin(cost_x, n_wg, np, cfg);
    if (grp == 1 && !two) br.done = 1;
    const bool narrow = br.t_all < (1ll << 30);   // budgets and costs fit 32-bit arithmetic (the device's 64-bit divisions are software)
#ifdef PREP_NOREC
    int4* rec = nullptr;
#else
    int4* rec = q.rec ? q.rec + (size_t)x * 512 * q.cap_cut + tid : nullptr;
#endif   // (segment ci of lane tid at [ci * 512 + tid]: a wave's records side by side)
    int my_cuts = 0, my_wgs = 0, my_over = 0;
    int jwin = SPLIT_NC;
    PSTAMP(2)
    for (int round = 0; round < 64; round++) {
        if (round == 1) PSTAMP(3)
        if (tid < 2) s_jmin[tid] = SPLIT_NC;
        __syncthreads();
        if (!br.done) {
            const long long T = split_candidate(br, j);
            my_cuts = 0, my_over = 0;
            auto keep = [&](int k, int begin, int end, int wg) {
                if (rec) {
                    if (my_cuts < q.cap_cut)
                        rec[(size_t)my_cuts * 512] = make_int4(k, begin, end, wg);
                    else
                        my_over = 1;
                }
                my_cuts++;
            };
            my_wgs = narrow ? split_fill<int>((int)T, R, cfg, keep, n_wg) : split_fill<long long>(T, R, cfg, keep, n_wg);
            if (my_wgs <= n_wg) atomicMin(&s_jmin[grp], j);
        }
        __syncthreads();
        if (!br.done) {
            jwin = s_jmin[grp];
            split_bracket_step(br, jwin);
        }
        // (every thread of a group holds the same bracket; the groups agree on the end through LDS)
        __syncthreads();
        if (j == 0) s_jmin[grp] = br.done;
        __syncthreads();
        const bool all_done = s_jmin[0] && s_jmin[1];
        __syncthreads();
        if (all_done) break;
    }
    PSTAMP(4)
    // the winner: search A's budget, or B's where one workgroup per CU ends earlier
    __shared__ int s_win[4];   // winning thread, its segments, its workgroups, record usable
    if (j == 0) lds[grp] = br.hi, lds[2 + grp] = jwin;
    __syncthreads();
    long long t_cut = lds[0];
    int wgrp = 0;
    if (two && cost_x / cfg.n_first + cfg.seg_cost < t_cut && lds[1] < t_cut) t_cut = lds[1], wgrp = 1;
    const int wj = (int)lds[2 + wgrp];
    if (tid == 0) {
        s_win[0] = -1;
        q.ps->t_cut[x] = t_cut;
    }
    __syncthreads();
    if (grp == wgrp && j == wj && wj < SPLIT_NC && rec && !my_over) {   // (its last fill was the one at t_cut)
        s_win[0] = tid;
        s_win[1] = my_cuts;
        s_win[2] = my_wgs;
    }
    __syncthreads();
    int* c_pair = q.cut_pair + (size_t)x * q.cap_cut;
    int* c_e0 = q.cut_e0 + (size_t)x * q.cap_cut;
    int* c_e1 = q.cut_e1 + (size_t)x * q.cap_cut;
    int* c_wg = q.cut_wg + (size_t)x * q.cap_cut;
    int* wfirst = q.wg_first + (size_t)x * (cfg.slots + 1);
    if (s_win[0] >= 0) {
        // ---- the cut, from the winner's record ----
        const int4* wr = q.rec + (size_t)x * 512 * q.cap_cut + s_win[0];
        const int n_cut = s_win[1], n_wgs = s_win[2];
        __threadfence_block();
        for (int ci = tid; ci < n_cut; ci += 512) {
            const int4 c = wr[(size_t)ci * 512];
            c_pair[ci] = g_pl_pair[c.x];
            c_e0[ci] = g_pl_e0[c.x] + c.y;
            c_e1[ci] = g_pl_e0[c.x] + c.z;
            c_wg[ci] = c.w;
            if (c.w < cfg.slots && (ci == 0 || wr[(size_t)(ci - 1) * 512].w != c.w)) wfirst[c.w] = ci;
        }
        if (tid == 0) {
            if (n_wgs > cfg.slots) atomicOr(&q.ps->bad, 2);
            wfirst[min(n_wgs, cfg.slots)] = n_cut;
            q.ps->n_cuts[x] = n_cut;
            q.ps->n_wgs[x] = min(n_wgs, cfg.slots);
        }
    } else if (tid == 0) {
        // ---- the cut, walked once more (no record: a list of more segments than a lane may keep) ----
        int n_cut = 0, last_wg = -1, over = 0;
        auto put = [&](int k, int begin, int end, int wg) {
            if (n_cut >= q.cap_cut || wg >= cfg.slots) {
                over = 1;
                return;
            }
            c_pair[n_cut] = g_pl_pair[k];
            c_e0[n_cut] = g_pl_e0[k] + begin;
            c_e1[n_cut] = g_pl_e0[k] + end;
            c_wg[n_cut] = wg;
            if (wg != last_wg) {
                wfirst[wg] = n_cut;
                last_wg = wg;
            }
            n_cut++;
        };
        const int n_wgs = split_fill<long long>(t_cut, R, cfg, put);
        if (over || n_wgs > cfg.slots) atomicOr(&q.ps->bad, 4);
        wfirst[min(n_wgs, cfg.slots)] = n_cut;
        q.ps->n_cuts[x] = n_cut;
        q.ps->n_wgs[x] = min(n_wgs, cfg.slots);
    }
    PSTAMP(5)
}

// The even split of one XCD list (ba_split.h): every workgroup's start is a closed form of its index — one lane each —, the segments
// (a workgroup's part of a pair) are placed by RANK among the sorted segment starts = pair starts + the workgroup starts that
// fall inside a pair.  No walk along the list, no search: ~3 us where the greedy fill + budget search took 75 - 215.
template <class RUNS>
__device__ __forceinline__ void prep_split_even(const PrepDev& q, const SplitCfg& cfg, const RUNS& R, int x, int np, long long ent_x,
                                                const int* g_pl_pair, const int* g_pl_e0) {
    const int tid = threadIdx.x;
    __shared__ int s_g[128], s_o[128], s_k[128];
    __shared__ int s_cnt[2];
    const SplitEven ev = split_even_budget(R.pl_h[np], ent_x, cfg);
    const int n_wg = min(ev.n_wg, 128), ent = (int)ent_x;
    if (tid < 2) s_cnt[tid] = 0;
    if (tid < n_wg) {
        int k, o;
        s_g[tid] = split_even_start(tid, ev, R, cfg, &k, &o);
        s_k[tid] = k;
        s_o[tid] = o;
    }
    __syncthreads();
    auto valid = [&](int v) { return s_g[v] < ent && (v == 0 || s_g[v] > s_g[v - 1]); };   // (starts are sorted: equal ones are one workgroup)
    int* c_pair = q.cut_pair + (size_t)x * q.cap_cut;
    int* c_e0 = q.cut_e0 + (size_t)x * q.cap_cut;
    int* c_e1 = q.cut_e1 + (size_t)x * q.cap_cut;
    int* c_wg = q.cut_wg + (size_t)x * q.cap_cut;
    int* wfirst = q.wg_first + (size_t)x * (cfg.slots + 1);
    for (int b = tid; b < n_wg + np; b += 512) {
        const bool is_cut = b < n_wg;
        int k, g;
        bool active;
        if (is_cut) {
            g = s_g[b], k = s_k[b];
            active = valid(b) && s_o[b] != 0;   // (a workgroup that starts at a pair's start is that pair start's segment)
        } else {
            k = b - n_wg;
            g = R.pl_e[k];
            active = true;
        }
        if (!active) continue;
        int inner_before = 0, starts_upto = 0, next = R.pl_e[k + 1], starts_here = 0;
        for (int v = 0; v < n_wg; v++) {
            if (!valid(v)) continue;
            const int gv = s_g[v];
            inner_before += (s_o[v] != 0 && gv < g) ? 1 : 0;
            starts_upto += gv <= g ? 1 : 0;
            starts_here += gv == g ? 1 : 0;
            if (gv > g && gv < next) next = gv;
        }
        const int idx = (is_cut ? k + 1 : k) + inner_before, wg = starts_upto - 1;
        if (idx >= q.cap_cut || wg >= cfg.slots || wg < 0) {
            atomicOr(&q.ps->bad, 4);
            continue;
        }
        c_pair[idx] = g_pl_pair[k];
        c_e0[idx] = g_pl_e0[k] + (g - R.pl_e[k]);
        c_e1[idx] = g_pl_e0[k] + (next - R.pl_e[k]);
        c_wg[idx] = wg;
        if (starts_here) wfirst[wg] = idx;   // the first segment of its workgroup
        atomicAdd(&s_cnt[0], 1);
        if (starts_here) atomicAdd(&s_cnt[1], 1);
    }
    __syncthreads();
    if (tid == 0) {
        const int n_cut = s_cnt[0], n_wgs = s_cnt[1];
        wfirst[min(n_wgs, cfg.slots)] = n_cut;
        q.ps->n_cuts[x] = n_cut;
        q.ps->n_wgs[x] = min(n_wgs, cfg.slots);
        q.ps->t_cut[x] = ev.T;
    }
}

#define PREP_LDS_RUNS 2048
#define PREP_LDS_PAIRS 1024
// One workgroup per XCD list: bucket offsets + run lists, the budget search, the final cut.
__global__ void __launch_bounds__(512) prep_split_kernel(PrepDev q, SplitCfg cfg) {
    __shared__ long long lds[512];
    __shared__ int s_run_cnt[PREP_LDS_RUNS], s_run_cost[PREP_LDS_RUNS], s_pl_n[PREP_LDS_PAIRS], s_pl_run0[PREP_LDS_PAIRS + 1];
    __shared__ double s_run_inv[PREP_LDS_RUNS];
    __shared__ int s_pl_e[PREP_LDS_PAIRS + 1];
    __shared__ long long s_pl_h[PREP_LDS_PAIRS + 1];
    __shared__ int s_jmin[2];
    (void)s_jmin;
    __shared__ long long s_cost;
    const int x = blockIdx.x, tid = threadIdx.x;
    PSTAMP(0)
    const PrepScalars& ps = *q.ps;
    const int* order = q.pair_order + (ps.by_products ? q.n_pairs : 0);
    int* g_run_cnt = q.run_cnt + (size_t)x * 16 * q.cap_pl;
    int* g_run_cost = q.run_cost + (size_t)x * 16 * q.cap_pl;
    int* g_pl_pair = q.pl_pair + (size_t)x * q.cap_pl;
    int* g_pl_n = q.pl_n + (size_t)x * q.cap_pl;
    int* g_pl_run0 = q.pl_run0 + (size_t)x * (q.cap_pl + 1);
    int* g_pl_e0 = q.pl_e0 + (size_t)x * q.cap_pl;
    int* g_pl_e = q.pl_e + (size_t)x * (q.cap_pl + 1);
    long long* g_pl_h = q.pl_h + (size_t)x * (q.cap_pl + 1);
    if (tid == 0) s_cost = 0;
    // ---- bucket offsets and run lists, the pairs in list order ----
    long long carry_e = q.ent_pre[ps.bound[x]];
    int carry_r = 0, carry_p = 0;
    long long cost_mine = 0, carry_h = 0;
    for (int base = 0; base < q.n_pairs; base += 512) {
        const int k = base + tid;
        const int pr = k < q.n_pairs ? order[k] : -1;
        int c[16], n = 0, r = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            c[i] = pr >= 0 ? q.hist[((size_t)x * q.n_pairs + pr) * 16 + i] : 0;
            n += c[i];
            r += c[i] > 0;
        }
        long long tn, tr, tp, th;
        const long long en = prep_block_scan<512>(n, lds, &tn);
        const int er = (int)prep_block_scan<512>(r, lds, &tr);
        const int ep = (int)prep_block_scan<512>(n > 0 ? 1 : 0, lds, &tp);
        long long pcost = 0;   // the pair's model cost in this list (+ its segment: H, ba_split.h)
        if (pr >= 0 && n > 0) {
            int a_, b_;
            prep_pair_ab(pr, a_, b_);
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (c[i] > 0) pcost += (long long)c[i] * split_entry_cost(q.F, a_, b_, i, cfg.cost_model);
            pcost += cfg.seg_cost;
        }
        const long long eh = prep_block_scan<512>(pcost, lds, &th);
        if (pr >= 0) {
            int a, b;
            prep_pair_ab(pr, a, b);
            long long e = carry_e + en;
            const int pl = carry_p + ep;
            int run = carry_r + er;
            const bool fits = pl < q.cap_pl;
            if (n > 0 && fits) {
                g_pl_pair[pl] = pr;
                g_pl_n[pl] = n;
                g_pl_run0[pl] = run;
                g_pl_e0[pl] = (int)e;
                g_pl_e[pl] = (int)(e - q.ent_pre[ps.bound[x]]);
                g_pl_h[pl] = carry_h + eh;
            }
            if (n > 0 && !fits) atomicOr(&q.ps->bad, 1);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                q.ebase[((size_t)x * q.n_pairs + pr) * 16 + i] = (int)e;
                e += c[i];
                if (c[i] > 0 && fits) {
                    const int cst = split_entry_cost(q.F, a, b, i, cfg.cost_model);
                    g_run_cnt[run] = c[i];
                    g_run_cost[run] = cst;
                    cost_mine += (long long)c[i] * cst;
                    run++;
                }
            }
        }
        carry_e += tn;
        carry_r += (int)tr;
        carry_p += (int)tp;
        carry_h += th;
    }
    const int np = min(carry_p, q.cap_pl), n_runs = carry_r;
    const long long ent_x = carry_e - q.ent_pre[ps.bound[x]];
    if (tid == 0) {
        g_pl_run0[np] = n_runs;
        g_pl_e[np] = (int)ent_x;
        g_pl_h[np] = carry_h;
    }
    for (int off = 32; off > 0; off >>= 1) cost_mine += __shfl_xor(cost_mine, off);
    __syncthreads();
    if ((tid & 63) == 0) atomicAdd((unsigned long long*)&s_cost, (unsigned long long)cost_mine);
    __threadfence_block();
    __syncthreads();
    const long long cost_x = s_cost;
    (void)cost_x;
    if (ent_x == 0 || np == 0) {
        if (tid == 0) {
            q.ps->n_cuts[x] = 0;
            q.ps->n_wgs[x] = 0;
            q.ps->t_cut[x] = 0;
        }
        return;
    }
    PSTAMP(1)
    // the lists in LDS when they fit (a fill reads them a few hundred times, one dependent read after another)
    if (n_runs <= PREP_LDS_RUNS && np <= PREP_LDS_PAIRS) {
        for (int i = tid; i < n_runs; i += 512) s_run_cnt[i] = g_run_cnt[i], s_run_cost[i] = g_run_cost[i], s_run_inv[i] = 1.0 / (double)g_run_cost[i];
        for (int i = tid; i < np; i += 512) s_pl_n[i] = g_pl_n[i];
        for (int i = tid; i <= np; i += 512) s_pl_run0[i] = g_pl_run0[i], s_pl_e[i] = g_pl_e[i], s_pl_h[i] = g_pl_h[i];
        __syncthreads();
        SplitRunsLds R;
        R.run_cnt = (lds_cptr)s_run_cnt, R.run_cost = (lds_cptr)s_run_cost, R.pl_n = (lds_cptr)s_pl_n, R.pl_run0 = (lds_cptr)s_pl_run0;
        R.pl_e = (lds_cptr)s_pl_e, R.pl_h = (lds_lptr)s_pl_h;
        R.run_inv = (lds_dptr)s_run_inv;
        R.np = np;
#ifdef PTAM_AB_SWITCHES   // (the measurement build keeps the greedy fill + budget search beside the even split: tools/dev/r06_split_ab.sh)
        if (cfg.greedy)
            prep_split_search(q, cfg, R, x, np, ent_x, cost_x, g_pl_pair, g_pl_e0, lds, s_jmin);
        else
#endif
            prep_split_even(q, cfg, R, x, np, ent_x, g_pl_pair, g_pl_e0);
    } else {
        __syncthreads();
        SplitRuns R;
        R.run_cnt = g_run_cnt, R.run_cost = g_run_cost, R.pl_n = g_pl_n, R.pl_run0 = g_pl_run0;
        R.pl_e = g_pl_e, R.pl_h = g_pl_h;
        R.np = np;
#ifdef PTAM_AB_SWITCHES   // (the measurement build keeps the greedy fill + budget search beside the even split: tools/dev/r06_split_ab.sh)
        if (cfg.greedy)
            prep_split_search(q, cfg, R, x, np, ent_x, cost_x, g_pl_pair, g_pl_e0, lds, s_jmin);
        else
#endif
            prep_split_even(q, cfg, R, x, np, ent_x, g_pl_pair, g_pl_e0);
    }
}

// grid (tile pair, XCD range): the entries of the pair's points in the range, placed by (pattern, point)
__global__ void __launch_bounds__(256) prep_entries_kernel(PrepDev q, BaDev d, int cost_model) {
    const int pr = blockIdx.x, x = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int a, b;
    prep_pair_ab(pr, a, b);
    if (a - b > q.ps->tband) return;
    __shared__ int run[16], wcnt[4][16], any;
    const size_t hb = ((size_t)x * q.n_pairs + pr) * 16;
    if (tid == 0) any = 0;
    __syncthreads();
    if (tid < 16) {
        run[tid] = q.ebase[hb + tid];
        if (q.hist[hb + tid] > 0) any = 1;
    }
    __syncthreads();
    if (!any) return;
    const int p0 = q.ps->bound[x], p1 = q.ps->bound[x + 1];
    for (int base = p0; base < p1; base += 256) {
        const int p = base + tid;
        int pat = 0;
        bool has = false;
        if (p < p1) {
            const int ca = prep_code(q, p, a), cb = a == b ? ca : prep_code(q, p, b);
            has = ca && cb;
            pat = ca | (cb << 2);
        }
        if (tid < 64) wcnt[tid >> 4][tid & 15] = 0;
        __syncthreads();
        int lrank = 0;
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int q0 = __shfl(pat, leader);
            const unsigned long long m = __ballot(has && pat == q0);
            if (has && pat == q0) lrank = __popcll(m & ((1ull << lane) - 1ull));
            if (lane == leader) wcnt[wave][q0] = __popcll(m);
            todo &= ~m;
        }
        __syncthreads();
        if (has) {
            int pos = run[pat] + lrank;
            for (int w = 0; w < wave; w++) pos += wcnt[w][pat];
            const int i0 = d.rowptr[p], k = q.kp[p];
            int4 ra = make_int4(0, 0, -1, -1), rb = ra;
            for (int jj = 0; jj < k; jj++) {
                const int4 r = q.ptile[i0 + jj];
                if (r.x == a) ra = r;
                if (r.x == b) rb = r;
            }
            SchurEntry en;
            en.pt = p;
            en.ma = ra.y;
            en.mb = rb.y;
            en.pad = split_entry_cost(q.F, a, b, pat, cost_model) | (pat << 16);
            en.offa[0] = (unsigned)ra.z, en.offa[1] = (unsigned)ra.w;
            en.offb[0] = (unsigned)rb.z, en.offb[1] = (unsigned)rb.w;
            if (pos >= 0 && pos < d.n_schur_entries)
                d.s_entries[pos] = en;
            else
                atomicOr(&q.ps->bad, 8);
        }
        __syncthreads();
        if (tid < 16) run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        __syncthreads();
    }
}

// exclusive scan in place of n ints in global memory by one workgroup of 1024 threads; returns the total to every thread
__device__ __forceinline__ int prep_scan_ints_1024(int* v, int n, long long* lds) {
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int i0 = min(t * per, n), i1 = min(i0 + per, n);
    int s = 0;
    for (int i = i0; i < i1; i++) s += v[i];
    long long tot;
    int b = (int)prep_block_scan<1024>(s, lds, &tot);
    for (int i = i0; i < i1; i++) {
        const int x = v[i];
        v[i] = b;
        b += x;
    }
    __threadfence_block();
    __syncthreads();
    return (int)tot;
}

// One workgroup: partial-tile slots (contiguous per pair, in creation order: XCD range, then position), the segments in block
// order (block 8 i + x = the i-th workgroup of XCD x; short lists padded with empty workgroups), workgroup heads.
// (the general form: tables in global memory — a dependent round trip per phase, ~20 us; prep_finish_kernel below takes it only for
//  more tile pairs or segments than its LDS tables hold)
__device__ __forceinline__ void prep_finish_general(const PrepDev& q, const BaDev& d, int slots, long long* lds) {
    const int t = threadIdx.x;
    PrepScalars& ps = *q.ps;
    int longest = 0;
    for (int x = 0; x < 8; x++) longest = max(longest, ps.n_wgs[x]);
    const int NB = 8 * longest;
    // segments per (pair, XCD) and the first cut of each
    for (int x = 0; x < 8; x++) {
        const int* c_pair = q.cut_pair + (size_t)x * q.cap_cut;
        for (int ci = t; ci < ps.n_cuts[x]; ci += 1024) {
            const int pr = c_pair[ci];
            atomicAdd(&q.cpx[(size_t)pr * 8 + x], 1);
            if (ci == 0 || c_pair[ci - 1] != pr) q.pair_first[(size_t)pr * 8 + x] = ci;
        }
    }
    __threadfence_block();
    __syncthreads();
    const int n_slots = prep_scan_ints_1024(q.cpx, q.n_pairs * 8, lds);
    for (int pr = t; pr < q.n_pairs; pr += 1024) d.s_pair_wg_begin[pr] = q.cpx[(size_t)pr * 8];
    if (t == 0) d.s_pair_wg_begin[q.n_pairs] = n_slots;
    // segments per block, in block order
    for (int bq = t; bq < NB; bq += 1024) {
        const int i = bq >> 3, x = bq & 7;
        const int* wfirst = q.wg_first + (size_t)x * (slots + 1);
        q.wseg_tmp[bq] = i < ps.n_wgs[x] ? wfirst[i + 1] - wfirst[i] : 0;
    }
    __threadfence_block();
    __syncthreads();
    const int n_segs = prep_scan_ints_1024(q.wseg_tmp, NB, lds);
    for (int bq = t; bq < NB; bq += 1024) d.s_wg_seg[bq] = q.wseg_tmp[bq];
    if (t == 0) d.s_wg_seg[NB] = n_segs;
    for (int x = 0; x < 8; x++) {
        const size_t cb = (size_t)x * q.cap_cut;
        const int* wfirst = q.wg_first + (size_t)x * (slots + 1);
        for (int ci = t; ci < ps.n_cuts[x]; ci += 1024) {
            const int pr = q.cut_pair[cb + ci], i = q.cut_wg[cb + ci];
            SchurWG sg;
            sg.pair = pr;
            sg.e_begin = q.cut_e0[cb + ci];
            sg.e_end = q.cut_e1[cb + ci];
            sg.slot = q.cpx[(size_t)pr * 8 + x] + (ci - q.pair_first[(size_t)pr * 8 + x]);
            d.s_segs[q.wseg_tmp[8 * i + x] + (ci - wfirst[i])] = sg;
        }
    }
    __threadfence_block();
    __syncthreads();
    // a workgroup's segment range and its first segment in one 32-byte record (ba_schur.inc)
    for (int bq = t; bq < NB; bq += 1024) {
        const int s0 = q.wseg_tmp[bq], s1 = bq + 1 < NB ? q.wseg_tmp[bq + 1] : n_segs;
        int4 h0 = make_int4(s0, s1, 0, 0), h1 = make_int4(0, 0, 0, 0);
        if (s1 > s0) {
            const SchurWG sg = d.s_segs[s0];
            h0.z = sg.pair, h0.w = sg.e_begin, h1.x = sg.e_end, h1.y = sg.slot;
        }
        ((int4*)d.s_wg_head)[2 * bq] = h0;
        ((int4*)d.s_wg_head)[2 * bq + 1] = h1;
    }
    if (t == 0) {
        ps.n_schur_wg = NB;
        ps.n_segs = n_segs;
        ps.n_slots = n_slots;
    }
}


#define PF_MAX_CUTS 2048
#define PF_MAX_CPX 4096
// The same with every table in LDS: the cuts are read ONCE, slots / block order / heads are worked out between barriers, the
// results are written once (two round trips instead of eight).
__global__ void __launch_bounds__(1024) prep_finish_kernel(PrepDev q, BaDev d, int slots) {
    __shared__ long long lds[16];
    __shared__ int c_e0[PF_MAX_CUTS], c_e1[PF_MAX_CUTS];   // per cut (all lists, list after list)
    __shared__ unsigned short c_pair[PF_MAX_CUTS], c_pos[PF_MAX_CUTS], c_wg[PF_MAX_CUTS], c_x[PF_MAX_CUTS];   // (pairs < 512, segments <= 2 048)
    __shared__ int cpx[PF_MAX_CPX + 1];
    __shared__ unsigned short pfirst[PF_MAX_CPX];
    __shared__ int wseg[513], cbase[9], nwg[8];
    const int t = threadIdx.x;
    PrepScalars& ps = *q.ps;
    if (t < 8) nwg[t] = ps.n_wgs[t];
    if (t == 0) {
        int run = 0;
        for (int x = 0; x < 8; x++) {
            cbase[x] = run;
            run += ps.n_cuts[x];
        }
        cbase[8] = run;
    }
    __syncthreads();
    const int n_all = cbase[8], n_cpx = q.n_pairs * 8;
    if (n_all > PF_MAX_CUTS || n_cpx > PF_MAX_CPX || 8 * slots > 512) {
        prep_finish_general(q, d, slots, lds);   // (its scans need the sixteen wave totals only)
        return;
    }
    int longest = 0;
    for (int x = 0; x < 8; x++) longest = max(longest, nwg[x]);
    const int NB = 8 * longest;
    for (int i = t; i < n_cpx; i += 1024) cpx[i] = 0;
    for (int bq = t; bq <= NB; bq += 1024) wseg[bq] = 0;
    for (int i = t; i < n_all; i += 1024) {
        int x = 0;
        while (i >= cbase[x + 1]) x++;
        const size_t g = (size_t)x * q.cap_cut + (i - cbase[x]);
        c_pair[i] = (unsigned short)q.cut_pair[g];
        c_e0[i] = q.cut_e0[g];
        c_e1[i] = q.cut_e1[g];
        c_wg[i] = (unsigned short)q.cut_wg[g];
        c_x[i] = (unsigned short)x;
    }
    __syncthreads();
    // segments per (pair, XCD), the first cut of each, segments per block
    for (int i = t; i < n_all; i += 1024) {
        const int x = c_x[i], pr = c_pair[i];
        atomicAdd(&cpx[pr * 8 + x], 1);
        if (i == cbase[x] || c_pair[i - 1] != pr) pfirst[pr * 8 + x] = (unsigned short)i;
        atomicAdd(&wseg[8 * c_wg[i] + x], 1);
    }
    __syncthreads();
    // two exclusive scans, each value by one thread
    int v1[4], s1 = 0;
    for (int u = 0; u < 4; u++) {
        const int i = 4 * t + u;
        v1[u] = i < n_cpx ? cpx[i] : 0;
        s1 += v1[u];
    }
    long long tot1;
    int b1 = (int)prep_block_scan<1024>(s1, lds, &tot1);
    for (int u = 0; u < 4; u++) {
        const int i = 4 * t + u;
        if (i < n_cpx) cpx[i] = b1;
        b1 += v1[u];
    }
    const int v2 = t < NB ? wseg[t] : 0;
    long long tot2;
    const int b2 = (int)prep_block_scan<1024>(v2, lds, &tot2);
    __syncthreads();
    if (t < NB) wseg[t] = b2;
    const int n_slots = (int)tot1, n_segs = (int)tot2;
    if (t == 0) wseg[NB] = n_segs;
    __syncthreads();
    // where each cut goes: its block's first segment + its index inside the block (the cuts of a workgroup are consecutive in
    // its list: index = distance from the workgroup's first cut)
    for (int i = t; i < n_all; i += 1024) {
        const int x = c_x[i], wg = c_wg[i];
        const int* wfirst = q.wg_first + (size_t)x * (slots + 1);
        c_pos[i] = (unsigned short)(wseg[8 * wg + x] + (i - cbase[x] - wfirst[wg]));
    }
    for (int pr = t; pr < q.n_pairs; pr += 1024) d.s_pair_wg_begin[pr] = cpx[pr * 8];
    if (t == 0) d.s_pair_wg_begin[q.n_pairs] = n_slots;
    for (int bq = t; bq <= NB; bq += 1024) d.s_wg_seg[bq] = wseg[bq];
    __syncthreads();
    for (int i = t; i < n_all; i += 1024) {
        const int x = c_x[i], pr = c_pair[i];
        SchurWG sg;
        sg.pair = pr;
        sg.e_begin = c_e0[i];
        sg.e_end = c_e1[i];
        sg.slot = cpx[pr * 8 + x] + (i - pfirst[pr * 8 + x]);
        d.s_segs[c_pos[i]] = sg;
        // a workgroup's segment range and its first segment in one 32-byte record (ba_schur.inc)
        const int bq = 8 * c_wg[i] + x;
        if (c_pos[i] == wseg[bq]) {
            ((int4*)d.s_wg_head)[2 * bq] = make_int4(wseg[bq], wseg[bq + 1], sg.pair, sg.e_begin);
            ((int4*)d.s_wg_head)[2 * bq + 1] = make_int4(sg.e_end, sg.slot, 0, 0);
        }
    }
    for (int bq = t; bq < NB; bq += 1024)
        if (wseg[bq + 1] == wseg[bq]) {   // (an empty workgroup of a short list)
            ((int4*)d.s_wg_head)[2 * bq] = make_int4(wseg[bq], wseg[bq], 0, 0);
            ((int4*)d.s_wg_head)[2 * bq + 1] = make_int4(0, 0, 0, 0);
        }
    if (t == 0) {
        ps.n_schur_wg = NB;
        ps.n_segs = n_segs;
        ps.n_slots = n_slots;
    }
}

// ---- deterministic mode: per tile of DET_TILE consecutive measurements the measurements by free cameras, camera-major, ascending
// measurement id inside a camera; cam_ptr rows index cam_meas globally ----
__global__ void __launch_bounds__(256) prep_det_count_kernel(BaDev d, int* tile_free) {
    const int t = blockIdx.x, m0 = t * DET_TILE, m1 = min(d.M, m0 + DET_TILE);
    __shared__ int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    int c = 0;
    for (int i = m0 + threadIdx.x; i < m1; i += 256) c += d.m_fidx[i] >= 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s, c);
    __syncthreads();
    if (threadIdx.x == 0) tile_free[t] = s;
}
__global__ void __launch_bounds__(1024) prep_det_scan_kernel(int* tile_free, int n) {
    __shared__ long long lds[1024];
    prep_scan_ints_1024(tile_free, n, lds);
}
__global__ void __launch_bounds__(256) prep_det_lists_kernel(BaDev d, const int* __restrict__ tile_base) {
    __shared__ int fidx[DET_TILE];
    const int t = blockIdx.x, m0 = t * DET_TILE, m1 = min(d.M, m0 + DET_TILE), n = m1 - m0;
    for (int i = threadIdx.x; i < n; i += 256) fidx[i] = d.m_fidx[m0 + i];
    __syncthreads();
    // thread per camera: count, then (behind a scan over the cameras) place
    int* row = d.cam_ptr + (size_t)t * (d.F + 1);
    for (int f = threadIdx.x; f < d.F; f += 256) {
        int c = 0;
        for (int i = 0; i < n; i++) c += fidx[i] == f;
        row[f + 1] = c;
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = tile_base[t];
        row[0] = acc;
        for (int f = 0; f < d.F; f++) {
            acc += row[f + 1];
            row[f + 1] = acc;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int f = threadIdx.x; f < d.F; f += 256) {
        int pos = row[f];
        for (int i = 0; i < n; i++)
            if (fidx[i] == f) d.cam_meas[pos++] = m0 + i;
    }
}
