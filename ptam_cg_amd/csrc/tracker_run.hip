// tracker_run.hip — a tracked frame's two random orders drawn on the device (ptam_tracker_draw_shuffles; the definition is
// tracker_plan.h).  std::random_shuffle of src/Tracker.cc:483-484 and :597-600 becomes: a 64-bit key per point, a random high word
// over the point's index, sorted ascending; the order is the keys' low words.
//   tr_draw_lds_kernel<E>  maps of at most TR_DRAW_LDS_MAX = 8192 points.  Two workgroups of 1024 threads, one per order.  A thread
//                          holds E = 1, 2, 4 or 8 keys in registers (element e = r * 1024 + thread, r < E; the smallest E with
//                          E * 1024 >= n; the places past n hold ~0, above every key because a low word stays below 2^31), and
//                          the bitonic network over the E * 1024 places exchanges
//                            at a distance of 1024 and more between a thread's own registers,
//                            at 64..512 through LDS (8 E KB; thread t reads slot t ^ distance of row r: each 32-lane half reads
//                            32 consecutive 8-byte slots, one bank row),
//                            below 64 between the lanes of a wave.
//                          8192 places: 91 steps, of which 6 in registers, 22 through LDS, 63 between lanes.
//   beyond that            tr_keys_kernel makes the keys of both orders, mt_sort_keys (maptables.hip) sorts each, tr_low_words_kernel
//                          takes the low words; the keys live in 4 n words of the tracker's own block.
// Sizes at which the path changes: 1024, 2048, 4096 (E), 8192 (the sort in global memory, four merge passes up to 16384 keys).
#include "common.h"
#include "track_internal.h"
#include "tracker_plan.h"
#include "maptables_internal.h"   // mt_sort_keys

// tp_shuffle_key on the device; base = (2 * frame + w) << 32
__device__ __forceinline__ unsigned long long tr_key(unsigned long long seed, unsigned long long base, unsigned i) {
    unsigned long long z = seed + ((base | i) + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z >> 32) << 32 | i;
}

// the exchange of a bitonic step for the key at a place whose `lower` says it is the pair's lower place
__device__ __forceinline__ unsigned long long tr_pick(unsigned long long v, unsigned long long o, bool lower, bool ascending) {
    return (lower == ascending) ? (v < o ? v : o) : (v < o ? o : v);
}
// a step at a distance of DR rows (DR * 1024 places) between the thread's own registers
template <int E, int DR> __device__ __forceinline__ void tr_row_step(unsigned long long (&v)[E], int size) {
#pragma unroll
    for (int r = 0; r < E; r++)
        if ((r & DR) == 0 && (r | DR) < E) {
            const unsigned long long a = v[r], b = v[r | DR];
            const bool ascending = ((r << 10) & size) == 0;
            const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
            v[r] = ascending ? lo : hi;
            v[r | DR] = ascending ? hi : lo;
        }
}

// order w of n <= E * 1024 points into out, by one workgroup of 1024 threads
template <int E>
__device__ __forceinline__ void tr_draw_lds_body(int n, unsigned long long seed, unsigned long long frame, int w, int* __restrict__ out) {
    __shared__ unsigned long long ks[E * 1024];
    const int tid = threadIdx.x;
    const unsigned long long base = (2ull * frame + (unsigned long long)w) << 32;
    unsigned long long v[E];
#pragma unroll
    for (int r = 0; r < E; r++) {
        const int e = r * 1024 + tid;
        v[r] = e < n ? tr_key(seed, base, (unsigned)e) : ~0ull;
    }
    for (int size = 2; size <= E * 1024; size <<= 1)
        for (int dist = size >> 1; dist > 0; dist >>= 1) {   // (size and dist are the same for every thread)
            if (dist >= 1024) {
                if (dist == 4096) tr_row_step<E, 4>(v, size);
                else if (dist == 2048) tr_row_step<E, 2>(v, size);
                else tr_row_step<E, 1>(v, size);
                continue;
            }
            const bool lower = (tid & dist) == 0;
            if (dist >= 64) {
#pragma unroll
                for (int r = 0; r < E; r++) ks[r * 1024 + tid] = v[r];
                __syncthreads();
#pragma unroll
                for (int r = 0; r < E; r++) v[r] = tr_pick(v[r], ks[r * 1024 + (tid ^ dist)], lower, ((r * 1024 + tid) & size) == 0);
                __syncthreads();
            } else {
#pragma unroll
                for (int r = 0; r < E; r++) v[r] = tr_pick(v[r], __shfl_xor(v[r], dist, 64), lower, ((r * 1024 + tid) & size) == 0);
            }
        }
#pragma unroll
    for (int r = 0; r < E; r++) {
        const int e = r * 1024 + tid;
        if (e < n) out[e] = (int)(unsigned)v[r];
    }
}
template <int E>
__global__ void __launch_bounds__(1024) tr_draw_lds_kernel(int n, unsigned long long seed, unsigned long long frame, int* __restrict__ perm_a,
                                                           int* __restrict__ perm_b) {
    tr_draw_lds_body<E>(n, seed, frame, blockIdx.x, blockIdx.x ? perm_b : perm_a);
}
// the cameras of a batch chain: workgroup (w, y) draws order w of job y; E serves the largest map among them
template <int E> __global__ void __launch_bounds__(1024) tr_draw_lds_batch_kernel(const TrDrawJob* __restrict__ jobs) {
    const TrDrawJob j = jobs[blockIdx.y];
    tr_draw_lds_body<E>(j.n, j.seed, j.frame, blockIdx.x, blockIdx.x ? j.perm_b : j.perm_a);
}

// the keys of both orders: keys0[i], keys1[i] for i < n
__global__ void __launch_bounds__(256) tr_keys_kernel(int n, unsigned long long seed, unsigned long long frame, unsigned long long* __restrict__ keys0,
                                                      unsigned long long* __restrict__ keys1) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= 2ll * n) return;
    const int w = g >= n, i = (int)(g - (w ? n : 0));
    (w ? keys1 : keys0)[i] = tr_key(seed, (2ull * frame + (unsigned long long)w) << 32, (unsigned)i);
}
__global__ void __launch_bounds__(256) tr_low_words_kernel(int n, const unsigned long long* __restrict__ sorted0, const unsigned long long* __restrict__ sorted1,
                                                           int* __restrict__ perm_a, int* __restrict__ perm_b) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= 2ll * n) return;
    const int w = g >= n, i = (int)(g - (w ? n : 0));
    (w ? perm_b : perm_a)[i] = (int)(unsigned)(w ? sorted1 : sorted0)[i];
}

// Enqueues the draw on st: perm_a / perm_b get n entries each.  keys: 4 n words of work, needed (and looked at) only for
// n > TR_DRAW_LDS_MAX.
int tr_draw_shuffles_on(hipStream_t st, int n, uint64_t seed, uint64_t frame, int* perm_a, int* perm_b, unsigned long long* keys) {
    if (n <= 0) return PTAM_OK;
    if (n <= TR_DRAW_LDS_MAX) {
        typedef void (*fn_t)(int, unsigned long long, unsigned long long, int*, int*);
        const fn_t fn = n <= 1024 ? tr_draw_lds_kernel<1> : n <= 2048 ? tr_draw_lds_kernel<2> : n <= 4096 ? tr_draw_lds_kernel<4> : tr_draw_lds_kernel<8>;
        hipLaunchKernelGGL(fn, dim3(2), dim3(1024), 0, st, n, (unsigned long long)seed, (unsigned long long)frame, perm_a, perm_b);
    } else {
        if (!keys) {
            ptam_set_error("the draw of %d shuffle keys has no work space", n);
            return PTAM_E_STATE;
        }
        const size_t N = (size_t)n;
        const unsigned blocks = (unsigned)((2ll * n + 255) / 256);
        hipLaunchKernelGGL(tr_keys_kernel, dim3(blocks), dim3(256), 0, st, n, (unsigned long long)seed, (unsigned long long)frame, keys, keys + 2 * N);
        const unsigned long long* s0 = mt_sort_keys(st, n, keys, keys + N);
        const unsigned long long* s1 = mt_sort_keys(st, n, keys + 2 * N, keys + 3 * N);
        hipLaunchKernelGGL(tr_low_words_kernel, dim3(blocks), dim3(256), 0, st, n, s0, s1, perm_a, perm_b);
    }
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

// nb jobs in device memory, every one with 0 <= n <= n_max <= TR_DRAW_LDS_MAX: one launch
int tr_draw_shuffles_batch_on(hipStream_t st, int nb, int n_max, const TrDrawJob* d_jobs) {
    if (nb <= 0) return PTAM_OK;
    if (n_max > TR_DRAW_LDS_MAX) {
        ptam_set_error("a batched draw of %d shuffle keys exceeds the %d the kernel sorts", n_max, (int)TR_DRAW_LDS_MAX);
        return PTAM_E_ARG;
    }
    typedef void (*fn_t)(const TrDrawJob*);
    const fn_t fn = n_max <= 1024 ? tr_draw_lds_batch_kernel<1> : n_max <= 2048 ? tr_draw_lds_batch_kernel<2> : n_max <= 4096 ? tr_draw_lds_batch_kernel<4>
                                                                                                                            : tr_draw_lds_batch_kernel<8>;
    hipLaunchKernelGGL(fn, dim3(2, (unsigned)nb), dim3(1024), 0, st, d_jobs);
    HIP_TRY(hipGetLastError());
    return PTAM_OK;
}

extern "C" int ptam_shuffle_order_host(uint64_t seed, uint64_t frame, int which, int n, int32_t* out) {
    ARG_TRY((which == 0 || which == 1) && n >= 0 && (n == 0 || out));
    tp_shuffle_order(seed, frame, which, n, out);
    return PTAM_OK;
}

void tracker_run_preload_kernels() {
    ptam_preload((const void*)tr_draw_lds_kernel<1>);
    ptam_preload((const void*)tr_draw_lds_kernel<2>);
    ptam_preload((const void*)tr_draw_lds_kernel<4>);
    ptam_preload((const void*)tr_draw_lds_kernel<8>);
    ptam_preload((const void*)tr_draw_lds_batch_kernel<1>);
    ptam_preload((const void*)tr_draw_lds_batch_kernel<2>);
    ptam_preload((const void*)tr_draw_lds_batch_kernel<4>);
    ptam_preload((const void*)tr_draw_lds_batch_kernel<8>);
    ptam_preload((const void*)tr_keys_kernel);
    ptam_preload((const void*)tr_low_words_kernel);
}
