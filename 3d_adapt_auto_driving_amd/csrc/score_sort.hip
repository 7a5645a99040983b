// score_sort.hip -- the general score sort: order (b, n) <- the indices of scores (b, n) by (score descending, NaN first, index
// ascending), torch.sort(descending=True, stable=True)'s order.  The proposal layer's second launch (proposal.hip).
//
// Up to SS_CHUNK = 4096 keys a scene is one workgroup: all keys in LDS, one bitonic network (score_sort_kernel).  Beyond that one
// workgroup per scene would be 105 bitonic passes of 8 rounds each over 16384 keys, 183 us on 8 CUs while the proposal stream waits.
// So every 4096-key chunk of a scene is sorted by its own workgroup (78 passes of 2 rounds, 32 KB of LDS: score_sort_chunk_kernel),
// and the sorted runs are merged pairwise by merge-path kernels (score_merge_kernel: a thread finds its 8 outputs' split point by
// binary search and merges them): 4 x 4096 -> 2 x 8192 -> 16384, ping-pong between the two key buffers of scratch slot 11.  Keys are
// distinct, so the result is the one-workgroup kernel's (tests/test_gpu_e2e.py compares both against torch's stable sort).
#include "score_sort.hpp"

namespace prcnn {

constexpr int SS_THREADS = 1024, SS_CHUNK = 4096, SS_MERGE_V = 8;

// one workgroup per scene; n padded to npad = 2^k <= SS_CHUNK with +inf keys; writes order (b, n) i32
__global__ __launch_bounds__(SS_THREADS) void score_sort_kernel(int n, int npad, const float *__restrict__ scores,
                                                                int *__restrict__ order)
{
    extern __shared__ unsigned long long keys[];
    const int b = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < npad; i += SS_THREADS)
        keys[i] = i < n ? sort_key(scores[(long)b * n + i], (unsigned)i) : ~0ull;
    __syncthreads();
    bitonic_sort_pairs<SS_THREADS>(keys, npad, t);
    for (int i = t; i < n; i += SS_THREADS) order[(long)b * n + i] = (int)(keys[i] & 0xffffffffu);
}

__global__ __launch_bounds__(SS_THREADS) void score_sort_chunk_kernel(int n, int npad, const float *__restrict__ scores,
                                                                      unsigned long long *__restrict__ keys_out)
{
    __shared__ unsigned long long keys[SS_CHUNK];
    const int b = blockIdx.y, c0 = blockIdx.x * SS_CHUNK, t = threadIdx.x;
    for (int i = t; i < SS_CHUNK; i += SS_THREADS) {
        const int g = c0 + i;
        keys[i] = g < n ? sort_key(scores[(long)b * n + g], (unsigned)g) : ~0ull;
    }
    __syncthreads();
    bitonic_sort_pairs<SS_THREADS>(keys, SS_CHUNK, t);
    for (int i = t; i < SS_CHUNK; i += SS_THREADS) keys_out[(long)b * npad + c0 + i] = keys[i];
}

// src: per scene npad keys = sorted runs of `run` keys; dst <- runs of 2 * run (or, last round, order (b, n) i32 <- the indices)
__global__ __launch_bounds__(256) void score_merge_kernel(int n, int npad, int run, const unsigned long long *__restrict__ src,
                                                          unsigned long long *__restrict__ dst, int *__restrict__ order)
{
    const int b = blockIdx.y;
    const int g0 = (blockIdx.x * 256 + threadIdx.x) * SS_MERGE_V;
    if (g0 >= npad) return;
    const int pair = g0 / (2 * run), d = g0 - pair * 2 * run;
    const unsigned long long *__restrict__ A = src + (long)b * npad + (long)pair * 2 * run;
    const unsigned long long *__restrict__ B = A + run;
    int lo = max(0, d - run), hi = min(d, run);            // how many of the first d outputs come from A
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A[mid] < B[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int ia = lo, ib = d - lo;
    unsigned long long va = ia < run ? A[ia] : ~0ull, vb = ib < run ? B[ib] : ~0ull;
#pragma unroll
    for (int q = 0; q < SS_MERGE_V; ++q) {
        // exhausted runs read as the all-ones pad key, which also ends every run's tail: take A on equality (only pads are equal)
        const bool from_a = ib >= run || (ia < run && va <= vb);
        const unsigned long long v = from_a ? va : vb;
        if (from_a) { ++ia; va = ia < run ? A[ia] : ~0ull; } else { ++ib; vb = ib < run ? B[ib] : ~0ull; }
        const int g = g0 + q;
        if (order) { if (g < n) order[(long)b * n + g] = (int)(v & 0xffffffffu); }
        else dst[(long)b * npad + g] = v;
    }
}

int score_order(int b, int n, const float *scores, int *order, hipStream_t st)
{
    PRCNN_REQUIRE(b >= 0 && n > 0 && n <= SS_MAX_N, "score_order: bad sizes (n <= %d)", SS_MAX_N);
    if (b == 0) return PRCNN_OK;
    int npad = 1;
    while (npad < n) npad <<= 1;
    if (npad <= SS_CHUNK) {       // 32 KiB of keys at the most: below every dynamic-LDS limit
        hipLaunchKernelGGL(score_sort_kernel, dim3(b), dim3(SS_THREADS), (size_t)npad * sizeof(unsigned long long), st, n, npad, scores, order);
        return PRCNN_OK;
    }
    unsigned long long *kbuf = (unsigned long long *)scratch_for(st, (size_t)2 * b * npad * sizeof(unsigned long long), 11);
    if (!kbuf) { set_error("score_order: cannot allocate the sort scratch"); return PRCNN_ELAUNCH; }
    unsigned long long *ka = kbuf, *kb = kbuf + (size_t)b * npad;
    hipLaunchKernelGGL(score_sort_chunk_kernel, dim3(npad / SS_CHUNK, b), dim3(SS_THREADS), 0, st, n, npad, scores, ka);
    for (int run = SS_CHUNK; run < npad; run <<= 1) {
        const bool final_round = 2 * run >= npad;
        hipLaunchKernelGGL(score_merge_kernel, dim3(ceil_div(npad, 256 * SS_MERGE_V), b), dim3(256), 0, st, n, npad, run, ka, kb,
                           final_round ? order : nullptr);
        unsigned long long *tmp = ka; ka = kb; kb = tmp;
    }
    return PRCNN_OK;
}

}  // namespace prcnn
