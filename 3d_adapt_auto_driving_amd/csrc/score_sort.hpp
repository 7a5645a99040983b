// score_sort.hpp -- ordering scores on the device: the 64-bit key, the two LDS bitonic networks over such keys, and the host entry of
// the general sort (score_sort.hip).  The keys of one problem are distinct (the index is part of the key): any network gives THE order.
#pragma once
#include "common.hpp"

namespace prcnn {

// key: descending score, ties by ascending index
__device__ __forceinline__ unsigned long long sort_key(float score, unsigned idx)
{
    unsigned u = __float_as_uint(score);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending-order image of the float
    if (score != score) u = 0xffffffffu;              // NaN of either sign sorts FIRST, as in torch.sort(descending=True)
    return ((unsigned long long)(~u) << 32) | idx;     // inverted: larger score sorts first
}

// Pair-indexed network: n = 2^k keys in LDS, filled and fenced by the caller; the THREADS threads stride over the n / 2 pairs (lo, lo + j)
// of a pass.  For n above THREADS (score_sort.hip: up to 4096 keys on 1024 threads).
template <int THREADS>
__device__ __forceinline__ void bitonic_sort_pairs(unsigned long long *keys, int n, int t)
{
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = t; i < n / 2; i += THREADS) {
                const int lo = ((i / j) * 2 * j) + (i % j), hi = lo + j;   // pair (lo, lo + j)
                const bool up = ((lo & k) == 0);
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == up) { keys[lo] = c; keys[hi] = a; }
            }
            __syncthreads();
        }
}

// Partner-indexed network: thread t < N owns key t and exchanges with t ^ j when that partner is above it; threads t >= N only take part
// in the barriers.  For N <= the workgroup (final_stage.hip: 128 keys).
template <int N>
__device__ __forceinline__ void bitonic_sort_partner(unsigned long long *keys, int t)
{
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const int partner = t ^ j;
            if (t < N && partner > t) {
                const bool up = ((t & k) == 0);
                const unsigned long long a = keys[t], d = keys[partner];
                if ((a > d) == up) { keys[t] = d; keys[partner] = a; }
            }
            __syncthreads();
        }
}

constexpr int SS_MAX_N = 65536;     // keys per scene the general sort takes (32768 = tools/cfgs/double.yaml)
// order (b, n) i32 <- the indices of scores (b, n) in key order; owns the padded size, the chunk / merge plan and scratch slot 11
// (score_sort.hip).  Launches only: the caller checks the launch.
int score_order(int b, int n, const float *scores, int *order, hipStream_t st);

}  // namespace prcnn
