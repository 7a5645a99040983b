// cell_sort.hpp -- what the one-workgroup counting sorts by grid cell share (csrc/ball_dense.hip, csrc/three_nn_grid.hip,
// csrc/fps.hip fps_order_kernel; the cell functions also serve csrc/ball_grid.hip):
//   cell_coord / cell_hash      the hashed (x, z) cell of the two ball-query grids;
//   RectXZ, rect_wave_reduce,   the workgroup's (x, z) bounding rectangle: the caller accumulates its own points with add() or
//   rect_total                  add_finite() -- the two treatments of non-finite values stay the callers' -- and places the barrier;
//   GlobalPoints / RegPoints    where a build kernel's points come from: re-read from global memory in every pass, or PPT points per
//                               thread loaded once into registers, each with a register memo (its cell, or bucket << 16 | rank);
//   cell_scan                   exclusive scan of the LDS counters: every counter becomes its bucket's start, the scatter cursor;
//   cell_sort                   count by cell, scan, scatter: the counting sort itself.
// The sorts are LDS-atomic and latency bound: one text for all of them costs nothing (DESIGN.md section 33 has the numbers).
#pragma once
#include "common.hpp"
#include <math.h>

namespace prcnn {

__device__ __forceinline__ unsigned cell_hash(int ix, int iz, unsigned mask)
{
    return (((unsigned)ix * 73856093u) ^ ((unsigned)iz * 19349663u)) & mask;
}

__device__ __forceinline__ int cell_coord(float v, double inv_s)
{
    double c = floor((double)v * inv_s);
    c = fmin(fmax(c, -1.0e9), 1.0e9);
    return (int)c;
}

struct RectXZ {
    float x0 = INFINITY, x1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
    // fminf / fmaxf return the operand that is a number: a NaN coordinate is passed over, an infinite one is taken
    __device__ __forceinline__ void add(float x, float z) { x0 = fminf(x0, x); x1 = fmaxf(x1, x); z0 = fminf(z0, z); z1 = fmaxf(z1, z); }
    // non-finite coordinates are skipped, each axis by itself
    __device__ __forceinline__ void add_finite(float x, float z)
    {
        if (isfinite(x)) { x0 = fminf(x0, x); x1 = fmaxf(x1, x); }
        if (isfinite(z)) { z0 = fminf(z0, z); z1 = fmaxf(z1, z); }
    }
};

// every wave's rectangle into red[4][THREADS / 64]; after the caller's barrier rect_total() is the workgroup's, in any thread
template <int THREADS>
__device__ __forceinline__ void rect_wave_reduce(RectXZ r, float (*red)[THREADS / 64])
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        r.x0 = fminf(r.x0, __shfl_xor(r.x0, d, 64)); r.x1 = fmaxf(r.x1, __shfl_xor(r.x1, d, 64));
        r.z0 = fminf(r.z0, __shfl_xor(r.z0, d, 64)); r.z1 = fmaxf(r.z1, __shfl_xor(r.z1, d, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = r.x0; red[1][w] = r.x1; red[2][w] = r.z0; red[3][w] = r.z1; }
}

template <int THREADS>
__device__ __forceinline__ RectXZ rect_total(const float (*red)[THREADS / 64])
{
    RectXZ r;
    r.x0 = red[0][0]; r.x1 = red[1][0]; r.z0 = red[2][0]; r.z1 = red[3][0];
    for (int w = 1; w < THREADS / 64; ++w) {
        r.x0 = fminf(r.x0, red[0][w]); r.x1 = fmaxf(r.x1, red[1][w]); r.z0 = fminf(r.z0, red[2][w]); r.z1 = fmaxf(r.z1, red[3][w]);
    }
    return r;
}

// A point source hands every point of the cloud that the thread owns to f(k, x, y, z, memo): k the point's index, memo the
// register in which a register source keeps what the kernel wants to remember of the point, first set by note(g) to g(x, z) (a
// global source has none and its note() does nothing: the kernel computes g again, or keeps what it needs in scratch memory).
// each(): all of them; each_chunk(): in index chunks with a barrier behind every chunk, so that what a chunk draws from an LDS
// counter lies below what the next one draws.
template <int THREADS>
struct GlobalPoints {
    static constexpr bool REG = false;
    const float *p;
    int n;
    __device__ __forceinline__ void load(const float *pts, int count) { p = pts; n = count; }
    template <class G>
    __device__ __forceinline__ void note(G) {}
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
        int none = 0;
        for (int k = threadIdx.x; k < n; k += THREADS) f(k, p[3 * k], p[3 * k + 1], p[3 * k + 2], none);
    }
    template <class F>
    __device__ __forceinline__ void each_chunk(int chunk, F f)
    {
        int none = 0;
        for (int base = 0; base < n; base += chunk) {
            const int hi = min(base + chunk, n);
            for (int k = base + threadIdx.x; k < hi; k += THREADS) f(k, p[3 * k], p[3 * k + 1], p[3 * k + 2], none);
            __syncthreads();
        }
    }
};

// thread t holds points t, t + THREADS, ...: n <= PPT * THREADS.  Every coordinate is loaded once, all loads in flight together;
// the passes of a build are then LDS and ALU work only.  A chunk is a round of THREADS consecutive indices, whatever `chunk` says.
template <int THREADS, int PPT>
struct RegPoints {
    static constexpr bool REG = true;
    float x[PPT], y[PPT], z[PPT];
    int memo[PPT];
    int n;
    __device__ __forceinline__ void load(const float *pts, int count)
    {
        n = count;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int k = j * THREADS + threadIdx.x;
            x[j] = y[j] = z[j] = 0.f;
            if (k < n) { x[j] = pts[3 * k]; y[j] = pts[3 * k + 1]; z[j] = pts[3 * k + 2]; }
        }
    }
    // memo = g(x, z) for every slot, the dead ones (zeros) included: straight-line code whose PPT chains the compiler interleaves
    template <class G>
    __device__ __forceinline__ void note(G g)
    {
#pragma unroll
        for (int j = 0; j < PPT; ++j) memo[j] = g(x[j], z[j]);
    }
    template <class F>
    __device__ __forceinline__ void each(F f)
    {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int k = j * THREADS + threadIdx.x;
            if (k < n) f(k, x[j], y[j], z[j], memo[j]);
        }
    }
    template <class F>
    __device__ __forceinline__ void each_chunk(int, F f)
    {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int k = j * THREADS + threadIdx.x;
            if (k < n) f(k, x[j], y[j], z[j], memo[j]);
            if ((j + 1) * THREADS < n + THREADS) __syncthreads();      // no barrier behind a round that holds no point
        }
    }
};

// Exclusive scan of cnt[0 .. cells) (LDS) by a workgroup of THREADS; thread t owns `per` counters -- t * per + i (contiguous: cells
// that follow each other stay with one thread, the last threads may own none), or with STRIDED t + THREADS * i (cells = per *
// THREADS; the threads of a wave read neighbouring words, conflict-free).  Every counter is left at its bucket's start, and
// sink(cell, start, count) is called for it.  wsum[THREADS / 64]: LDS; wsum_read = an earlier scan's wsum may still be being read.
template <int THREADS, bool STRIDED, class Sink>
__device__ __forceinline__ void cell_scan(int *cnt, int cells, int per, int *wsum, bool wsum_read, Sink sink)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int lo = STRIDED ? t : min(t * per, cells), step = STRIDED ? THREADS : 1;
    const int mine = STRIDED ? per : min(lo + per, cells) - lo;
    int sum = 0;
    for (int i = 0; i < mine; ++i) sum += cnt[lo + i * step];
    const int incl = wave_incl_scan(sum, lane);
    if (wsum_read) __syncthreads();
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int i = 0; i < w; ++i) run += wsum[i];
    for (int i = 0; i < mine; ++i) {
        const int c = lo + i * step;
        const int v = cnt[c];
        cnt[c] = run;
        sink(c, run, v);
        run += v;
    }
}

// The counting sort of a source's points by cell_of(x, z) < cells, over zeroed counters (with a barrier behind the zeroing):
// place(pos, k, x, y, z) is called once per point with its position in cell order (arrival order inside a cell).
template <int THREADS, class Source, class CellOf, class Sink, class Place>
__device__ __forceinline__ void cell_sort(Source &src, int *cnt, int cells, int per, int *wsum, bool wsum_read, CellOf cell_of,
                                          Sink sink, Place place)
{
    auto cell = [&](float x, float z, int memo) { return Source::REG ? memo : cell_of(x, z); };
    src.note(cell_of);
    src.each([&](int, float x, float, float z, int &memo) { atomicAdd(&cnt[cell(x, z, memo)], 1); });
    __syncthreads();
    cell_scan<THREADS, false>(cnt, cells, per, wsum, wsum_read, sink);
    __syncthreads();
    src.each([&](int k, float x, float y, float z, int &memo) { place(atomicAdd(&cnt[cell(x, z, memo)], 1), k, x, y, z); });
}

}  // namespace prcnn
