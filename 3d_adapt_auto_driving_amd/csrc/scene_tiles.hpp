// scene_tiles.hpp -- what the ragged-scene data units share (csrc/gt_database.hip, csrc/stat_norm.hip, csrc/aug_scene.hip,
// csrc/train_input.hip, csrc/road_planes.hip, csrc/beam_resample.hip): points of all scenes sit back to back (pt_off), cut into 64-point tiles, one wave per tile (tile_off).
//   SceneTile / scene_tile   where a thread stands: scene, tile, lane, point index, whether the tile / the point exists;
//   tile_exclusive_scan      one workgroup's ordered exclusive scan over a scene's tile counts, in place;
//   tile_grid                the launch grid of a per-tile kernel: (workgroups that cover max_tiles, ny).
#pragma once
#include "common.hpp"
#include <algorithm>

namespace prcnn {

struct SceneTile {
    int s, tile, ntile, n, idx, lane;
    long p0;
    bool live, valid;                            // the tile exists in the scene; the point exists in the scene
};

// Batch: any of the prcnn_*_batch structs (pt_off, tile_off); THREADS / WAVE tiles per workgroup along blockIdx.x
template <int THREADS, class Batch>
__device__ __forceinline__ void scene_tile(const Batch &b, int s, SceneTile &c)
{
    c.s = s;
    c.tile = blockIdx.x * (THREADS / WAVE) + threadIdx.x / WAVE;
    c.ntile = b.tile_off[s + 1] - b.tile_off[s];
    c.p0 = b.pt_off[s];
    c.n = b.pt_off[s + 1] - b.pt_off[s];
    c.lane = threadIdx.x & (WAVE - 1);
    c.idx = c.tile * WAVE + c.lane;
    c.live = c.tile < c.ntile;
    c.valid = c.live && c.idx < c.n;
}

// exclusive scan of a[0], a[stride], ... (n values) in place by one workgroup of THREADS; returns the total to every thread.
// Rounds of THREADS values: inside a wave by shuffles, across the waves through wsum[THREADS / WAVE] (LDS), across the rounds by
// a carry.  A caller that scans twice over the same wsum puts a barrier between the two calls.
template <int THREADS>
__device__ __forceinline__ int tile_exclusive_scan(int *a, int n, int stride, int *wsum)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += THREADS) {
        const int i = i0 + threadIdx.x;
        const int v = i < n ? a[(long)stride * i] : 0;
        int inc = v;                             // wave_incl_scan (common.hpp) as text: through the call the scan kernels schedule differently
        for (int d = 1; d < WAVE; d <<= 1) { const int o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
        __syncthreads();
        if (lane == WAVE - 1) wsum[w] = inc;
        __syncthreads();
        int before = carry, tot = 0;
#pragma unroll
        for (int q = 0; q < THREADS / WAVE; ++q) { if (q < w) before += wsum[q]; tot += wsum[q]; }
        if (i < n) a[(long)stride * i] = before + inc - v;
        carry += tot;
    }
    return carry;
}

static inline dim3 tile_grid(int max_tiles, int ny, int threads)
{
    const int per = threads / WAVE;
    return dim3((unsigned)std::max(1, (max_tiles + per - 1) / per), (unsigned)ny);
}

}  // namespace prcnn
