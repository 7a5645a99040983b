// beam_resample.hip -- the LiDAR beam of every point of a batch of ragged sweeps, recovered from the elevation, and the rows of the
// beams a caller keeps (beam_resample.py).  The reference project has no counterpart; the definition is
// beam_resample.py's device="cpu" path, which these kernels equal in every bit.
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles (tile_off; scene_tiles.hpp).  Three entries, no host read inside:
//   prcnn_beam_hist     a workgroup takes BR_HIST_TILES consecutive tiles of one scene: the edge table staged in LDS, per point
//                       t = z / sqrt(x x + y y) in f64 and its bin by binary search (comparisons only) -> point_bin; a workgroup-private
//                       u32 histogram in LDS, flushed with global u32 atomic adds (integer sums have no order);
//   prcnn_beam_lloyd    one workgroup per scene: 1-D Lloyd on the histogram; centres, the bin -> cluster table and the integer moments
//                       live in LDS; the moments are u64 LDS atomic adds, the one f64 operation per cluster and round is their quotient;
//   prcnn_beam_select   beam id and keep flag per point, ballot + popcount per tile, the ordered exclusive scan of scene_tiles.hpp, every
//                       kept row stored at tile offset + popcount(ballot below the lane) as four 32-bit words.
// Arithmetic: f64 on the f32 coordinates, every product, sum, quotient and root rounded once (the _rn forms; -ffp-contract=off besides);
// no transcendental function touches a point -- the table's tangents are the host's.
#include "common.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int BR_THREADS = 256;                              // 4 waves
constexpr int BR_HIST_TILES = PRCNN_BEAM_HIST_TILES;         // tiles a workgroup of the histogram launch walks with one staged table
constexpr int BR_MAX_BINS = PRCNN_BEAM_MAX_BINS;
constexpr int BR_MAX_K = PRCNN_BEAM_MAX_K;
constexpr int BR_MAX_ITERS = PRCNN_BEAM_MAX_ITERS;
// the LDS budgets: the histogram launch holds bins + 1 doubles and bins words, the Lloyd launch 3 K doubles and 2 bins words
static_assert((BR_MAX_BINS + 1) * 8 + BR_MAX_BINS * 4 <= 64 * 1024 && BR_MAX_K * 24 + BR_MAX_BINS * 8 <= 64 * 1024, "LDS budget");

struct BrScenes {                                            // what scene_tile reads
    const int *pt_off, *tile_off;
};

// the largest i with E[i] <= t among E[0 .. bins]; -1 when there is none or when it is the last edge
__device__ __forceinline__ int br_search(const double *E, int bins, double t)
{
    int lo = 0, hi = bins + 1;                               // the number of edges <= t lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (E[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1 < bins ? lo - 1 : -1;
}

__device__ __forceinline__ int br_point_bin(const float4 r, double ox, double oy, double oz, const double *E, int bins)
{
    if (!(isfinite(r.x) && isfinite(r.y) && isfinite(r.z))) return -1;
    const double x = (double)r.x - ox, y = (double)r.y - oy, z = (double)r.z - oz;
    const double rho2 = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
    if (rho2 == 0.0) return -1;
    return br_search(E, bins, __ddiv_rn(z, __dsqrt_rn(rho2)));
}

__global__ __launch_bounds__(BR_THREADS) void beam_hist_kernel(int bins, const int *__restrict__ pt_off, const float *__restrict__ velo,
                                                               const double *__restrict__ edges, double ox, double oy, double oz,
                                                               int *__restrict__ point_bin, unsigned int *__restrict__ hist)
{
    extern __shared__ double br_hist_lds[];                  // the edges (bins + 1), behind them the histogram (bins words)
    double *sE = br_hist_lds;
    unsigned int *sh = (unsigned int *)(br_hist_lds + bins + 1);
    const int s = blockIdx.y, n = pt_off[s + 1] - pt_off[s];
    const long p0 = pt_off[s], i0 = (long)blockIdx.x * BR_HIST_TILES * WAVE;
    if (i0 >= n) return;                                     // (uniform in the workgroup)
    const long i1 = min((long)n, i0 + (long)BR_HIST_TILES * WAVE);
    for (int i = threadIdx.x; i <= bins; i += BR_THREADS) sE[i] = edges[i];
    for (int i = threadIdx.x; i < bins; i += BR_THREADS) sh[i] = 0u;
    __syncthreads();
    for (long i = i0 + threadIdx.x; i < i1; i += BR_THREADS) {
        const int b = br_point_bin(*(const float4 *)(velo + 4 * (p0 + i)), ox, oy, oz, sE, bins);
        point_bin[p0 + i] = b;
        if (b >= 0) atomicAdd(sh + b, 1u);                   // LDS
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += BR_THREADS)
        if (sh[i]) atomicAdd(hist + (long)s * bins + i, sh[i]);
}

__global__ __launch_bounds__(BR_THREADS) void beam_lloyd_kernel(int bins, int K, const unsigned int *__restrict__ hist, int *__restrict__ table,
                                                                double *__restrict__ centres, unsigned int *__restrict__ counts,
                                                                int *__restrict__ iters, int *__restrict__ flags)
{
    extern __shared__ double br_lloyd_lds[];                 // centres (K), sum count * bin and sum count (K u64 each), histogram, table (bins words each)
    __shared__ int sctl[4];                                  // lowest, highest occupied bin; a bin changed cluster; the centres left their order
    double *sc = br_lloyd_lds;
    unsigned long long *snum = (unsigned long long *)(sc + K), *sden = snum + K;
    unsigned int *sh = (unsigned int *)(sden + K);
    int *sa = (int *)(sh + bins);
    const int s = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { sctl[0] = bins; sctl[1] = -1; sctl[2] = 0; sctl[3] = 0; }
    __syncthreads();
    int mylo = bins, myhi = -1;
    for (int i = tid; i < bins; i += BR_THREADS) {
        const unsigned int v = hist[(long)s * bins + i];
        sh[i] = v;
        sa[i] = -1;
        if (v) { mylo = min(mylo, i); myhi = max(myhi, i); }
    }
    if (myhi >= 0) { atomicMin(&sctl[0], mylo); atomicMax(&sctl[1], myhi); }
    __syncthreads();
    const int lo = sctl[0], hi = sctl[1];                    // hi < 0: no assigned point, no cluster
    for (int k = tid; k < K; k += BR_THREADS) {
        sc[k] = hi < 0 ? 0.0 : K == 1 ? (double)lo : __dadd_rn((double)lo, __ddiv_rn((double)((long)k * (hi - lo)), (double)(K - 1)));
        snum[k] = 0ull;
        sden[k] = 0ull;
    }
    int it = 0, cap = 0;
    while (hi >= 0) {                                        // (every exit is uniform in the workgroup)
        __syncthreads();
        if (tid == 0) sctl[2] = 0;
        __syncthreads();
        bool changed = false;
        for (int i = tid; i < bins; i += BR_THREADS) {
            if (!sh[i]) continue;
            int best = 0;
            double dbest = fabs((double)i - sc[0]);
            for (int k = 1; k < K; ++k) {
                const double d = fabs((double)i - sc[k]);
                if (d < dbest) { dbest = d; best = k; }      // equal distances stay with the lower k
            }
            if (best != sa[i]) { sa[i] = best; changed = true; }
        }
        if (changed) sctl[2] = 1;                            // (many threads, one value: no atomic needed; so for sctl[3] below)
        __syncthreads();
        if (!sctl[2]) break;
        for (int k = tid; k < K; k += BR_THREADS) { snum[k] = 0ull; sden[k] = 0ull; }
        __syncthreads();
        for (int i = tid; i < bins; i += BR_THREADS) {
            if (!sh[i]) continue;
            atomicAdd(snum + sa[i], (unsigned long long)sh[i] * (unsigned long long)i);      // LDS, integers
            atomicAdd(sden + sa[i], (unsigned long long)sh[i]);
        }
        __syncthreads();
        for (int k = tid; k < K; k += BR_THREADS)
            if (sden[k]) sc[k] = __ddiv_rn((double)snum[k], (double)sden[k]);
        if (++it == BR_MAX_ITERS) { cap = 1; break; }
    }
    __syncthreads();
    for (int k = tid + 1; k < K; k += BR_THREADS)
        if (!(sc[k - 1] <= sc[k])) sctl[3] = 1;
    __syncthreads();
    for (int i = tid; i < bins; i += BR_THREADS) table[(long)s * bins + i] = sa[i];
    for (int k = tid; k < K; k += BR_THREADS) {
        centres[(long)s * K + k] = sc[k];
        counts[(long)s * K + k] = (unsigned int)sden[k];
    }
    if (tid == 0) {
        iters[s] = it;
        flags[s] = (cap ? PRCNN_BEAM_HIT_CAP : 0) | (sctl[3] ? PRCNN_BEAM_UNSORTED : 0);
    }
}

// the beam of the lane's point (-1: unassigned, or no point) -> is the row kept
__device__ __forceinline__ bool br_keep(const SceneTile &c, int bins, int K, const int *point_bin, const int *table, const unsigned char *keep_beam,
                                        int keep_unassigned, int &beam)
{
    beam = -1;
    if (!c.valid) return false;
    const int b = point_bin[c.p0 + c.idx];
    if (b >= 0 && b < bins) beam = table[(long)c.s * bins + b];
    return beam >= 0 && beam < K ? keep_beam[beam] != 0 : keep_unassigned != 0;
}

__global__ __launch_bounds__(BR_THREADS) void beam_flag_kernel(BrScenes b, int bins, int K, const int *point_bin, const int *table,
                                                               const unsigned char *keep_beam, int keep_unassigned, int *beam_id, int *tile_cnt)
{
    SceneTile c;
    scene_tile<BR_THREADS>(b, blockIdx.y, c);
    if (!c.live) return;                                     // (uniform in the wave)
    int beam;
    const unsigned long long m = __ballot(br_keep(c, bins, K, point_bin, table, keep_beam, keep_unassigned, beam));
    if (c.valid) beam_id[c.p0 + c.idx] = beam;
    if (c.lane == 0) tile_cnt[b.tile_off[c.s] + c.tile] = __popcll(m);
}

__global__ __launch_bounds__(BR_THREADS) void beam_scan_kernel(BrScenes b, int *tile_cnt, int *kept_n)
{
    __shared__ int wsum[BR_THREADS / WAVE];
    const int s = blockIdx.x;
    const int tot = tile_exclusive_scan<BR_THREADS>(tile_cnt + b.tile_off[s], b.tile_off[s + 1] - b.tile_off[s], 1, wsum);
    if (threadIdx.x == 0) kept_n[s] = tot;
}

__global__ __launch_bounds__(BR_THREADS) void beam_write_kernel(BrScenes b, int bins, int K, const float *velo, const int *point_bin, const int *table,
                                                                const unsigned char *keep_beam, int keep_unassigned, const int *tile_cnt,
                                                                float *rows)
{
    SceneTile c;
    scene_tile<BR_THREADS>(b, blockIdx.y, c);
    if (!c.live) return;
    int beam;
    const bool keep = br_keep(c, bins, K, point_bin, table, keep_beam, keep_unassigned, beam);
    const unsigned long long m = __ballot(keep);
    if (!keep) return;
    // the scene's kept rows are rows [p0, p0 + n): a row outside them would be a counting bug, never a write into another scene
    const long pos = c.p0 + tile_cnt[b.tile_off[c.s] + c.tile] + __popcll(m & ((1ull << c.lane) - 1ull));
    if (pos >= c.p0 && pos < c.p0 + c.n) *(uint4 *)(rows + 4 * pos) = *(const uint4 *)(velo + 4 * (c.p0 + c.idx));
}

}  // namespace prcnn

using namespace prcnn;

#define BR_SIZES(what, cond) PRCNN_REQUIRE((cond) && n_scenes >= 0 && n_scenes <= 65535, what ": bad sizes")

extern "C" int prcnn_beam_hist(int n_scenes, int max_tiles, int bins, const int *pt_off, const float *velo, const double *edges, double ox,
                               double oy, double oz, int *point_bin, unsigned int *hist, void *stream)
{
    BR_SIZES("beam_hist", max_tiles >= 0);
    PRCNN_REQUIRE(bins >= 1 && bins <= BR_MAX_BINS, "beam_hist: bins must be in 1..%d (the edge table and the histogram stay in LDS)", BR_MAX_BINS);
    PRCNN_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz), "beam_hist: the origin must be finite");
    PRCNN_REQUIRE(pt_off && velo && edges && point_bin && hist, "beam_hist: null pointer");
    if (n_scenes == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, sizeof(unsigned int) * (size_t)n_scenes * bins, st) != hipSuccess) {
        set_error("beam_hist: clearing the histograms failed");
        return PRCNN_EINVAL;
    }
    const size_t lds = sizeof(double) * (bins + 1) + sizeof(unsigned int) * bins;
    const dim3 grid((unsigned)std::max(1, ceil_div(max_tiles, BR_HIST_TILES)), (unsigned)n_scenes);
    hipLaunchKernelGGL(beam_hist_kernel, grid, dim3(BR_THREADS), lds, st, bins, pt_off, velo, edges, ox, oy, oz, point_bin, hist);
    return check_launch("beam_hist");
}

extern "C" int prcnn_beam_lloyd(int n_scenes, int bins, int beams, const unsigned int *hist, int *table, double *centres, unsigned int *counts,
                                int *iters, int *flags, void *stream)
{
    BR_SIZES("beam_lloyd", true);
    PRCNN_REQUIRE(bins >= 1 && bins <= BR_MAX_BINS, "beam_lloyd: bins must be in 1..%d (the histogram and the table stay in LDS)", BR_MAX_BINS);
    PRCNN_REQUIRE(beams >= 1 && beams <= BR_MAX_K, "beam_lloyd: beams must be in 1..%d", BR_MAX_K);
    PRCNN_REQUIRE(hist && table && centres && counts && iters && flags, "beam_lloyd: null pointer");
    if (n_scenes == 0) return PRCNN_OK;
    const size_t lds = 24 * (size_t)beams + 8 * (size_t)bins;
    hipLaunchKernelGGL(beam_lloyd_kernel, dim3(n_scenes), dim3(BR_THREADS), lds, (hipStream_t)stream, bins, beams, hist, table, centres, counts,
                       iters, flags);
    return check_launch("beam_lloyd");
}

extern "C" int prcnn_beam_select(int n_scenes, int max_tiles, int bins, int beams, const int *pt_off, const int *tile_off, const float *velo,
                                 const int *point_bin, const int *table, const unsigned char *keep_beam, int keep_unassigned, int *beam_id,
                                 int *tile_cnt, int *kept_n, float *rows, void *stream)
{
    BR_SIZES("beam_select", max_tiles >= 0);
    PRCNN_REQUIRE(bins >= 1 && bins <= BR_MAX_BINS && beams >= 1 && beams <= BR_MAX_K, "beam_select: bins must be in 1..%d and beams in 1..%d",
                  BR_MAX_BINS, BR_MAX_K);
    PRCNN_REQUIRE(pt_off && tile_off && velo && point_bin && table && keep_beam && beam_id && tile_cnt && kept_n && rows, "beam_select: null pointer");
    if (n_scenes == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    const BrScenes b = {pt_off, tile_off};
    const dim3 tiles = tile_grid(max_tiles, n_scenes, BR_THREADS), threads(BR_THREADS);
    hipLaunchKernelGGL(beam_flag_kernel, tiles, threads, 0, st, b, bins, beams, point_bin, table, keep_beam, keep_unassigned, beam_id, tile_cnt);
    hipLaunchKernelGGL(beam_scan_kernel, dim3(n_scenes), threads, 0, st, b, tile_cnt, kept_n);
    hipLaunchKernelGGL(beam_write_kernel, tiles, threads, 0, st, b, bins, beams, velo, point_bin, table, keep_beam, keep_unassigned, tile_cnt, rows);
    return check_launch("beam_select");
}
