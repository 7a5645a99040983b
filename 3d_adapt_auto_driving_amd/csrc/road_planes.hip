// road_planes.hip -- the road plane of every scene of a batch of ragged LiDAR sweeps (road_planes.py): RANSAC over
// host-drawn point triples, two least-squares refits, the final inlier count and rms.  The reference project has no counterpart; the
// estimator is this package's own and road_planes.py's device="cpu" path restates it in numpy, hypothesis by hypothesis.
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles (tile_off; scene_tiles.hpp).  One call, no host read inside:
//   flag / scan / write   candidates = points whose rect x, z lie in the range, compacted in point order into cand (a scene's
//                         candidates start at its pt_off; M of them -> cand_n): ballot + popcount per tile, ordered exclusive scan,
//                         every lane recomputes its flag and stores at tile offset + popcount(ballot below the lane);
//   hypotheses            one thread per (scene, h): three candidates from the host's draws -> hyp[h] = unit normal, d, p0, accepted;
//   score                 the hot launch: a workgroup owns RP_GROUP_TILES consecutive candidate tiles of one scene (each of its four
//                         waves RP_WAVE_TILES of them), keeps their coordinates in registers as f64 and walks all hypotheses; a
//                         hypothesis' numbers are read through wave-uniform addresses (scalar loads), the count is ballot +
//                         popcount, lane h % 64 holds hypothesis h's count, the four waves' counts meet in LDS (integers, fixed
//                         order) -> part (scene, workgroup, h);
//   select                one workgroup per scene: the partials summed in workgroup order -> scores; the largest score, the smallest h
//                         among equals (one 64-bit key, maximum); the fallback rules; the starting plane and p0 -> out, p0;
//   moments / solve       three times: f64 per-thread sums over a fixed element assignment (candidate i belongs to thread
//                         i % (RP_MOMENT_GROUPS * 256)), butterfly over the wave, the four waves in wave order -> mom (scene,
//                         workgroup, 10); then one thread per scene adds the workgroups' partials in order and (rounds 0, 1) solves
//                         the shifted 3 x 3 system by Cramer's rule, or (round 2) writes inliers and rms.  No floating-point atomics.
// Arithmetic: rect coordinates f32 as kitti_io.Calibration.lidar_to_rect (point_chains.hpp); everything behind them f64 on those f32
// values, one rounding per operation (-ffp-contract=off), written in the order road_planes.py evaluates it.  Only the moment sums differ
// from the numpy path, and only in the order of their terms.
#include "common.hpp"
#include "point_chains.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int RP_THREADS = 256;                              // 4 waves
constexpr int RP_WAVE_TILES = 4;                             // candidate tiles a wave of the scoring launch keeps in registers
constexpr int RP_GROUP_TILES = PRCNN_RP_GROUP_TILES;         // ... and a workgroup
static_assert(RP_GROUP_TILES == RP_WAVE_TILES * (RP_THREADS / WAVE), "a scoring workgroup's tiles are its waves'");
constexpr int RP_HYP = PRCNN_RP_HYP;                         // doubles per hypothesis: nx, ny, nz, d, p0 x, y, z, accepted
constexpr int RP_MOM = PRCNN_RP_MOM;                         // doubles per moment partial: n, Sx, Sz, Sy, Sxx, Sxz, Szz, Sxy, Szy, Sdd
constexpr int RP_GROUPS = PRCNN_RP_MOMENT_GROUPS;            // moment workgroups per scene
constexpr int RP_OUT = PRCNN_RP_OUT;                         // doubles per scene in out
enum { RP_O_PLANE = 0, RP_O_RMS = 4, RP_O_CAND, RP_O_BEST, RP_O_RANSAC, RP_O_INLIERS, RP_O_FALLBACK };
static_assert(RP_O_FALLBACK + 1 == RP_OUT, "out row");

struct RpScenes {                                            // what scene_tile reads
    const int *pt_off, *tile_off;
};

__device__ __forceinline__ bool rp_candidate(const RpScenes &b, const SceneTile &c, const float *velo, const float *calib, double x0, double x1,
                                             double z0, double z1, float v[3])
{
    v[0] = v[1] = v[2] = 0.f;
    if (!c.valid) return false;
    lidar_to_rect_m(calib + 12 * c.s, *(const float4 *)(velo + 4 * (c.p0 + c.idx)), c.n == 1, v);
    return (double)v[0] >= x0 && (double)v[0] <= x1 && (double)v[2] >= z0 && (double)v[2] <= z1;
}

__global__ __launch_bounds__(RP_THREADS) void rp_flag_kernel(RpScenes b, const float *velo, const float *calib, double x0, double x1, double z0,
                                                             double z1, int *tile_cnt)
{
    SceneTile c;
    scene_tile<RP_THREADS>(b, blockIdx.y, c);
    if (!c.live) return;                                     // (uniform in the wave)
    float v[3];
    const unsigned long long m = __ballot(rp_candidate(b, c, velo, calib, x0, x1, z0, z1, v));
    if (c.lane == 0) tile_cnt[b.tile_off[c.s] + c.tile] = __popcll(m);
}

__global__ __launch_bounds__(RP_THREADS) void rp_scan_kernel(RpScenes b, int *tile_cnt, int *cand_n)
{
    __shared__ int wsum[RP_THREADS / WAVE];
    const int s = blockIdx.x;
    const int tot = tile_exclusive_scan<RP_THREADS>(tile_cnt + b.tile_off[s], b.tile_off[s + 1] - b.tile_off[s], 1, wsum);
    if (threadIdx.x == 0) cand_n[s] = tot;
}

__global__ __launch_bounds__(RP_THREADS) void rp_write_kernel(RpScenes b, const float *velo, const float *calib, double x0, double x1, double z0,
                                                              double z1, const int *tile_cnt, float *cand)
{
    SceneTile c;
    scene_tile<RP_THREADS>(b, blockIdx.y, c);
    if (!c.live) return;
    float v[3];
    const bool in = rp_candidate(b, c, velo, calib, x0, x1, z0, z1, v);
    const unsigned long long m = __ballot(in);
    if (!in) return;
    // the scene's candidates are rows [p0, p0 + n): a row outside them would be a counting bug, never a write into another scene
    const long pos = c.p0 + tile_cnt[b.tile_off[c.s] + c.tile] + __popcll(m & ((1ull << c.lane) - 1ull));
    if (pos >= c.p0 && pos < c.p0 + c.n) *(float4 *)(cand + 4 * pos) = make_float4(v[0], v[1], v[2], 0.f);
}

// min(floor(u M), M - 1), never below 0 (a NaN draw takes candidate 0)
__device__ __forceinline__ int rp_draw(double u, int M)
{
    const double t = floor(u * (double)M);
    return t >= 0.0 ? (t < (double)(M - 1) ? (int)t : M - 1) : 0;
}

__global__ void rp_hypothesis_kernel(int n_scenes, int iters, const int *pt_off, const int *cand_n, const float *cand, const double *draws,
                                     double cos_tilt, double *hyp)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)n_scenes * iters) return;
    const int s = (int)(q / iters), M = cand_n[s];
    double *o = hyp + RP_HYP * q;
    double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0, p[3][3] = {};
    bool ok = M >= 3;
    if (ok) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 r = *(const float4 *)(cand + 4 * ((long)pt_off[s] + rp_draw(draws[3 * q + j], M)));
            p[j][0] = r.x; p[j][1] = r.y; p[j][2] = r.z;
        }
        const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        nx = e1y * e2z - e1z * e2y;
        ny = e1z * e2x - e1x * e2z;
        nz = e1x * e2y - e1y * e2x;
        const double L = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
        ok = L > 1e-6;
        if (ok) {
            nx = __ddiv_rn(nx, L); ny = __ddiv_rn(ny, L); nz = __ddiv_rn(nz, L);
            if (ny > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            ok = -ny >= cos_tilt;
            d = -((nx * p[0][0] + ny * p[0][1]) + nz * p[0][2]);
            ok = ok && d > 0.0;
        }
    }
    o[0] = nx; o[1] = ny; o[2] = nz; o[3] = d; o[4] = p[0][0]; o[5] = p[0][1]; o[6] = p[0][2]; o[7] = ok ? 1.0 : 0.0;
}

// ---- the hot launch
__global__ __launch_bounds__(RP_THREADS) void rp_score_kernel(int iters, const int *__restrict__ pt_off, const int *__restrict__ cand_n,
                                                              const float *__restrict__ cand, const double *__restrict__ hyp,
                                                              double thresh, int *__restrict__ part)
{
    __shared__ int scount[RP_THREADS / WAVE][WAVE];
    const int s = blockIdx.y, g = blockIdx.x, M = cand_n[s];
    if ((long)g * RP_GROUP_TILES * WAVE >= M) return;        // (uniform in the workgroup) select reads the workgroups below M only
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    double x[RP_WAVE_TILES], y[RP_WAVE_TILES], z[RP_WAVE_TILES];
#pragma unroll
    for (int k = 0; k < RP_WAVE_TILES; ++k) {
        const long i = ((long)g * RP_GROUP_TILES + w * RP_WAVE_TILES + k) * WAVE + lane;
        x[k] = y[k] = z[k] = NAN;                            // no candidate here: the test below is false for it
        if (i < M) {
            const float4 r = *(const float4 *)(cand + 4 * ((long)pt_off[s] + i));
            x[k] = r.x; y[k] = r.y; z[k] = r.z;
        }
    }
    const double *hs = hyp + (long)RP_HYP * iters * s;
    int *out = part + ((long)s * gridDim.x + g) * iters;
    for (int h0 = 0; h0 < iters; h0 += WAVE) {
        int mine = 0;
        const int hn = min(WAVE, iters - h0);
        for (int j = 0; j < hn; ++j) {
            const double *q = hs + (long)RP_HYP * (h0 + j);  // a wave-uniform address: scalar loads
            int cnt = 0;
            if (q[7] != 0.0) {
                const double nx = q[0], ny = q[1], nz = q[2], d = q[3];
#pragma unroll
                for (int k = 0; k < RP_WAVE_TILES; ++k)
                    cnt += (int)__popcll(__ballot(fabs(((nx * x[k] + ny * y[k]) + nz * z[k]) + d) <= thresh));
            }
            mine = lane == j ? cnt : mine;
        }
        scount[w][lane] = mine;
        __syncthreads();
        if (w == 0 && lane < hn) out[h0 + lane] = ((scount[0][lane] + scount[1][lane]) + scount[2][lane]) + scount[3][lane];
        __syncthreads();
    }
}

__global__ __launch_bounds__(RP_THREADS) void rp_select_kernel(int iters, int n_groups, const int *cand_n, const double *hyp, const int *part,
                                                               int min_inliers, double default_height, int *scores, double *p0, double *out)
{
    __shared__ long long skey[RP_THREADS / WAVE];
    const int s = blockIdx.x, M = cand_n[s];
    const int live_groups = min(n_groups, (int)(((long)M + RP_GROUP_TILES * WAVE - 1) / (RP_GROUP_TILES * WAVE)));
    long long key = -1;                                      // score << 32 | (INT_MAX - h): the maximum is the rule of the ties
    for (int h = threadIdx.x; h < iters; h += RP_THREADS) {
        int sc = 0;
        const bool ok = hyp[RP_HYP * ((long)s * iters + h) + 7] != 0.0;
        if (ok)
            for (int g = 0; g < live_groups; ++g) sc += part[((long)s * n_groups + g) * iters + h];
        scores[(long)s * iters + h] = sc;
        if (ok) key = max(key, ((long long)sc << 32) | (long long)(0x7fffffff - h));
    }
    for (int off = 32; off >= 1; off >>= 1) key = max(key, __shfl_xor(key, off, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) skey[threadIdx.x / WAVE] = key;
    __syncthreads();
    if (threadIdx.x != 0) return;
    key = max(max(skey[0], skey[1]), max(skey[2], skey[3]));
    double *o = out + (long)RP_OUT * s, *p = p0 + 4L * s;
    const int best = key < 0 ? -1 : 0x7fffffff - (int)(key & 0x7fffffffLL), score = key < 0 ? 0 : (int)(key >> 32);
    const int fallback = M < 3 ? 1 : key < 0 ? 2 : score < min_inliers ? 3 : 0;
    o[0] = 0.0; o[1] = -1.0; o[2] = 0.0; o[3] = default_height;
    p[0] = p[1] = p[2] = p[3] = 0.0;
    if (!fallback) {
        const double *q = hyp + RP_HYP * ((long)s * iters + best);
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
        p[0] = q[4]; p[1] = q[5]; p[2] = q[6];
    }
    o[RP_O_RMS] = 0.0; o[RP_O_CAND] = M; o[RP_O_BEST] = fallback ? -1 : best; o[RP_O_RANSAC] = score; o[RP_O_INLIERS] = 0.0;
    o[RP_O_FALLBACK] = fallback;
}

__global__ __launch_bounds__(RP_THREADS) void rp_moment_kernel(const int *__restrict__ pt_off, const int *__restrict__ cand_n,
                                                               const float *__restrict__ cand, const double *__restrict__ p0,
                                                               const double *__restrict__ out, double thresh, double *__restrict__ mom)
{
    __shared__ double sm[RP_THREADS / WAVE][RP_MOM];
    const int s = blockIdx.y, M = cand_n[s];
    const double *o = out + (long)RP_OUT * s, *p = p0 + 4L * s;
    const double a = o[0], b = o[1], c = o[2], d = o[3], px = p[0], py = p[1], pz = p[2];
    double v[RP_MOM] = {};
    for (long i = (long)blockIdx.x * RP_THREADS + threadIdx.x; i < M; i += (long)RP_GROUPS * RP_THREADS) {
        const float4 r = *(const float4 *)(cand + 4 * ((long)pt_off[s] + i));
        const double x = r.x, y = r.y, z = r.z;
        const double dist = ((a * x + b * y) + c * z) + d;
        if (!(fabs(dist) <= thresh)) continue;
        const double xs = x - px, ys = y - py, zs = z - pz;
        v[0] += 1.0; v[1] += xs; v[2] += zs; v[3] += ys;
        v[4] += xs * xs; v[5] += xs * zs; v[6] += zs * zs; v[7] += xs * ys; v[8] += zs * ys;
        v[9] += dist * dist;
    }
#pragma unroll
    for (int k = 0; k < RP_MOM; ++k) {
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, WAVE);
        if ((threadIdx.x & (WAVE - 1)) == 0) sm[threadIdx.x / WAVE][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < RP_MOM)
        mom[((long)s * RP_GROUPS + blockIdx.x) * RP_MOM + threadIdx.x] =
            ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// round 0, 1: the refit; round 2: inliers and rms of the final plane
__global__ void rp_solve_kernel(int n_scenes, int round, const double *mom, const double *p0, double cos_tilt, double *out)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scenes) return;
    double *o = out + (long)RP_OUT * s;
    double m[RP_MOM];
    for (int k = 0; k < RP_MOM; ++k) {
        double acc = 0.0;
        for (int g = 0; g < RP_GROUPS; ++g) acc += mom[((long)s * RP_GROUPS + g) * RP_MOM + k];
        m[k] = acc;
    }
    if (round == 2) {
        o[RP_O_INLIERS] = m[0];
        o[RP_O_RMS] = m[0] > 0.0 ? __dsqrt_rn(__ddiv_rn(m[9], m[0])) : 0.0;
        return;
    }
    if (o[RP_O_FALLBACK] != 0.0) return;
    const double n = m[0], Sx = m[1], Sz = m[2], Sy = m[3], Sxx = m[4], Sxz = m[5], Szz = m[6], Sxy = m[7], Szy = m[8];
    const double *p = p0 + 4L * s;
    const double m00 = Szz * n - Sz * Sz, m01 = Sxz * n - Sz * Sx, m02 = Sxz * Sz - Szz * Sx;
    const double det = (Sxx * m00 - Sxz * m01) + Sx * m02;
    if (!isfinite(det) || det == 0.0) return;
    const double da = (Sxy * m00 - Sxz * (Szy * n - Sz * Sy)) + Sx * (Szy * Sz - Szz * Sy);
    const double db = (Sxx * (Szy * n - Sz * Sy) - Sxy * m01) + Sx * (Sxz * Sy - Szy * Sx);
    const double dg = (Sxx * (Szz * Sy - Szy * Sz) - Sxz * (Sxz * Sy - Szy * Sx)) + Sxy * m02;
    const double alpha = __ddiv_rn(da, det), beta = __ddiv_rn(db, det), gamma = __ddiv_rn(dg, det);
    const double norm = __dsqrt_rn((alpha * alpha + 1.0) + beta * beta);
    const double a = __ddiv_rn(alpha, norm), b = __ddiv_rn(-1.0, norm), c = __ddiv_rn(beta, norm);
    const double d = __ddiv_rn((((-alpha) * p[0] + p[1]) - beta * p[2]) + gamma, norm);
    if (!(-b >= cos_tilt) || !(d > 0.0) || !isfinite(a) || !isfinite(c) || !isfinite(d)) return;
    o[0] = a; o[1] = b; o[2] = c; o[3] = d;
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_road_planes(int n_scenes, int max_tiles, int iters, const int *pt_off, const int *tile_off, const float *velo,
                                 const float *calib, const double *draws, double x0, double x1, double z0, double z1, double thresh,
                                 double cos_tilt, int min_inliers, double default_height, int *tile_cnt, int *cand_n, float *cand,
                                 double *hyp, int *part, int *scores, double *p0, double *mom, double *out, void *stream)
{
    PRCNN_REQUIRE(n_scenes >= 0 && max_tiles >= 0 && iters >= 1, "road_planes: bad sizes");
    PRCNN_REQUIRE(n_scenes <= 65535, "road_planes: bad sizes (more than 65535 scenes)");
    if (n_scenes == 0) return PRCNN_OK;
    PRCNN_REQUIRE(pt_off && tile_off && velo && calib && draws && tile_cnt && cand_n && cand && hyp && part && scores && p0 && mom && out,
                  "road_planes: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const RpScenes b = {pt_off, tile_off};
    const int n_groups = std::max(1, (max_tiles + RP_GROUP_TILES - 1) / RP_GROUP_TILES);
    const dim3 tiles = tile_grid(max_tiles, n_scenes, RP_THREADS), threads(RP_THREADS);
    hipLaunchKernelGGL(rp_flag_kernel, tiles, threads, 0, st, b, velo, calib, x0, x1, z0, z1, tile_cnt);
    hipLaunchKernelGGL(rp_scan_kernel, dim3(n_scenes), threads, 0, st, b, tile_cnt, cand_n);
    hipLaunchKernelGGL(rp_write_kernel, tiles, threads, 0, st, b, velo, calib, x0, x1, z0, z1, tile_cnt, cand);
    const long nh = (long)n_scenes * iters;
    hipLaunchKernelGGL(rp_hypothesis_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, st, n_scenes, iters, pt_off, cand_n, cand, draws,
                       cos_tilt, hyp);
    hipLaunchKernelGGL(rp_score_kernel, dim3(n_groups, n_scenes), threads, 0, st, iters, pt_off, cand_n, cand, hyp, thresh, part);
    hipLaunchKernelGGL(rp_select_kernel, dim3(n_scenes), threads, 0, st, iters, n_groups, cand_n, hyp, part, min_inliers, default_height,
                       scores, p0, out);
    for (int round = 0; round < 3; ++round) {
        hipLaunchKernelGGL(rp_moment_kernel, dim3(RP_GROUPS, n_scenes), threads, 0, st, pt_off, cand_n, cand, p0, out, thresh, mom);
        hipLaunchKernelGGL(rp_solve_kernel, dim3((n_scenes + 63) / 64), dim3(64), 0, st, n_scenes, round, mom, p0, cos_tilt, out);
    }
    return check_launch("road_planes");
}
