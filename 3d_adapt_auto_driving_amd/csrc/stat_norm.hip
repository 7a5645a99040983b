// stat_norm.hip -- statistical normalization (stat_norm/norm.py:186-330 rescale_ptc / postprocessing) for a batch of ragged
// scenes: every Car / Van box of a KITTI scene is rescaled toward another domain's mean size, its LiDAR points with it.
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles, one wave per tile (tile_off); the rescaled boxes of all
// scenes sit back to back too (box_off).  Four passes:
//   count   velo -> rect once per point, then every box of the scene (LDS chunks of SN_CHUNK): the inside count of every
//           (box, tile) pair, the env_mask0 count and the min / max of the inside box-frame coordinates per box, the count of
//           the points outside every box per tile; then ordered exclusive scans over the tiles of every box and of the remainder;
//   choose  (avoid_conflict) the 11 env counts of every box in one sweep over the scene (bounds = min / max x the per-ratio
//           scale: exact, rounding is monotonic; a negative scale swaps them), then the first ratio that qualifies, and the
//           patch bases (the patches of the scene's boxes in label order, then the remainder);
//   write   the output cloud in the reference's order: each box's inside points in index order (a point inside two boxes goes
//           to both), then the points outside every box; scaled, rotated back, shifted (align_front), rect -> velo, (x,y,z,1) f32;
//   occlusion  each pixel's owner is the highest-index box2d that covers it (the reference paints in order), counted per object.
// All arithmetic is f64 and compiled with -ffp-contract=off.  Every np.dot of the reference is OpenBLAS dgemm: a chain of fused
// multiply-adds over the inner index, first term a plain product (tests/golden g15 pins it; a one-row product against a transposed
// matrix goes through another kernel with the middle term first, see patch_back).  cos / sin / the scale factors come from the host.
#include "common.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int SN_THREADS = 256;                  // 4 waves = 4 tiles per workgroup
constexpr int SN_CHUNK = 128;                    // boxes per LDS chunk: count pass
constexpr int SN_CCHUNK = 32;                    //                      conflict pass
constexpr int SN_WCHUNK = 48;                    //                      write pass
constexpr int SN_OCC_MAX = 2048;                 // objects per scene in the occlusion pass (LDS)
constexpr int SN_NRATIO = 11;                    // np.arange(1, -0.1, -0.1)

// per-box f64 record (boxd, PRCNN_SN_BOXD doubles: the layout is prcnn_hip.h's): the first SN_GEOM are what the point tests read
constexpr int SN_GEOM = PRCNN_SN_SCALE;
// per-box int record (boxi, PRCNN_SN_BOXI ints): the fields between the count and the ratio index never leave the device
constexpr int SN_ENV0 = 1, SN_ENV = 2, SN_BASE = 14;   // env_mask0 count, 11 env counts, patch base

struct SnCalib {                                 // row-major f64, as kitti_util.Calibration holds them
    double v2c[12], r0[9], r0inv[9], c2v[12];
};

__device__ __forceinline__ void velo_to_rect(const SnCalib &c, float px, float py, float pz, double r[3])
{
    double ref[3];
    const double x = px, y = py, z = pz;
#pragma unroll
    for (int j = 0; j < 3; ++j) {                // cart2hom . V2C^T
        double a = x * c.v2c[4 * j];
        a = fma(y, c.v2c[4 * j + 1], a);
        a = fma(z, c.v2c[4 * j + 2], a);
        ref[j] = a + c.v2c[4 * j + 3];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                // (R0 . ref^T)^T
        double a = ref[0] * c.r0[3 * j];
        a = fma(ref[1], c.r0[3 * j + 1], a);
        r[j] = fma(ref[2], c.r0[3 * j + 2], a);
    }
}

__device__ __forceinline__ void rect_to_velo(const SnCalib &c, const double p[3], float o[3])
{
    double ref[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {                // (inv(R0) . p^T)^T
        double a = p[0] * c.r0inv[3 * j];
        a = fma(p[1], c.r0inv[3 * j + 1], a);
        ref[j] = fma(p[2], c.r0inv[3 * j + 2], a);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {                // cart2hom . C2V^T
        double a = ref[0] * c.c2v[4 * j];
        a = fma(ref[1], c.c2v[4 * j + 1], a);
        a = fma(ref[2], c.c2v[4 * j + 2], a);
        o[j] = (float)(a + c.c2v[4 * j + 3]);
    }
}

// box frame of a rect point: np.dot(p - t, R)
__device__ __forceinline__ void box_frame(const double *bx, const double r[3], double f[3])
{
    const double d0 = r[0] - bx[PRCNN_SN_T], d1 = r[1] - bx[PRCNN_SN_T + 1], d2 = r[2] - bx[PRCNN_SN_T + 2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double a = d0 * bx[PRCNN_SN_R + j];
        a = fma(d1, bx[PRCNN_SN_R + 3 + j], a);
        f[j] = fma(d2, bx[PRCNN_SN_R + 6 + j], a);
    }
}

__device__ __forceinline__ bool inside_box(const double *bx, const double f[3], bool env)
{
    return f[0] > bx[PRCNN_SN_XLO] && f[0] < bx[PRCNN_SN_XHI] && f[1] > bx[PRCNN_SN_YLO] && f[1] < (env ? -0.5 : 0.0) && f[2] > bx[PRCNN_SN_ZLO] &&
           f[2] < bx[PRCNN_SN_ZHI];
}

__device__ __forceinline__ double wave_min(double v)
{
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

__device__ __forceinline__ void load_rect(const prcnn_sn_batch &b, const SceneTile &c, double r[3])
{
    r[0] = r[1] = r[2] = 0.0;
    if (c.valid) {
        const float *p = b.velo + 4 * (c.p0 + c.idx);
        velo_to_rect(((const SnCalib *)b.calib)[c.s], p[0], p[1], p[2], r);
    }
}

__device__ __forceinline__ void load_boxes(const prcnn_sn_batch &b, int b0, int nb, double *lds)
{
    __syncthreads();
    for (int i = threadIdx.x; i < nb * SN_GEOM; i += SN_THREADS)
        lds[i] = b.boxd[(long)(b0 + i / SN_GEOM) * PRCNN_SN_BOXD + i % SN_GEOM];
    __syncthreads();
}

// ---- pass 1: counts per (box, tile), env_mask0, min / max; remainder per tile
__global__ __launch_bounds__(SN_THREADS) void sn_count_kernel(prcnn_sn_batch b)
{
    __shared__ double sbox[SN_CHUNK * SN_GEOM];
    SceneTile c;
    scene_tile<SN_THREADS>(b, blockIdx.y, c);
    double r[3];
    load_rect(b, c, r);
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    bool any = false;
    for (int k0 = 0; k0 < nb; k0 += SN_CHUNK) {
        const int kn = min(SN_CHUNK, nb - k0);
        load_boxes(b, bb + k0, kn, sbox);
        if (!c.live) continue;
        for (int k = 0; k < kn; ++k) {
            const double *bx = sbox + k * SN_GEOM;
            double f[3];
            box_frame(bx, r, f);
            const bool in = c.valid && inside_box(bx, f, false);
            const bool e0 = c.valid && inside_box(bx, f, true);
            any |= in;
            const unsigned long long bin = __ballot(in), be0 = __ballot(e0);
            const int g = bb + k0 + k;
            int *bi = b.boxi + (long)g * PRCNN_SN_BOXI;
            if (c.lane == 0) {
                b.bt_cnt[b.bt_off[c.s] + (long)(k0 + k) * c.ntile + c.tile] = __popcll(bin);
                if (be0) atomicAdd(bi + SN_ENV0, (int)__popcll(be0));
            }
            if (b.avoid && bin) {
                double *mm = b.mm + 6L * g;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double lo = wave_min(in ? f[j] : INFINITY), hi = wave_max(in ? f[j] : -INFINITY);
                    if (c.lane == 0) { atomicMin(mm + j, lo); atomicMax(mm + 3 + j, hi); }
                }
            }
        }
    }
    if (c.live) {
        const unsigned long long rem = __ballot(c.valid && !any);
        if (c.lane == 0) b.rem_cnt[b.tile_off[c.s] + c.tile] = __popcll(rem);
    }
}

// ---- pass 1b: one workgroup per (box | remainder, scene): ordered offsets over the tiles, totals
__global__ __launch_bounds__(SN_THREADS) void sn_scan_kernel(prcnn_sn_batch b)
{
    __shared__ int wsum[SN_THREADS / WAVE];
    const int s = blockIdx.y, k = blockIdx.x;
    const int bb = b.box_off[s], nb = b.box_off[s + 1] - bb;
    if (k > nb) return;
    const int nt = b.tile_off[s + 1] - b.tile_off[s];
    if (k < nb) {
        const int tot = tile_exclusive_scan<SN_THREADS>(b.bt_cnt + b.bt_off[s] + (long)k * nt, nt, 1, wsum);
        if (threadIdx.x == 0) b.boxi[(long)(bb + k) * PRCNN_SN_BOXI + PRCNN_SN_CNT] = tot;
    } else {
        const int tot = tile_exclusive_scan<SN_THREADS>(b.rem_cnt + b.tile_off[s], nt, 1, wsum);
        if (threadIdx.x == 0) b.scene_i[4 * s + 0] = tot;
    }
}

// ---- pass 2 (avoid_conflict): the 11 env counts of every box with inside points
__global__ __launch_bounds__(SN_THREADS) void sn_conflict_kernel(prcnn_sn_batch b)
{
    __shared__ double sbox[SN_CCHUNK * SN_GEOM];
    __shared__ double sbnd[SN_CCHUNK * SN_NRATIO * 5];      // per box and ratio: xlo, xhi, ylo, zlo, zhi
    __shared__ int scnt[SN_CCHUNK];
    SceneTile c;
    scene_tile<SN_THREADS>(b, blockIdx.y, c);
    double r[3];
    load_rect(b, c, r);
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    for (int k0 = 0; k0 < nb; k0 += SN_CCHUNK) {
        const int kn = min(SN_CCHUNK, nb - k0);
        load_boxes(b, bb + k0, kn, sbox);
        for (int i = threadIdx.x; i < kn * SN_NRATIO; i += SN_THREADS) {
            const int k = i / SN_NRATIO, q = i % SN_NRATIO;
            const double *mm = b.mm + 6L * (bb + k0 + k);
            const double *sc = b.boxd + (long)(bb + k0 + k) * PRCNN_SN_BOXD + PRCNN_SN_SCALE + 3 * q;
            double lo[3], hi[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {                    // min / max of (inside coordinate * scale)
                lo[j] = sc[j] >= 0.0 ? mm[j] * sc[j] : mm[3 + j] * sc[j];
                hi[j] = sc[j] >= 0.0 ? mm[3 + j] * sc[j] : mm[j] * sc[j];
            }
            double *o = sbnd + (long)i * 5;
            o[0] = lo[0]; o[1] = hi[0]; o[2] = lo[1]; o[3] = lo[2]; o[4] = hi[2];
            if (q == 0) scnt[k] = b.boxi[(long)(bb + k0 + k) * PRCNN_SN_BOXI + PRCNN_SN_CNT];
        }
        __syncthreads();
        if (!c.live) continue;
        for (int k = 0; k < kn; ++k) {
            if (scnt[k] == 0) continue;
            double f[3];
            box_frame(sbox + k * SN_GEOM, r, f);
            int *env = b.boxi + (long)(bb + k0 + k) * PRCNN_SN_BOXI + SN_ENV;
            for (int q = 0; q < SN_NRATIO; ++q) {
                const double *o = sbnd + (long)(k * SN_NRATIO + q) * 5;
                const bool e = c.valid && f[0] > o[0] && f[0] < o[1] && f[1] > o[2] && f[1] < -0.5 && f[2] > o[3] && f[2] < o[4];
                const unsigned long long m = __ballot(e);
                if (c.lane == 0 && m) atomicAdd(env + q, (int)__popcll(m));
            }
        }
    }
}

// ---- pass 2b: one thread per scene -- the ratio of every box, patch bases, output size
__global__ void sn_choose_kernel(prcnn_sn_batch b, int n_scenes)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_scenes) return;
    int base = 0;
    for (int g = b.box_off[s]; g < b.box_off[s + 1]; ++g) {
        int *bi = b.boxi + (long)g * PRCNN_SN_BOXI;
        const int cnt = bi[PRCNN_SN_CNT];
        int q = -1;                                           // no inside point: ratio 0
        if (cnt > 0) {
            q = 0;                                            // ratio 1
            if (b.avoid) {
                q = SN_NRATIO - 1;                            // none qualifies: the last value stands
                for (int i = 0; i < SN_NRATIO; ++i)
                    if (bi[SN_ENV + i] - bi[SN_ENV0] < 10) { q = i; break; }
            }
        }
        bi[PRCNN_SN_RIDX] = q;
        bi[SN_BASE] = base;
        base += cnt;
    }
    b.scene_i[4 * s + 1] = base;
    b.scene_i[4 * s + 2] = base + b.scene_i[4 * s + 0];
}

// patch point back to rect: np.dot(f * scale, R^T) + t, then the align_front shifts.  A patch of ONE point is a (1,3) . (3,3)^T
// product, which OpenBLAS runs through its gemv kernel: the middle term first.
__device__ __forceinline__ void patch_back(const double *bx, const double f[3], int single, double p[3])
{
    const double *fs = bx + PRCNN_SN_FSCALE;
    const double a0 = f[0] * fs[0], a1 = f[1] * fs[1], a2 = f[2] * fs[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double *Rj = bx + PRCNN_SN_R + 3 * j;                 // row j of R = column j of R^T
        double a;
        if (single) { a = a1 * Rj[1]; a = fma(a0, Rj[0], a); a = fma(a2, Rj[2], a); }
        else { a = a0 * Rj[0]; a = fma(a1, Rj[1], a); a = fma(a2, Rj[2], a); }
        p[j] = a + bx[PRCNN_SN_T + j];
    }
    if (bx[PRCNN_SN_FLAG1] != 0.0) { p[0] = p[0] + bx[PRCNN_SN_SHIFT]; p[2] = p[2] + bx[PRCNN_SN_SHIFT + 1]; }
    if (bx[PRCNN_SN_FLAG2] != 0.0) { p[0] = p[0] + bx[PRCNN_SN_SHIFT + 2]; p[2] = p[2] + bx[PRCNN_SN_SHIFT + 3]; }
}

// the scene's rows are [o0, o1): a row outside them would be a counting bug, never a write into another scene or past the buffer
__device__ __forceinline__ void store_point(float *out, long pos, long o0, long o1, const float v[3])
{
    if (pos >= o0 && pos < o1) *(float4 *)(out + 4 * pos) = make_float4(v[0], v[1], v[2], 1.0f);
}

// ---- pass 3: the output clouds
__global__ __launch_bounds__(SN_THREADS) void sn_write_kernel(prcnn_sn_batch b)
{
    __shared__ double sbox[SN_WCHUNK * PRCNN_SN_BOXD];
    __shared__ int sbase[SN_WCHUNK], scnt[SN_WCHUNK];
    SceneTile c;
    scene_tile<SN_THREADS>(b, blockIdx.y, c);
    double r[3];
    load_rect(b, c, r);
    const SnCalib &cal = ((const SnCalib *)b.calib)[c.s];
    const long o0 = b.out_off[c.s], o1 = b.out_off[c.s + 1];
    const unsigned long long below = (1ull << c.lane) - 1ull;
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    bool any = false;
    for (int k0 = 0; k0 < nb; k0 += SN_WCHUNK) {
        const int kn = min(SN_WCHUNK, nb - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < kn * PRCNN_SN_BOXD; i += SN_THREADS) sbox[i] = b.boxd[(long)(bb + k0) * PRCNN_SN_BOXD + i];
        for (int i = threadIdx.x; i < kn; i += SN_THREADS) {
            sbase[i] = b.boxi[(long)(bb + k0 + i) * PRCNN_SN_BOXI + SN_BASE];
            scnt[i] = b.boxi[(long)(bb + k0 + i) * PRCNN_SN_BOXI + PRCNN_SN_CNT];
        }
        __syncthreads();
        if (!c.live) continue;
        for (int k = 0; k < kn; ++k) {
            if (scnt[k] == 0) continue;
            const double *bx = sbox + k * PRCNN_SN_BOXD;
            double f[3];
            box_frame(bx, r, f);
            const bool in = c.valid && inside_box(bx, f, false);
            const unsigned long long m = __ballot(in);
            if (!m) continue;
            any |= in;
            if (in) {
                const long pos = o0 + sbase[k] + b.bt_cnt[b.bt_off[c.s] + (long)(k0 + k) * c.ntile + c.tile] + __popcll(m & below);
                double p[3];
                float v[3];
                patch_back(bx, f, scnt[k] == 1, p);
                rect_to_velo(cal, p, v);
                store_point(b.out, pos, o0, o1, v);
            }
        }
    }
    const bool rest = c.valid && !any;
    const unsigned long long m = __ballot(rest);
    if (rest) {
        const long pos = o0 + b.scene_i[4 * c.s + 1] + b.rem_cnt[b.tile_off[c.s] + c.tile] + __popcll(m & below);
        float v[3];
        rect_to_velo(cal, r, v);
        store_point(b.out, pos, o0, o1, v);
    }
}

// ---- occlusion: pixel owner = highest object index whose box2d rectangle covers it; counts per object
__global__ __launch_bounds__(SN_THREADS) void sn_occlusion_kernel(int h, int w, const int *obj_off, const int *rects, int *counts)
{
    __shared__ int srect[SN_OCC_MAX * 4];
    __shared__ int shist[SN_OCC_MAX];
    const int s = blockIdx.y;
    const int o0 = obj_off[s], no = obj_off[s + 1] - o0;
    for (int i = threadIdx.x; i < no * 4; i += SN_THREADS) srect[i] = rects[4L * o0 + i];
    for (int i = threadIdx.x; i < no; i += SN_THREADS) shist[i] = 0;
    __syncthreads();
    const long npix = (long)h * w;
    for (long p = (long)blockIdx.x * SN_THREADS + threadIdx.x; p < npix; p += (long)gridDim.x * SN_THREADS) {
        const int y = (int)(p / w), x = (int)(p % w);
        for (int i = no - 1; i >= 0; --i) {
            const int *rc = srect + 4 * i;                    // y0, y1, x0, x1 (half-open, already clipped)
            if (y >= rc[0] && y < rc[1] && x >= rc[2] && x < rc[3]) { atomicAdd(&shist[i], 1); break; }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < no; i += SN_THREADS)
        if (shist[i]) atomicAdd(counts + o0 + i, shist[i]);
}

}  // namespace prcnn

using namespace prcnn;

static int sn_check(const prcnn_sn_batch *b, const char *what)
{
    PRCNN_REQUIRE(b, "%s: null pointer", what);
    PRCNN_REQUIRE(b->n_scenes >= 0 && b->max_tiles >= 0 && b->max_boxes >= 0, "%s: bad sizes", what);
    PRCNN_REQUIRE(b->pt_off && b->tile_off && b->box_off && b->bt_off && b->velo && b->calib && b->boxd && b->boxi && b->bt_cnt &&
                      b->rem_cnt && b->scene_i && (!b->avoid || b->mm),
                  "%s: null pointer", what);
    return PRCNN_OK;
}

extern "C" int prcnn_stat_norm_count(const prcnn_sn_batch *b, void *stream)
{
    const int rc = sn_check(b, "stat_norm_count");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sn_count_kernel, tile_grid(b->max_tiles, b->n_scenes, SN_THREADS), dim3(SN_THREADS), 0, st, *b);
    hipLaunchKernelGGL(sn_scan_kernel, dim3(b->max_boxes + 1, b->n_scenes), dim3(SN_THREADS), 0, st, *b);
    return check_launch("stat_norm_count");
}

extern "C" int prcnn_stat_norm_choose(const prcnn_sn_batch *b, void *stream)
{
    const int rc = sn_check(b, "stat_norm_choose");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (b->avoid && b->max_boxes > 0) hipLaunchKernelGGL(sn_conflict_kernel, tile_grid(b->max_tiles, b->n_scenes, SN_THREADS), dim3(SN_THREADS), 0, st, *b);
    hipLaunchKernelGGL(sn_choose_kernel, dim3((b->n_scenes + 63) / 64), dim3(64), 0, st, *b, b->n_scenes);
    return check_launch("stat_norm_choose");
}

extern "C" int prcnn_stat_norm_write(const prcnn_sn_batch *b, void *stream)
{
    const int rc = sn_check(b, "stat_norm_write");
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(b->out_off && b->out, "stat_norm_write: null pointer");
    if (b->n_scenes == 0) return PRCNN_OK;
    hipLaunchKernelGGL(sn_write_kernel, tile_grid(b->max_tiles, b->n_scenes, SN_THREADS), dim3(SN_THREADS), 0, (hipStream_t)stream, *b);
    return check_launch("stat_norm_write");
}

extern "C" int prcnn_stat_norm_occlusion(int n_scenes, int h, int w, int max_objects, const int *obj_off, const int *rects,
                                         int *counts, void *stream)
{
    PRCNN_REQUIRE(n_scenes >= 0 && h >= 0 && w >= 0 && max_objects >= 0, "stat_norm_occlusion: bad sizes");
    PRCNN_REQUIRE(max_objects <= SN_OCC_MAX, "stat_norm_occlusion: bad sizes (more than %d objects in a scene)", SN_OCC_MAX);
    if (n_scenes == 0 || max_objects == 0 || (long)h * w == 0) return PRCNN_OK;
    PRCNN_REQUIRE(obj_off && rects && counts, "stat_norm_occlusion: null pointer");
    const long npix = (long)h * w;
    const int gx = (int)std::min<long>(32, (npix + SN_THREADS * 16 - 1) / (SN_THREADS * 16));
    hipLaunchKernelGGL(sn_occlusion_kernel, dim3(gx, n_scenes), dim3(SN_THREADS), 0, (hipStream_t)stream, h, w, obj_off, rects, counts);
    return check_launch("stat_norm_occlusion");
}
