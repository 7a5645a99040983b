// bev_render.hip -- bird's-eye-view scene images (stat_norm/visualize.py compare_stat_norm, as PNG pixels): the object mask and the
// point binning over a ragged batch of clouds, then the image composition with exact box outlines.  bev.py holds the numpy
// definition of every count, flag and pixel; DESIGN.md section 37.
//
//   bin      one wave per 64-point tile (scene_tiles.hpp).  lidar -> rect in f64, one rounding per operation (-ffp-contract=off, no
//            fma: the checker's elementwise sums); every box of the cloud (LDS chunks of PRCNN_BEV_BOX_CHUNK f64 records, rotation made
//            on the host) decides "inside" exactly as stat_norm's inside_box does; the point's layer is its layer_in / layer_out byte;
//            x, z rounded to f32 and binned; one u32 atomicAdd per kept point straight to the count plane (the data are sparse), the
//            binned / dropped totals summed per wave (ballot + popcount) before one atomic each.  Integer atomics only.
//   compose  one thread per pixel, 16 x 16 pixels per workgroup.  The image's segments pass through LDS PRCNN_BEV_SEG_CHUNK at a time:
//            each thread culls one segment by its bounding box grown by R against the tile's pixel centres, the survivors are
//            compacted in list order, every pixel runs the int64 distance test over them and keeps the last match.  No atomics; the
//            result of a pixel does not depend on the launch shape.
#include "common.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int BEV_THREADS = 256;                 // bin: 4 waves = 4 tiles per workgroup; compose: 16 x 16 pixels
constexpr int BEV_TILE = 16;
static_assert(PRCNN_BEV_SEG_CHUNK == BEV_THREADS, "the cull takes one segment per thread and pass");
static_assert(PRCNN_BEV_BOXD == PRCNN_SN_ZHI + 1, "a box record ends with the five bounds");

struct BevBatch {                                // prcnn_bev_bin's arguments, as the kernel and scene_tile read them
    int n_clouds, max_tiles, n_images, height, width;
    float x0, z0, inv;
    const int *pt_off, *tile_off, *box_off, *image;
    const float *velo;
    const double *calib, *boxd;
    const unsigned char *layer_out, *layer_in;
    unsigned int *counts;
    unsigned char *cls;
    int *stats;
};

struct BevCalib {                                // row-major f64, as stat_norm.Calib holds them
    double v2c[12], r0[9];
};

// R0 (V2C [p 1]): plain products and sums, left to right
__device__ __forceinline__ void bev_rect(const BevCalib &c, float px, float py, float pz, double r[3])
{
    const double x = px, y = py, z = pz;
    double ref[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) ref[j] = ((x * c.v2c[4 * j] + y * c.v2c[4 * j + 1]) + z * c.v2c[4 * j + 2]) + c.v2c[4 * j + 3];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = (ref[0] * c.r0[3 * j] + ref[1] * c.r0[3 * j + 1]) + ref[2] * c.r0[3 * j + 2];
}

// f = (r - t) R, strictly inside the bounds
__device__ __forceinline__ bool bev_inside(const double *bx, const double r[3])
{
    const double d0 = r[0] - bx[PRCNN_SN_T], d1 = r[1] - bx[PRCNN_SN_T + 1], d2 = r[2] - bx[PRCNN_SN_T + 2];
    double f[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = (d0 * bx[PRCNN_SN_R + j] + d1 * bx[PRCNN_SN_R + 3 + j]) + d2 * bx[PRCNN_SN_R + 6 + j];
    return f[0] > bx[PRCNN_SN_XLO] && f[0] < bx[PRCNN_SN_XHI] && f[1] > bx[PRCNN_SN_YLO] && f[1] < 0.0 && f[2] > bx[PRCNN_SN_ZLO] &&
           f[2] < bx[PRCNN_SN_ZHI];
}

__global__ __launch_bounds__(BEV_THREADS) void bev_bin_kernel(BevBatch b)
{
    __shared__ double sbox[PRCNN_BEV_BOX_CHUNK * PRCNN_BEV_BOXD];
    SceneTile c;
    scene_tile<BEV_THREADS>(b, blockIdx.y, c);
    double r[3] = {0.0, 0.0, 0.0};
    if (c.valid) {
        const float *p = b.velo + 4 * (c.p0 + c.idx);
        bev_rect(((const BevCalib *)b.calib)[c.s], p[0], p[1], p[2], r);
    }
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    bool in = false;
    for (int k0 = 0; k0 < nb; k0 += PRCNN_BEV_BOX_CHUNK) {
        const int kn = min(PRCNN_BEV_BOX_CHUNK, nb - k0);
        __syncthreads();
        for (int i = threadIdx.x; i < kn * PRCNN_BEV_BOXD; i += BEV_THREADS) sbox[i] = b.boxd[(long)(bb + k0) * PRCNN_BEV_BOXD + i];
        __syncthreads();
        if (!c.valid) continue;
        for (int k = 0; k < kn; ++k) in |= bev_inside(sbox + k * PRCNN_BEV_BOXD, r);
    }
    if (!c.live) return;                         // behind the last barrier
    const long p = c.p0 + c.idx;
    const int img = b.image[c.s];
    int layer = PRCNN_BEV_LAYERS;
    if (c.valid) {
        layer = in ? b.layer_in[p] : b.layer_out[p];
        if (b.cls) b.cls[p] = in ? 1 : 0;
    }
    const bool drawn = c.valid && layer < PRCNN_BEV_LAYERS && img >= 0 && img < b.n_images;
    const float u = ((float)r[0] - b.x0) * b.inv, v = ((float)r[2] - b.z0) * b.inv;
    const bool keep = drawn && u >= 0.0f && u < (float)b.width && v >= 0.0f && v < (float)b.height;     // a NaN drops the point
    if (keep) {
        const int col = (int)floorf(u), row = b.height - 1 - (int)floorf(v);
        if (col >= 0 && col < b.width && row >= 0 && row < b.height)
            atomicAdd(b.counts + (((long)img * PRCNN_BEV_LAYERS + layer) * b.height + row) * b.width + col, 1u);
    }
#pragma unroll
    for (int l = 0; l < PRCNN_BEV_LAYERS; ++l) {
        const unsigned long long mk = __ballot(keep && layer == l), md = __ballot(drawn && !keep && layer == l);
        if (c.lane == 0) {
            int *st = b.stats + ((long)img * PRCNN_BEV_LAYERS + l) * 2;
            if (mk) atomicAdd(st, (int)__popcll(mk));
            if (md) atomicAdd(st + 1, (int)__popcll(md));
        }
    }
}

// is the pixel centre (px, py) within R of the segment g = ax, ay, bx, by?  int64 throughout (bounds: prcnn_hip.h)
__device__ __forceinline__ bool bev_seg_hit(long long px, long long py, const int *g, long long r2)
{
    const long long ax = g[0], ay = g[1], dx = (long long)g[2] - ax, dy = (long long)g[3] - ay, qx = px - ax, qy = py - ay;
    const long long len = dx * dx + dy * dy, t = qx * dx + qy * dy;
    if (t <= 0) return qx * qx + qy * qy <= r2;              // a zero-length segment is its endpoint (t = 0)
    if (t >= len) {
        const long long ex = px - g[2], ey = py - g[3];
        return ex * ex + ey * ey <= r2;
    }
    const long long cr = qx * dy - qy * dx;
    return cr * cr <= r2 * len;
}

__device__ __forceinline__ int bev_step(unsigned int n) { return min(31 - __clz((int)n), 3); }     // floor(log2 n), n > 0: a bit scan

__global__ __launch_bounds__(BEV_THREADS) void bev_compose_kernel(int height, int width, int radius, int n_palette,
                                                                  const unsigned int *counts, const int *seg_off, const int *segs,
                                                                  const unsigned char *palette, unsigned char *rgb)
{
    __shared__ int sseg[PRCNN_BEV_SEG_CHUNK * PRCNN_BEV_SEG];
    __shared__ int wcnt[BEV_THREADS / WAVE];
    __shared__ unsigned char spal[PRCNN_BEV_PALETTE_MAX * 3];
    const int s = blockIdx.z;
    const int c0 = blockIdx.x * BEV_TILE, r0 = blockIdx.y * BEV_TILE;
    const int col = c0 + (threadIdx.x & (BEV_TILE - 1)), row = r0 + threadIdx.x / BEV_TILE;
    const bool live = col < width && row < height;
    for (int i = threadIdx.x; i < n_palette * 3; i += BEV_THREADS) spal[i] = palette[i];
    // the tile's pixel centres, grown by R: a segment whose bounding box misses this rectangle is farther than R from every one
    const int tx0 = 8 * c0 + 4 - radius, tx1 = 8 * min(c0 + BEV_TILE - 1, width - 1) + 4 + radius;
    const int ty0 = 8 * r0 + 4 - radius, ty1 = 8 * min(r0 + BEV_TILE - 1, height - 1) + 4 + radius;
    const long long px = 8LL * col + 4, py = 8LL * row + 4, r2 = (long long)radius * radius;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int q1 = seg_off[s + 1];
    int hit = -1;
    for (int q0 = seg_off[s]; q0 < q1; q0 += PRCNN_BEV_SEG_CHUNK) {
        const int q = q0 + threadIdx.x;
        int g[PRCNN_BEV_SEG] = {0, 0, 0, 0, -1};
        bool keep = false;
        if (q < q1) {
#pragma unroll
            for (int j = 0; j < PRCNN_BEV_SEG; ++j) g[j] = segs[(long)q * PRCNN_BEV_SEG + j];
            keep = g[4] >= 0 && g[4] < n_palette && max(g[0], g[2]) >= tx0 && min(g[0], g[2]) <= tx1 && max(g[1], g[3]) >= ty0 &&
                   min(g[1], g[3]) <= ty1;
        }
        const unsigned long long m = __ballot(keep);
        __syncthreads();                         // the pass before has been read
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        int base = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < BEV_THREADS / WAVE; ++i) { if (i < w) base += wcnt[i]; tot += wcnt[i]; }
        if (keep) {
            int *o = sseg + (base + __popcll(m & below)) * PRCNN_BEV_SEG;       // list order kept: the last match wins
#pragma unroll
            for (int j = 0; j < PRCNN_BEV_SEG; ++j) o[j] = g[j];
        }
        __syncthreads();
        if (!live) continue;
        for (int i = 0; i < tot; ++i)
            if (bev_seg_hit(px, py, sseg + i * PRCNN_BEV_SEG, r2)) hit = sseg[i * PRCNN_BEV_SEG + 4];
    }
    __syncthreads();                             // the palette (an image without segments has met no barrier)
    if (!live) return;
    int pal = 0;
    if (hit >= 0) {
        pal = hit;
    } else {
        const long plane = (long)height * width, at = (long)row * width + col;
        const unsigned int *cs = counts + (long)s * PRCNN_BEV_LAYERS * plane;
        for (int l = PRCNN_BEV_LAYERS - 1; l >= 0; --l) {
            const unsigned int n = cs[l * plane + at];
            if (n) { pal = 1 + 4 * l + bev_step(n); break; }
        }
    }
    unsigned char *o = rgb + (((long)s * height + row) * width + col) * 3;
    o[0] = spal[3 * pal]; o[1] = spal[3 * pal + 1]; o[2] = spal[3 * pal + 2];
}

}  // namespace prcnn

using namespace prcnn;

static bool bev_side(int v) { return v >= 1 && v <= PRCNN_BEV_MAX_SIDE; }

extern "C" int prcnn_bev_bin(int n_clouds, int max_tiles, int n_images, int height, int width, float x0, float z0, float inv,
                             const int *pt_off, const int *tile_off, const int *box_off, const int *image, const float *velo,
                             const double *calib, const double *boxd, const unsigned char *layer_out, const unsigned char *layer_in,
                             unsigned int *counts, unsigned char *cls, int *stats, void *stream)
{
    PRCNN_REQUIRE(n_clouds >= 0 && max_tiles >= 0 && n_images >= 0 && bev_side(height) && bev_side(width),
                  "bev_bin: bad sizes (an image side is 1..%d pixels)", PRCNN_BEV_MAX_SIDE);
    if (n_images == 0) return PRCNN_OK;
    PRCNN_REQUIRE(counts && stats, "bev_bin: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t planes = (size_t)n_images * PRCNN_BEV_LAYERS;
    if (hipMemsetAsync(counts, 0, planes * height * width * sizeof(unsigned int), st) != hipSuccess ||
        hipMemsetAsync(stats, 0, planes * 2 * sizeof(int), st) != hipSuccess) {
        set_error("bev_bin: zeroing the count planes failed: %s", hipGetErrorString(hipGetLastError()));
        return PRCNN_ELAUNCH;
    }
    if (n_clouds == 0 || max_tiles == 0) return PRCNN_OK;
    PRCNN_REQUIRE(pt_off && tile_off && box_off && image && velo && calib && boxd && layer_out && layer_in, "bev_bin: null pointer");
    const BevBatch b = {n_clouds, max_tiles, n_images, height, width, x0, z0, inv, pt_off, tile_off, box_off, image, velo, calib, boxd,
                        layer_out, layer_in, counts, cls, stats};
    hipLaunchKernelGGL(bev_bin_kernel, tile_grid(max_tiles, n_clouds, BEV_THREADS), dim3(BEV_THREADS), 0, st, b);
    return check_launch("bev_bin");
}

extern "C" int prcnn_bev_compose(int n_images, int height, int width, int line_px, int n_palette, const unsigned int *counts,
                                 const int *seg_off, const int *segs, const unsigned char *palette, unsigned char *rgb, void *stream)
{
    PRCNN_REQUIRE(n_images >= 0 && n_images <= 65535 && bev_side(height) && bev_side(width) && line_px >= 1 && line_px <= PRCNN_BEV_MAX_LINE &&
                      n_palette >= 1 + 4 * PRCNN_BEV_LAYERS && n_palette <= PRCNN_BEV_PALETTE_MAX,
                  "bev_compose: bad sizes (an image side is 1..%d pixels, line_px 1..%d, the palette %d..%d rows)", PRCNN_BEV_MAX_SIDE,
                  PRCNN_BEV_MAX_LINE, 1 + 4 * PRCNN_BEV_LAYERS, PRCNN_BEV_PALETTE_MAX);
    if (n_images == 0) return PRCNN_OK;
    PRCNN_REQUIRE(counts && seg_off && segs && palette && rgb, "bev_compose: null pointer");
    const dim3 grid(ceil_div(width, BEV_TILE), ceil_div(height, BEV_TILE), n_images);
    hipLaunchKernelGGL(bev_compose_kernel, grid, dim3(BEV_THREADS), 0, (hipStream_t)stream, height, width, 4 * line_px, n_palette, counts,
                       seg_off, segs, palette, rgb);
    return check_launch("bev_compose");
}
