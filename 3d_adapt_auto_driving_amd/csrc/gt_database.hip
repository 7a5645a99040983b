// gt_database.hip -- per-object point extraction of the GT database (tools/generate_gt_database.py:59-87) for a batch of ragged
// scenes: every labelled box of a scene gets the rect-frame points (and intensities) that lie inside it, in point-index order.
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles, one wave per tile (tile_off); the boxes of all scenes
// sit back to back too (box_off).  Three passes, none of which stores the (boxes, points) flag matrix of the reference:
//   count   velo -> rect once per point (registers), then every box of the scene (LDS chunks of GT_CHUNK): one ballot + popcount
//           per (tile, box) -> bt_cnt;
//   scan    one workgroup per (box, scene): ordered exclusive scan of the box's tile counts in place, the total -> counts;
//   write   (after the host has turned the totals into row offsets) every lane recomputes its flag and stores
//           (x, y, z rect | intensity) at out_off[box] + bt_cnt[box][tile] + popcount(ballot below the lane).  A point inside two
//           boxes goes to both.
// Arithmetic (f32, -ffp-contract=off):
//   rect    kitti_io.Calibration.lidar_to_rect = np.dot([p 1], M), M = np.dot(V2C.T, R0.T) handed in by the host: product, two fused
//           multiply-adds, one add (the chain csrc/input_stage.hip spells out, pinned by tests/golden g11).  A scene of ONE point
//           is a (1, 4) . (4, 3) product, which numpy hands to OpenBLAS's gemv kernel: fma(x, m0, y * m1) + fma(z, m2, m3);
//   inside  roipool3d.cpp:82-95 as csrc/roipool_host.hip restates it: cy = bottom_y - h/2 (one rounding), the early reject at 10 m along
//           x / z and h/2 along y, the rotation with one rounding per product and per add, inclusive bounds.  h/2, w/2, l/2 are
//           formed in f32, which is exact (the reference forms them in double) for every size that is not subnormal.  cos / sin
//           come from the host (prcnn_gt_box_trig: the libm calls of the host path).
#include "common.hpp"
#include "gt_common.hpp"
#include "point_chains.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int GT_THREADS = 256;                  // 4 waves = 4 tiles per workgroup

// one coalesced 16-byte load per lane; rect = [p 1] . M with M (4, 3) row-major
__device__ __forceinline__ float4 gt_load_rect(const prcnn_gt_batch &b, const SceneTile &c)
{
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c.valid) {
        const float4 p = *(const float4 *)(b.velo + 4 * (c.p0 + c.idx));
        float v[3];
        lidar_to_rect_m(b.calib + 12 * c.s, p, c.n == 1, v);   // a (1, 4) . (4, 3) product is a gemv call: two pairs, then their sum
        r = make_float4(v[0], v[1], v[2], p.w);
    }
    return r;
}

// boxes [g0, g0 + nb) -> LDS records (all threads of the workgroup; barriers on both sides)
__device__ __forceinline__ void gt_stage_boxes(const prcnn_gt_batch &b, int g0, int nb, float *lds)
{
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += GT_THREADS) {
        const float *bx = b.boxes + 7L * (g0 + k);
        gt_box_record(bx, bx[3], b.trig[2L * (g0 + k)], b.trig[2L * (g0 + k) + 1], lds + k * GT_REC);
    }
    __syncthreads();
}

// ---- pass 1: counts per (box, tile)
__global__ __launch_bounds__(GT_THREADS) void gt_count_kernel(prcnn_gt_batch b)
{
    __shared__ float sbox[GT_CHUNK * GT_REC];
    SceneTile c;
    scene_tile<GT_THREADS>(b, blockIdx.y, c);
    const float4 r = gt_load_rect(b, c);
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    int *cnt = b.bt_cnt + b.bt_off[c.s] + c.tile;
    for (int k0 = 0; k0 < nb; k0 += GT_CHUNK) {
        const int kn = min(GT_CHUNK, nb - k0);
        gt_stage_boxes(b, bb + k0, kn, sbox);
        if (!c.live) continue;
        for (int k = 0; k < kn; ++k) {
            const unsigned long long m = __ballot(c.valid && gt_inside(sbox + k * GT_REC, r));
            if (c.lane == 0) cnt[(long)(k0 + k) * c.ntile] = __popcll(m);
        }
    }
}

// ---- pass 2: one workgroup per (box, scene): exclusive scan over the box's tiles in place, the total -> counts
__global__ __launch_bounds__(GT_THREADS) void gt_scan_kernel(prcnn_gt_batch b)
{
    __shared__ int wsum[GT_THREADS / WAVE];
    const int s = blockIdx.y, k = blockIdx.x;
    const int bb = b.box_off[s], nb = b.box_off[s + 1] - bb;
    if (k >= nb) return;
    const int nt = b.tile_off[s + 1] - b.tile_off[s];
    const int tot = tile_exclusive_scan<GT_THREADS>(b.bt_cnt + b.bt_off[s] + (long)k * nt, nt, 1, wsum);
    if (threadIdx.x == 0) b.counts[bb + k] = tot;
}

// ---- pass 3: the objects' rows
__global__ __launch_bounds__(GT_THREADS) void gt_write_kernel(prcnn_gt_batch b)
{
    __shared__ float sbox[GT_CHUNK * GT_REC];
    __shared__ long long sbase[GT_CHUNK + 1];
    SceneTile c;
    scene_tile<GT_THREADS>(b, blockIdx.y, c);
    const float4 r = gt_load_rect(b, c);
    const unsigned long long below = (1ull << c.lane) - 1ull;
    const int bb = b.box_off[c.s], nb = b.box_off[c.s + 1] - bb;
    const int *cnt = b.bt_cnt + b.bt_off[c.s] + c.tile;
    for (int k0 = 0; k0 < nb; k0 += GT_CHUNK) {
        const int kn = min(GT_CHUNK, nb - k0);
        gt_stage_boxes(b, bb + k0, kn, sbox);                 // its leading barrier also covers sbase's readers
        for (int k = threadIdx.x; k <= kn; k += GT_THREADS) sbase[k] = b.out_off[bb + k0 + k];
        __syncthreads();
        if (!c.live) continue;
        for (int k = 0; k < kn; ++k) {
            if (sbase[k + 1] == sbase[k]) continue;           // no point of the scene lies in this box
            const bool in = c.valid && gt_inside(sbox + k * GT_REC, r);
            const unsigned long long m = __ballot(in);
            if (!m) continue;
            if (in) {
                // the object's rows are [sbase[k], sbase[k + 1]): a row outside them would be a counting bug, never a write
                // into another object or past the buffer
                const long long pos = sbase[k] + cnt[(long)(k0 + k) * c.ntile] + __popcll(m & below);
                if (pos >= sbase[k] && pos < sbase[k + 1]) *(float4 *)(b.out + 4 * pos) = r;
            }
        }
    }
}

}  // namespace prcnn

using namespace prcnn;

static int gt_check(const prcnn_gt_batch *b, const char *what)
{
    PRCNN_REQUIRE(b, "%s: null pointer", what);
    PRCNN_REQUIRE(b->n_scenes >= 0 && b->max_tiles >= 0 && b->max_boxes >= 0, "%s: bad sizes", what);
    PRCNN_REQUIRE(b->n_scenes <= 65535 && b->max_boxes <= 65535, "%s: bad sizes (more than 65535 scenes, or boxes in a scene)", what);
    PRCNN_REQUIRE(b->pt_off && b->tile_off && b->box_off && b->bt_off && b->velo && b->calib && b->boxes && b->trig && b->bt_cnt &&
                      b->counts, "%s: null pointer", what);
    return PRCNN_OK;
}

extern "C" int prcnn_gt_box_chunk(void) { return GT_CHUNK; }

/* HOST: (cos ry, sin ry) of every box as the host path's point test evaluates them (csrc/roipool_host.hip point_in_box) */
extern "C" int prcnn_gt_box_trig(int n, const float *boxes3d, float *trig)
{
    PRCNN_REQUIRE(n >= 0, "gt_box_trig: bad sizes");
    if (n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(boxes3d && trig, "gt_box_trig: null pointer");
    for (int i = 0; i < n; ++i) {
        const float angle = boxes3d[7L * i + 6];
        trig[2L * i] = cosf(angle);
        trig[2L * i + 1] = sinf(angle);
    }
    return PRCNN_OK;
}

extern "C" int prcnn_gt_extract_count(const prcnn_gt_batch *b, void *stream)
{
    const int rc = gt_check(b, "gt_extract_count");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0 || b->max_boxes == 0 || b->max_tiles == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gt_count_kernel, tile_grid(b->max_tiles, b->n_scenes, GT_THREADS), dim3(GT_THREADS), 0, st, *b);
    hipLaunchKernelGGL(gt_scan_kernel, dim3(b->max_boxes, b->n_scenes), dim3(GT_THREADS), 0, st, *b);
    return check_launch("gt_extract_count");
}

extern "C" int prcnn_gt_extract_write(const prcnn_gt_batch *b, void *stream)
{
    const int rc = gt_check(b, "gt_extract_write");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0 || b->max_boxes == 0 || b->max_tiles == 0) return PRCNN_OK;
    PRCNN_REQUIRE(b->out_off && b->out, "gt_extract_write: null pointer");
    hipLaunchKernelGGL(gt_write_kernel, tile_grid(b->max_tiles, b->n_scenes, GT_THREADS), dim3(GT_THREADS), 0, (hipStream_t)stream, *b);
    return check_launch("gt_extract_write");
}
