// train_input.hip -- the RPN training input stage (lib/datasets/kitti_rcnn_dataset.py:249-382 get_rpn_sample in TRAIN mode, with
// apply_gt_aug_to_one_scene :428-531 and data_augmentation :533-591) for a batch of ragged scenes.  No draw of the loader depends on
// a geometric result except through a few counts, so the host owns the random stream (train_input.py): it hands every scene the
// ordered list of at most PLACE_MAX_CAND database objects that reach the overlap test, and, after one round trip of a few ints per
// scene, the sampler's choice as ranks.
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles (tile_off; scene_tiles.hpp); the label boxes' overlap
// records sit back to back too (box_off).  The database's points stay resident (db_pts).
//   place   filter   velo -> rect -> image, valid flag (point_chains.hpp, as aug_scene.hip; a scene read from rectified_data is rect
//                    already);
//           place    one wave per scene: every candidate against every label box (LDS chunks of GT_CHUNK) and against every earlier
//                    candidate under the ONLINE rule (kitti_utils.get_iou3d), all pairs in parallel, then the greedy accept in try
//                    order from the ballots' conflict words (placement.hpp).  The candidate x box matrix is never stored;
//           count    one flag byte per point: bit 0 kept (valid and inside no accepted box enlarged by h + 2), bit 1 near (z < 40);
//                    per tile the kept and the near counts;  scan: ordered exclusive scans per scene, the totals -> sizes;
//           compact  the kept / near / far points' indices in point order (every position is a prefix count: no atomics);
//   emit    one thread per output row: its code names a rank in one of the three lists or a row of the resident database (with the
//           object's y shift), then rotation, scale, flip -> pts_rect, pts_input, pts_features.
// Arithmetic (-ffp-contract=off):
//   overlap   get_iou3d works on the f32 corner arrays of boxes3d_to_corners3d; the host makes them with numpy (a handful of boxes) and
//             passes every box as a record of PRCNN_TR_REC doubles: the four BEV corners x, z, min_h, max_h (the f32 corner means) and its f32 volume
//             term.  The polygon intersection is a Sutherland-Hodgman clip in f64, operation by operation as train_input.py's
//             quad_intersection_area; h_overlap is an f32 difference; iou = f32(o3 / ((f32 vol_a + vol_b) - o3)); a candidate is placed
//             when every value is < 1e-8 (a NaN rejects, as np.max would);
//   inside    gt_common.hpp (g18) over [x, y, z, h + 2, w, l, ry] with the host's (cos ry, sin ry);
//   y shift   f32(f64(y) - move_height), as aug_scene.hip;
//   rotation  np.dot(pc[:, [0, 2]] as f64, rotmat.T): first term a plain product, the second fused, rounded to f32 once;
//   scale     f32 product with the f32-rounded scale; flip: x negated; intensity - 0.5 in f32.
#include "common.hpp"
#include "gt_common.hpp"
#include "placement.hpp"
#include "point_chains.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int TR_THREADS = 256;                  // 4 waves = 4 tiles per workgroup
constexpr int TR_SIZES = PLACE_MAX_CAND + 3;     // ints per scene in sizes: kept, near kept, accepted, the accepted slots in order

// ---- filter
__global__ __launch_bounds__(TR_THREADS) void train_filter_kernel(prcnn_train_batch b)
{
    SceneTile c;
    scene_tile<TR_THREADS>(b, b.scene_begin + blockIdx.y, c);
    if (!c.valid) return;
    const float4 p = *(const float4 *)(b.velo + 4 * (c.p0 + c.idx));
    float x, y, z;
    const bool ok = rect_valid_point(p, ((const SceneCalib *)b.calib)[c.s], c.n == 1, b.is_rect[c.s] != 0,
                                     b.reduce_by_range ? b.scope : nullptr, x, y, z);
    *(float4 *)(b.rect + 4 * (c.p0 + c.idx)) = make_float4(x, y, z, p.w);
    b.valid[c.p0 + c.idx] = ok ? 1 : 0;
}

// ---- place
// area of the intersection of two convex quadrilaterals (x, z corner pairs in ring order): the first clipped by the four edges of the
// second; train_input.py quad_intersection_area is the same operations in the same order
__device__ double tr_quad_clip_area(const double *A, const double *B)
{
    double px[9], pz[9], qx[9], qz[9];
    int n = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) { px[i] = A[2 * i]; pz[i] = A[2 * i + 1]; }
    double sb = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        sb = __dadd_rn(sb, __dsub_rn(__dmul_rn(B[2 * i], B[2 * j + 1]), __dmul_rn(B[2 * j], B[2 * i + 1])));
    }
    const double sign = sb >= 0.0 ? 1.0 : -1.0;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const int f = (e + 1) & 3;
        const double ax = B[2 * e], az = B[2 * e + 1];
        const double ex = __dsub_rn(B[2 * f], ax), ez = __dsub_rn(B[2 * f + 1], az);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int k = i + 1 == n ? 0 : i + 1;
            const double cx = px[i], cz = pz[i], nx = px[k], nz = pz[k];
            const double dc = __dmul_rn(sign, __dsub_rn(__dmul_rn(ex, __dsub_rn(cz, az)), __dmul_rn(ez, __dsub_rn(cx, ax))));
            const double dn = __dmul_rn(sign, __dsub_rn(__dmul_rn(ex, __dsub_rn(nz, az)), __dmul_rn(ez, __dsub_rn(nx, ax))));
            const bool ic = dc >= 0.0, in = dn >= 0.0;
            if (ic && m < 9) { qx[m] = cx; qz[m] = cz; ++m; }
            if (ic != in && m < 9) {
                const double t = __ddiv_rn(dc, __dsub_rn(dc, dn));
                qx[m] = __dadd_rn(cx, __dmul_rn(t, __dsub_rn(nx, cx)));
                qz[m] = __dadd_rn(cz, __dmul_rn(t, __dsub_rn(nz, cz)));
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) { px[i] = qx[i]; pz[i] = qz[i]; }
    }
    if (n < 3) return 0.0;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const int k = i + 1 == n ? 0 : i + 1;
        s = __dadd_rn(s, __dsub_rn(__dmul_rn(px[i], pz[k]), __dmul_rn(px[k], pz[i])));
    }
    return __dmul_rn(0.5, fabs(s));
}

// kitti_utils.get_iou3d of (new box a, present box b) -> true when the pair does NOT allow the placement
__device__ __forceinline__ bool tr_conflict(const double *a, const double *b)
{
    const float max_of_min = fmaxf((float)a[8], (float)b[8]), min_of_max = fminf((float)a[9], (float)b[9]);
    const float hov = __fsub_rn(min_of_max, max_of_min);
    if (hov <= 0.f) return false;                                   // h_overlap == 0: the entry stays 0
    const double o3 = __dmul_rn(tr_quad_clip_area(a, b), (double)hov);
    const double un = __dsub_rn((double)__fadd_rn((float)a[10], (float)b[10]), o3);
    const float iou = __double2float_rn(__ddiv_rn(o3, un));
    return !((double)iou < 1e-8);
}

__global__ __launch_bounds__(WAVE) void train_place_kernel(prcnn_train_batch b)
{
    __shared__ double sorig[GT_CHUNK * PRCNN_TR_REC];
    __shared__ double scand[PLACE_MAX_CAND * PRCNN_TR_REC];
    __shared__ unsigned srej;
    const int s = b.scene_begin + blockIdx.x, lane = threadIdx.x;
    const int nc = min(max(b.cand_n[s], 0), PLACE_MAX_CAND);
    for (int p = lane; p < nc * PRCNN_TR_REC; p += WAVE) scand[p] = b.cand_rec[(long)PLACE_MAX_CAND * PRCNN_TR_REC * s + p];
    // every candidate against the scene's label boxes, then against every earlier candidate (the records come enlarged)
    const int bb = b.box_off[s];
    const unsigned rej = place_reject_by_labels<double, PRCNN_TR_REC, tr_conflict>(scand, nc, sorig, b.box_off[s + 1] - bb, &srej, [&](int k0, int kn) {
        for (int p = lane; p < kn * PRCNN_TR_REC; p += WAVE) sorig[p] = b.box_rec[(long)PRCNN_TR_REC * (bb + k0) + p];
    });
    place_accept_greedy<double, PRCNN_TR_REC, tr_conflict>(scand, scand, nc, rej, b.sizes + (long)TR_SIZES * s + 3);
}

// ---- count: the flag byte of every point, the kept and near counts per tile
__global__ __launch_bounds__(TR_THREADS) void train_count_kernel(prcnn_train_batch b)
{
    __shared__ float sbox[PLACE_MAX_CAND * GT_REC];
    const int s = b.scene_begin + blockIdx.y;
    SceneTile c;
    scene_tile<TR_THREADS>(b, s, c);
    const int na = stage_accepted(b.sizes + (long)TR_SIZES * s + 3, (long)PLACE_MAX_CAND * s, b.cand_box, b.cand_trig, sbox);
    if (!c.live) return;
    bool keep = false, near = false;
    if (c.valid) {
        const float4 r = *(const float4 *)(b.rect + 4 * (c.p0 + c.idx));
        keep = b.valid[c.p0 + c.idx] != 0;
        for (int k = 0; k < na; ++k) keep = keep && !gt_inside(sbox + k * GT_REC, r);
        near = keep && r.z < 40.0f;
        b.flag[c.p0 + c.idx] = (unsigned char)((keep ? 1 : 0) | (near ? 2 : 0));
    }
    const unsigned long long mk = __ballot(keep), mn = __ballot(near);
    if (c.lane == 0) {
        const long t = 2L * (b.tile_off[s] + c.tile);
        b.tile_cnt[t] = __popcll(mk);
        b.tile_cnt[t + 1] = __popcll(mn);
    }
}

// ---- scan: one workgroup per scene: exclusive scans over the scene's tiles in place (kept, then near), the totals -> sizes[0..1]
__global__ __launch_bounds__(TR_THREADS) void train_scan_kernel(prcnn_train_batch b)
{
    __shared__ int wsum[TR_THREADS / WAVE];
    const int s = b.scene_begin + blockIdx.x;
    const int nt = b.tile_off[s + 1] - b.tile_off[s];
    for (int which = 0; which < 2; ++which) {
        const int tot = tile_exclusive_scan<TR_THREADS>(b.tile_cnt + 2L * b.tile_off[s] + which, nt, 2, wsum);
        if (threadIdx.x == 0) b.sizes[(long)TR_SIZES * s + which] = tot;
        __syncthreads();                                               // wsum is read to the end of a scan and written by the next
    }
}

// ---- compact: the kept / near / far points' indices in point order -> lists (3, sum n)
__global__ __launch_bounds__(TR_THREADS) void train_compact_kernel(prcnn_train_batch b)
{
    const int s = b.scene_begin + blockIdx.y;
    SceneTile c;
    scene_tile<TR_THREADS>(b, s, c);
    if (!c.live) return;
    const unsigned f = c.valid ? b.flag[c.p0 + c.idx] : 0u;
    const bool keep = f & 1u, near = f & 2u;
    const unsigned long long mk = __ballot(keep), mn = __ballot(near);
    if (!keep) return;
    const unsigned long long below = (1ull << c.lane) - 1ull;
    const long t = 2L * (b.tile_off[s] + c.tile);
    const int rk = b.tile_cnt[t] + __popcll(mk & below), rn = b.tile_cnt[t + 1] + __popcll(mn & below);
    const long total = b.pt_off[b.n_scenes];
    // a rank is a prefix count, so it is below the scene's size: a rank outside it would be a counting bug, never a write elsewhere
    if (rk >= 0 && rk < c.n) b.lists[c.p0 + rk] = c.idx;
    const int r = near ? rn : rk - rn;
    if (r >= 0 && r < c.n) b.lists[(near ? 1 : 2) * total + c.p0 + r] = c.idx;
}

// ---- emit
__global__ __launch_bounds__(TR_THREADS) void train_emit_kernel(prcnn_train_batch b)
{
    const long long row = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (row >= (long long)b.n_scenes * b.npoints) return;
    const int s = (int)(row / b.npoints);
    const long long code = b.codes[row];
    const int kind = (int)((code >> PRCNN_TR_KIND_SHIFT) & 0xff), slot = (int)((code >> PRCNN_TR_SLOT_SHIFT) & 0xff);
    const long long val = code & ((1LL << PRCNN_TR_SLOT_SHIFT) - 1);
    const long p0 = b.pt_off[s], n = b.pt_off[s + 1] - p0, total = b.pt_off[b.n_scenes];
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);                    // a code that names nothing readable stays a zero row
    if (kind <= PRCNN_TR_FAR) {                                    // PRCNN_TR_KEPT / NEAR / FAR: the list's index
        if (val < n) {
            const int idx = b.lists[kind * total + p0 + val];
            if (idx >= 0 && idx < n) p = *(const float4 *)(b.rect + 4 * (p0 + idx));
        }
    } else if (kind == PRCNN_TR_DB && val < b.n_db_rows && slot < PLACE_MAX_CAND) {
        p = *(const float4 *)(b.db_pts + 4 * val);
        p.y = __double2float_rn(__dsub_rn((double)p.y, b.cand_move[(long)PLACE_MAX_CAND * s + slot]));
    }
    const double *g = b.aug + 6L * s;                              // m00, m10, m01, m11, scale, flags (1 rotation, 2 scaling, 4 flip)
    const int flags = (int)g[5];
    float x = p.x, y = p.y, z = p.z;
    if (flags & 1) {
        const double dx = (double)x, dz = (double)z;
        x = __double2float_rn(__fma_rn(dz, g[1], __dmul_rn(dx, g[0])));
        z = __double2float_rn(__fma_rn(dz, g[3], __dmul_rn(dx, g[2])));
    }
    if (flags & 2) {
        const float sc = (float)g[4];
        x = __fmul_rn(x, sc); y = __fmul_rn(y, sc); z = __fmul_rn(z, sc);
    }
    if (flags & 4) x = -x;
    const float feat = __fsub_rn(p.w, 0.5f);
    float *pr = b.pts_rect + 3 * row;
    pr[0] = x; pr[1] = y; pr[2] = z;
    b.pts_features[row] = feat;
    float *pi = b.pts_input + (long long)b.input_channels * row;
    pi[0] = x; pi[1] = y; pi[2] = z;
    if (b.input_channels == 4) pi[3] = feat;
}

}  // namespace prcnn

using namespace prcnn;

static int train_check(const prcnn_train_batch *b, const char *what)
{
    PRCNN_REQUIRE(b, "%s: null pointer", what);
    PRCNN_REQUIRE(b->n_scenes >= 0 && b->max_tiles >= 0 && b->n_db_rows >= 0 && b->npoints >= 0, "%s: bad sizes", what);
    PRCNN_REQUIRE(b->n_scenes <= 65535, "%s: bad sizes (more than 65535 scenes)", what);
    PRCNN_REQUIRE(b->input_channels == 3 || b->input_channels == 4, "%s: input_channels must be 3 or 4", what);
    if (b->n_scenes == 0) return PRCNN_OK;
    PRCNN_REQUIRE(b->pt_off && b->tile_off && b->box_off && b->calib && b->scope && b->is_rect && b->box_rec && b->cand_n && b->cand_rec &&
                      b->cand_box && b->cand_trig && b->cand_move && b->sizes,
                  "%s: null pointer", what);
    PRCNN_REQUIRE(b->max_tiles == 0 || (b->velo && b->rect && b->valid && b->flag && b->tile_cnt && b->lists), "%s: null pointer", what);
    return PRCNN_OK;
}

extern "C" int prcnn_train_place(const prcnn_train_batch *b, void *stream)
{
    const int rc = train_check(b, "train_place");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0) return PRCNN_OK;
    PRCNN_REQUIRE(sizeof(SceneCalib) == PRCNN_CALIB_ROW * sizeof(float), "train_place: calib layout");
    PRCNN_REQUIRE(0 <= b->scene_begin && b->scene_begin <= b->scene_end && b->scene_end <= b->n_scenes, "train_place: bad scene range");
    const int ns = b->scene_end - b->scene_begin;
    if (ns == 0) return PRCNN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (b->max_tiles > 0) hipLaunchKernelGGL(train_filter_kernel, tile_grid(b->max_tiles, ns, TR_THREADS), dim3(TR_THREADS), 0, st, *b);
    hipLaunchKernelGGL(train_place_kernel, dim3(ns), dim3(WAVE), 0, st, *b);
    if (b->max_tiles > 0) hipLaunchKernelGGL(train_count_kernel, tile_grid(b->max_tiles, ns, TR_THREADS), dim3(TR_THREADS), 0, st, *b);
    hipLaunchKernelGGL(train_scan_kernel, dim3(ns), dim3(TR_THREADS), 0, st, *b);
    if (b->max_tiles > 0) hipLaunchKernelGGL(train_compact_kernel, tile_grid(b->max_tiles, ns, TR_THREADS), dim3(TR_THREADS), 0, st, *b);
    return check_launch("train_place");
}

extern "C" int prcnn_train_emit(const prcnn_train_batch *b, void *stream)
{
    const int rc = train_check(b, "train_emit");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0 || b->npoints == 0) return PRCNN_OK;
    PRCNN_REQUIRE(b->codes && b->aug && b->pts_rect && b->pts_input && b->pts_features, "train_emit: null pointer");
    PRCNN_REQUIRE(b->n_db_rows == 0 || b->db_pts, "train_emit: null pointer");
    PRCNN_REQUIRE(b->max_tiles > 0 || b->n_db_rows > 0, "train_emit: nothing to read rows from");
    const long long rows = (long long)b->n_scenes * b->npoints;
    PRCNN_REQUIRE((rows + TR_THREADS - 1) / TR_THREADS < (1LL << 31), "train_emit: too many rows: split the batch");
    hipLaunchKernelGGL(train_emit_kernel, dim3((unsigned)((rows + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, (hipStream_t)stream, *b);
    return check_launch("train_emit");
}
