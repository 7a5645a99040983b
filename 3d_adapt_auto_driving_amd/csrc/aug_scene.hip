// aug_scene.hip -- the geometric part of augmented-scene generation (tools/generate_aug_scene.py:150-234 aug_one_scene and the
// filter of :241-249) for a batch of ragged scenes and of jobs = (epoch, scene) pairs over them.  The random stream of the tool does
// not depend on any geometric result, so the host has replayed it: every job comes with the ordered list of at most PLACE_MAX_CAND
// database objects that reach the overlap test, already put on the scene's road plane (aug_scene.py).
//
// Points of all scenes sit back to back (pt_off), cut into 64-point tiles (tile_off; scene_tiles.hpp); the scenes' non-DontCare
// label boxes sit back to back too (box_off).  The database's points stay resident (db_pts / db_off).
//   filter   once per scene: velo -> rect -> image, valid flag (in the image, depth >= 0, inside PC_AREA_SCOPE) -> rect, valid;
//   place    one wave per job: every candidate against every label box of the scene (w + 0.5, l + 0.5; LDS chunks of GT_CHUNK) and
//            against every earlier candidate (w + 0.5, l + 0.5), all pairs in parallel; then the greedy accept in try order from the
//            ballots' conflict words (placement.hpp).  The candidate x box matrix is never stored;
//   count    per (job, tile): points that are valid and inside NO accepted box enlarged by h + 2 (one flag per point however many
//            enlargements hold it) -> tile_cnt;  scan: ordered exclusive scan per job, the total -> sizes;
//   write    (after the host has turned the sizes into row offsets) the kept points in point order, then every accepted object's
//            rows from the resident database with its y shift.  No atomics: every row's position is a prefix count.
// Arithmetic (-ffp-contract=off):
//   rect / image   point_chains.hpp (input_stage.hip's chains, g11); a scene of ONE point takes numpy's gemv forms (point_chains.hpp);
//   scope          the reference compares the f32 coordinates with a float64 array (70.4 is not an f32): compared in double here;
//   overlap        iou3d_utils.boxes_iou3d_gpu: BEV overlap of rbox_iou.hpp (new box first, as boxes_overlap_bev_gpu(a, b)) x
//                  clamp(min(y) - max(y - h), 0) / clamp(vol_a + vol_b - overlap, 1e-7), each operation rounded to f32 once;
//                  a candidate is placed when every such value is < 1e-8 (a NaN rejects, as np.max would);
//   inside         gt_common.hpp (g18) over [x, y, z, h + 2, w, l, ry] with the host's (cos ry, sin ry);
//   y shift        new_gt_points[:, 1] -= move_height with move_height a float64 scalar: f32(f64(y) - move_height) per point.
#include "common.hpp"
#include "gt_common.hpp"
#include "placement.hpp"
#include "point_chains.hpp"
#include "rbox_iou.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int AUG_THREADS = 256;                 // 4 waves = 4 tiles per workgroup
constexpr int AUG_SIZES = PLACE_MAX_CAND + 2;    // ints per job in sizes: kept points, accepted, the accepted slots in order
constexpr int AUG_REC = 9;                       // floats per staged overlap box: x1, z1, x2, z2, cos, sin, y - h, y, volume

// ---- filter: once per scene
__global__ __launch_bounds__(AUG_THREADS) void aug_filter_kernel(prcnn_aug_batch b)
{
    SceneTile c;
    scene_tile<AUG_THREADS>(b, blockIdx.y, c);
    if (!c.valid) return;
    const float4 p = *(const float4 *)(b.velo + 4 * (c.p0 + c.idx));
    float x, y, z;
    const bool ok = rect_valid_point(p, ((const SceneCalib *)b.calib)[c.s], c.n == 1, false, b.scope, x, y, z);
    *(float4 *)(b.rect + 4 * (c.p0 + c.idx)) = make_float4(x, y, z, p.w);
    b.valid[c.p0 + c.idx] = ok ? 1 : 0;
}

// ---- place
// box [x, y, z, h, w, l, ry] with w, l grown by `grow` (f32 additions, as cur_gt_boxes3d[:, 4:6] += 0.5) -> overlap record
__device__ __forceinline__ void aug_overlap_record(const float *bx, float grow, float *o)
{
    const float w = grow != 0.f ? __fadd_rn(bx[4], grow) : bx[4], l = grow != 0.f ? __fadd_rn(bx[5], grow) : bx[5];
    const float hl = __fmul_rn(l, 0.5f), hw = __fmul_rn(w, 0.5f);                 // kitti_utils.boxes3d_to_bev_torch
    o[0] = __fsub_rn(bx[0], hl); o[1] = __fsub_rn(bx[2], hw); o[2] = __fadd_rn(bx[0], hl); o[3] = __fadd_rn(bx[2], hw);
    o[4] = cos_f32(bx[6]); o[5] = sin_f32(bx[6]);                                 // make_rbox
    o[6] = __fsub_rn(bx[1], bx[3]); o[7] = bx[1];
    o[8] = __fmul_rn(__fmul_rn(bx[3], w), l);
}

__device__ __forceinline__ RBox aug_rbox(const float *o)
{
    RBox r;
    r.v[0] = o[0]; r.v[1] = o[1]; r.v[2] = o[2]; r.v[3] = o[3]; r.v[4] = 0.f;
    r.cosv = o[4]; r.sinv = o[5];
    return r;
}

// iou3d_utils.boxes_iou3d_gpu of (new box a, present box b); the clamps pass a NaN on, as torch.clamp does
__device__ __forceinline__ float aug_iou3d(const float *a, const float *b)
{
    const RBox A = aug_rbox(a), B = aug_rbox(b);
    const float bev = rbox_far_apart(A.v, B.v) ? 0.f : rbox_overlap(A, B);
    float oh = __fsub_rn(fminf(a[7], b[7]), fmaxf(a[6], b[6]));
    oh = oh < 0.f ? 0.f : oh;
    const float o3 = __fmul_rn(bev, oh);
    float den = __fsub_rn(__fadd_rn(a[8], b[8]), o3);
    den = den < 1e-7f ? 1e-7f : den;
    return __fdiv_rn(o3, den);
}

// a candidate is placed when every overlap value is < 1e-8 (a NaN rejects, as np.max would)
__device__ __forceinline__ bool aug_conflict(const float *a, const float *b) { return !(aug_iou3d(a, b) < 1e-8f); }

__global__ __launch_bounds__(WAVE) void aug_place_kernel(prcnn_aug_batch b)
{
    __shared__ float sorig[GT_CHUNK * AUG_REC];
    __shared__ float scand[PLACE_MAX_CAND * AUG_REC], sgrown[PLACE_MAX_CAND * AUG_REC];
    __shared__ unsigned srej;
    const int j = blockIdx.x, lane = threadIdx.x;
    const int s = b.job_scene[j];
    if (s < 0 || s >= b.n_scenes) return;            // (uniform in the workgroup) a job must name a scene of the batch
    const int nc = min(max(b.cand_n[j], 0), PLACE_MAX_CAND);
    if (lane < nc) {
        const float *bx = b.cand_box + 7L * ((long)PLACE_MAX_CAND * j + lane);
        aug_overlap_record(bx, 0.f, scand + lane * AUG_REC);
        aug_overlap_record(bx, 0.5f, sgrown + lane * AUG_REC);
    }
    // every candidate against the scene's label boxes (w + 0.5, l + 0.5), then against every earlier candidate, grown alike
    const int bb = b.box_off[s];
    const unsigned rej = place_reject_by_labels<float, AUG_REC, aug_conflict>(scand, nc, sorig, b.box_off[s + 1] - bb, &srej, [&](int k0, int kn) {
        for (int k = lane; k < kn; k += WAVE) aug_overlap_record(b.boxes + 7L * (bb + k0 + k), 0.5f, sorig + k * AUG_REC);
    });
    place_accept_greedy<float, AUG_REC, aug_conflict>(scand, sgrown, nc, rej, b.sizes + (long)AUG_SIZES * j + 2);
}

__device__ __forceinline__ bool aug_kept(const prcnn_aug_batch &b, const SceneTile &c, const float *lds, int na, float4 &r)
{
    r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!c.valid) return false;
    r = *(const float4 *)(b.rect + 4 * (c.p0 + c.idx));
    bool keep = b.valid[c.p0 + c.idx] != 0;
    for (int k = 0; k < na; ++k) keep = keep && !gt_inside(lds + k * GT_REC, r);
    return keep;
}

// ---- count: kept points per (job, tile)
__global__ __launch_bounds__(AUG_THREADS) void aug_count_kernel(prcnn_aug_batch b)
{
    __shared__ float sbox[PLACE_MAX_CAND * GT_REC];
    const int j = blockIdx.y;
    if (b.job_scene[j] < 0 || b.job_scene[j] >= b.n_scenes) return;
    SceneTile c;
    scene_tile<AUG_THREADS>(b, b.job_scene[j], c);
    const int na = stage_accepted(b.sizes + (long)AUG_SIZES * j + 2, (long)PLACE_MAX_CAND * j, b.cand_box, b.cand_trig, sbox);
    if (!c.live) return;
    float4 r;
    const unsigned long long m = __ballot(aug_kept(b, c, sbox, na, r));
    if (c.lane == 0) b.tile_cnt[b.jt_off[j] + c.tile] = __popcll(m);
}

// ---- scan: one workgroup per job: exclusive scan over the job's tiles in place, the total -> sizes[0]
__global__ __launch_bounds__(AUG_THREADS) void aug_scan_kernel(prcnn_aug_batch b)
{
    __shared__ int wsum[AUG_THREADS / WAVE];
    const int j = blockIdx.x, s = b.job_scene[j];
    if (s < 0 || s >= b.n_scenes) return;
    const int tot = tile_exclusive_scan<AUG_THREADS>(b.tile_cnt + b.jt_off[j], b.tile_off[s + 1] - b.tile_off[s], 1, wsum);
    if (threadIdx.x == 0) b.sizes[(long)AUG_SIZES * j] = tot;
}

// ---- write: the kept points' rows
__global__ __launch_bounds__(AUG_THREADS) void aug_write_kernel(prcnn_aug_batch b)
{
    __shared__ float sbox[PLACE_MAX_CAND * GT_REC];
    const int j = blockIdx.y;
    if (b.job_scene[j] < 0 || b.job_scene[j] >= b.n_scenes) return;
    SceneTile c;
    scene_tile<AUG_THREADS>(b, b.job_scene[j], c);
    const int na = stage_accepted(b.sizes + (long)AUG_SIZES * j + 2, (long)PLACE_MAX_CAND * j, b.cand_box, b.cand_trig, sbox);
    if (!c.live) return;
    float4 r;
    const bool keep = aug_kept(b, c, sbox, na, r);
    const unsigned long long m = __ballot(keep);
    if (!keep) return;
    // the job's kept rows are [base, base + sizes[0]) inside [out_off[j], out_off[j + 1]): a row outside them would be a counting bug,
    // never a write into another job or past the buffer
    const long long base = b.out_off[j], end = min(base + (long long)b.sizes[(long)AUG_SIZES * j], b.out_off[j + 1]);
    const long long pos = base + b.tile_cnt[b.jt_off[j] + c.tile] + __popcll(m & ((1ull << c.lane) - 1ull));
    if (pos >= base && pos < end) *(float4 *)(b.out + 4 * pos) = r;
}

// ---- write: the accepted objects' rows, gathered from the resident database, y -> f32(f64(y) - move_height)
__global__ __launch_bounds__(AUG_THREADS) void aug_objects_kernel(prcnn_aug_batch b)
{
    const int j = blockIdx.z, k = blockIdx.y;
    const int *sizes = b.sizes + (long)AUG_SIZES * j;
    if (k >= min(max(sizes[1], 0), PLACE_MAX_CAND)) return;
    const int slot = sizes[2 + k];
    if (slot < 0 || slot >= PLACE_MAX_CAND) return;
    const long q = (long)PLACE_MAX_CAND * j + slot;
    const int e = b.cand_db[q];
    if (e < 0 || e >= b.n_db) return;
    const long long src = b.db_off[e], n = b.db_off[e + 1] - src;
    const long long base = b.obj_off[(long)(PLACE_MAX_CAND + 1) * j + k];
    const long long end = min(b.obj_off[(long)(PLACE_MAX_CAND + 1) * j + k + 1], b.out_off[j + 1]);
    const double move = b.cand_move[q];
    for (long long i = (long long)blockIdx.x * AUG_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * AUG_THREADS) {
        float4 p = *(const float4 *)(b.db_pts + 4 * (src + i));
        p.y = __double2float_rn(__dsub_rn((double)p.y, move));
        const long long pos = base + i;
        if (pos >= b.out_off[j] && pos < end) *(float4 *)(b.out + 4 * pos) = p;
    }
}

}  // namespace prcnn

using namespace prcnn;

static int aug_check(const prcnn_aug_batch *b, const char *what)
{
    PRCNN_REQUIRE(b, "%s: null pointer", what);
    PRCNN_REQUIRE(b->n_scenes >= 0 && b->n_jobs >= 0 && b->max_tiles >= 0 && b->n_db >= 0, "%s: bad sizes", what);
    PRCNN_REQUIRE(b->n_scenes <= 65535 && b->n_jobs <= 65535, "%s: bad sizes (more than 65535 scenes or jobs)", what);
    if (b->n_scenes == 0 || b->n_jobs == 0) return PRCNN_OK;
    PRCNN_REQUIRE(b->pt_off && b->tile_off && b->box_off && b->calib && b->scope && b->job_scene && b->jt_off && b->cand_n && b->cand_db &&
                      b->cand_box && b->cand_trig && b->cand_move && b->sizes && b->db_off && b->boxes,
                  "%s: null pointer", what);
    PRCNN_REQUIRE(b->max_tiles == 0 || (b->velo && b->rect && b->valid && b->tile_cnt), "%s: null pointer", what);
    return PRCNN_OK;
}

extern "C" int prcnn_aug_max_candidates(void) { return PLACE_MAX_CAND; }

extern "C" int prcnn_aug_place(const prcnn_aug_batch *b, void *stream)
{
    const int rc = aug_check(b, "aug_place");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0 || b->n_jobs == 0) return PRCNN_OK;
    PRCNN_REQUIRE(sizeof(SceneCalib) == PRCNN_CALIB_ROW * sizeof(float), "aug_place: calib layout");
    hipStream_t st = (hipStream_t)stream;
    if (b->max_tiles > 0) hipLaunchKernelGGL(aug_filter_kernel, tile_grid(b->max_tiles, b->n_scenes, AUG_THREADS), dim3(AUG_THREADS), 0, st, *b);
    hipLaunchKernelGGL(aug_place_kernel, dim3(b->n_jobs), dim3(WAVE), 0, st, *b);
    if (b->max_tiles > 0) hipLaunchKernelGGL(aug_count_kernel, tile_grid(b->max_tiles, b->n_jobs, AUG_THREADS), dim3(AUG_THREADS), 0, st, *b);
    hipLaunchKernelGGL(aug_scan_kernel, dim3(b->n_jobs), dim3(AUG_THREADS), 0, st, *b);
    return check_launch("aug_place");
}

extern "C" int prcnn_aug_write(const prcnn_aug_batch *b, void *stream)
{
    const int rc = aug_check(b, "aug_write");
    if (rc != PRCNN_OK) return rc;
    if (b->n_scenes == 0 || b->n_jobs == 0) return PRCNN_OK;
    PRCNN_REQUIRE(b->out_off && b->obj_off && b->out, "aug_write: null pointer");
    PRCNN_REQUIRE(b->n_db == 0 || b->db_pts, "aug_write: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (b->max_tiles > 0) hipLaunchKernelGGL(aug_write_kernel, tile_grid(b->max_tiles, b->n_jobs, AUG_THREADS), dim3(AUG_THREADS), 0, st, *b);
    if (b->n_db > 0) hipLaunchKernelGGL(aug_objects_kernel, dim3(4, PLACE_MAX_CAND, b->n_jobs), dim3(AUG_THREADS), 0, st, *b);
    return check_launch("aug_write");
}
