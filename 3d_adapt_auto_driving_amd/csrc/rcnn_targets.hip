// rcnn_targets.hip -- the RCNN stage's training targets (reference: lib/rpn/proposal_target_layer.py; rcnn_targets.py drives it).
//   prcnn_rcnn_assign     every RoI of every scene against the scene's ground truth (trailing zero-sum rows cut off, counted here): row
//                         maximum of the 3-D IoU and the first index that attains it, the RoI's list (fg / hard bg / easy bg / none),
//                         and the three ascending index lists with their sizes.  The M x G matrix is never written.
//   prcnn_rcnn_aug_rois   the noise tries of one scene's sampled RoIs.  The reference walks them as a chain (a RoI's try count decides
//                         where the next RoI's draws start).  Here: whether RoI k succeeds at stream position i depends on (k, i)
//                         alone, so that table is evaluated in parallel over the window k <= i <= T k + T - 1, and one wave then walks
//                         the RoIs in order (ballot over the next T positions, first set bit, advance).  A background RoI has one try at
//                         a position that is known once the foreground walk has ended.
//   prcnn_rcnn_targets    one pass over the pooled rows: rotation / scale / flip augmentation, canonical transformation, cls_label,
//                         reg_valid_mask, the split of the pooled row into sampled_pts and pts_feature.
// The 3-D IoU is iou3d_utils.boxes_iou3d_gpu's composition: rbox_overlap (rbox_iou.hpp) on the BEV boxes of boxes3d_to_bev_torch, times
// the clamped height overlap, over the clamped union; one f32 rounding per operation.
#include "common.hpp"
#include "gt_common.hpp"
#include "rbox_iou.hpp"
#include "scene_tiles.hpp"
#include <math.h>

namespace prcnn {

constexpr int RT_THREADS = 256;
constexpr int RT_MAX_ROIS = 128;                 // sampled RoIs per scene (prcnn_rcnn_max_rois)
constexpr int RT_MAX_TRIES = 64;                 // tries per RoI: one ballot of the walking wave
constexpr int RT_REC = 10;                       // floats per staged box: BEV x1 z1 x2 z2, cos, sin, y - h, y, volume, ry

// box [x, y, z, h, w, l, ry] -> record (boxes3d_to_bev_torch + the height interval and volume of boxes_iou3d_gpu)
__device__ __forceinline__ void rt_record(const float *bx, float *o)
{
    const float hl = bx[5] / 2, hw = bx[4] / 2;
    o[0] = bx[0] - hl; o[1] = bx[2] - hw; o[2] = bx[0] + hl; o[3] = bx[2] + hw;
    o[4] = cos_f32(bx[6]); o[5] = sin_f32(bx[6]);
    o[6] = bx[1] - bx[3]; o[7] = bx[1];
    o[8] = __fmul_rn(__fmul_rn(bx[3], bx[4]), bx[5]);
    o[9] = bx[6];
}

__device__ __forceinline__ RBox rt_rbox(const float *o)
{
    RBox r;
    r.v[0] = o[0]; r.v[1] = o[1]; r.v[2] = o[2]; r.v[3] = o[3]; r.v[4] = o[9];
    r.cosv = o[4]; r.sinv = o[5];
    return r;
}

// iou3d_utils.boxes_iou3d_gpu for one pair (a: the RoI, b: the ground truth)
__device__ inline float rt_iou3d(const float *a, const float *b)
{
    const float bev = rbox_overlap(rt_rbox(a), rt_rbox(b));
    const float oh = fmaxf(__fsub_rn(fminf(a[7], b[7]), fmaxf(a[6], b[6])), 0.f);
    const float o3 = __fmul_rn(bev, oh);
    return __fdiv_rn(o3, fmaxf(__fsub_rn(__fadd_rn(a[8], b[8]), o3), 1e-7f));
}

// ------------------------------------------------------------------------------------------------------------------ (a) assign
// grid (tiles of 64 RoIs / 4, scenes).  cls (b, m): 0 fg, 1 hard bg, 2 easy bg, 3 none.
__global__ void __launch_bounds__(RT_THREADS) rt_assign_kernel(int m, int g, int ntile, const float *__restrict__ rois,
                                                               const float *__restrict__ gt, float fg_thresh, float bg_thresh, float bg_lo,
                                                               float *__restrict__ max_ov, int *__restrict__ assign,
                                                               unsigned char *__restrict__ cls, int *__restrict__ tile_cnt,
                                                               int *__restrict__ sizes)
{
    __shared__ float sgt[GT_CHUNK * RT_REC];
    __shared__ int s_g;
    const int s = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const int tile = blockIdx.x * (RT_THREADS / WAVE) + threadIdx.x / WAVE;
    const int r = tile * WAVE + lane;
    const float *sg = gt + (long)s * g * 7;
    if (threadIdx.x == 0) s_g = 0;
    __syncthreads();
    // the rows that remain when the trailing rows whose sum is 0 are cut off (proposal_target_layer.py:98-101; the sum in row order)
    for (int k = threadIdx.x; k < g; k += RT_THREADS) {
        float sum = 0.f;
        for (int q = 0; q < 7; ++q) sum = __fadd_rn(sum, sg[7 * k + q]);
        if (sum != 0.f) atomicMax(&s_g, k + 1);
    }
    __syncthreads();
    const int gn = s_g;
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[4 * s + 3] = gn;
    float a[RT_REC];
    const bool valid = r < m;
    if (valid) rt_record(rois + ((long)s * m + r) * 7, a);
    float best = -INFINITY;
    int besti = 0;
    for (int k0 = 0; k0 < gn; k0 += GT_CHUNK) {
        const int kn = min(GT_CHUNK, gn - k0);
        __syncthreads();
        if ((int)threadIdx.x < kn) rt_record(sg + 7L * (k0 + threadIdx.x), sgt + threadIdx.x * RT_REC);
        __syncthreads();
        if (valid)
            for (int k = 0; k < kn; ++k) {
                const float v = rt_iou3d(a, sgt + k * RT_REC);
                if (v > best) { best = v; besti = k0 + k; }          // torch.max: the first index that attains the maximum
            }
    }
    if (gn == 0) best = 0.f;
    int c = 3;
    if (valid) {
        if (best >= fg_thresh) c = 0;
        else if (best < bg_lo) c = 2;
        else if (best < bg_thresh) c = 1;
        max_ov[(long)s * m + r] = best;
        assign[(long)s * m + r] = besti;
        cls[(long)s * m + r] = (unsigned char)c;
    }
    if (tile < ntile) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const unsigned long long bal = __ballot(valid && c == q);
            if (lane == 0) tile_cnt[((long)s * 3 + q) * ntile + tile] = __popcll(bal);
        }
    }
}

// one workgroup per scene: the ordered scan of the tile counts (scene_tiles.hpp), then every tile writes its part of the three lists
__global__ void __launch_bounds__(RT_THREADS) rt_lists_kernel(int m, int ntile, const unsigned char *__restrict__ cls,
                                                              int *__restrict__ tile_cnt, int *__restrict__ lists, int *__restrict__ sizes)
{
    __shared__ int wsum[RT_THREADS / WAVE];
    const int s = blockIdx.x, lane = threadIdx.x & (WAVE - 1);
    for (int q = 0; q < 3; ++q) {
        __syncthreads();
        const int tot = tile_exclusive_scan<RT_THREADS>(tile_cnt + ((long)s * 3 + q) * ntile, ntile, 1, wsum);
        if (threadIdx.x == 0) sizes[4 * s + q] = tot;
    }
    __syncthreads();
    for (int tile = threadIdx.x / WAVE; tile < ntile; tile += RT_THREADS / WAVE) {
        const int r = tile * WAVE + lane;
        const int c = r < m ? (int)cls[(long)s * m + r] : 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const unsigned long long bal = __ballot(c == q);
            const int pos = tile_cnt[((long)s * 3 + q) * ntile + tile] + __popcll(bal & ((1ull << lane) - 1ull));
            if (c == q && pos < m) lists[((long)s * 3 + q) * m + pos] = r;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- (b) tries
// random_aug_box3d ('multiple': range_config[level]; 'single') in f32 as torch evaluates it: python scalars rounded to f32
__device__ __forceinline__ void rt_noised(const float *roi, const float *nz, int method, float *o)
{
    float pr, hr, ar;
    if (method == 1) {                            // 'multiple'
        const int lv = min(max((int)nz[0], 0), 4);
        const float P[5] = {0.2f, 0.3f, 0.5f, 0.8f, 1.0f};
        const float H[5] = {0.1f, 0.15f, 0.15f, 0.15f, 0.15f};
        const float A[5] = {(float)(M_PI / 12), (float)(M_PI / 12), (float)(M_PI / 9), (float)(M_PI / 6), (float)(M_PI / 3)};
        pr = P[lv]; hr = H[lv]; ar = A[lv];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            o[q] = __fadd_rn(roi[q], __fmul_rn(__fdiv_rn(__fsub_rn(nz[1 + q], 0.5f), 0.5f), pr));
            o[3 + q] = __fmul_rn(roi[3 + q], __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(nz[4 + q], 0.5f), 0.5f), hr), 1.0f));
        }
        o[6] = __fadd_rn(roi[6], __fmul_rn(__fdiv_rn(__fsub_rn(nz[7], 0.5f), 0.5f), ar));
    } else {                                      // 'single'
        hr = (float)(0.5 / 0.15); ar = (float)(0.5 / (M_PI / 12));
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            o[q] = __fadd_rn(roi[q], __fsub_rn(nz[1 + q], 0.5f));
            o[3 + q] = __fmul_rn(roi[3 + q], __fadd_rn(__fdiv_rn(__fsub_rn(nz[4 + q], 0.5f), hr), 1.0f));
        }
        o[6] = __fadd_rn(roi[6], __fdiv_rn(__fsub_rn(nz[7], 0.5f), ar));
    }
}

__device__ __forceinline__ int rt_clamp(int v, int hi) { return min(max(v, 0), hi - 1); }

// the source RoI of sampled RoI k: pick (list, position) -> lists[list][position]
__device__ __forceinline__ int rt_source(const prcnn_rcnn_aug &p, int k)
{
    const int l = rt_clamp(p.pick[2 * k], 3), pos = rt_clamp(p.pick[2 * k + 1], p.m);
    return rt_clamp(p.lists[(long)l * p.m + pos], p.m);
}

// the box RoI (source row src) tries at stream position i, and its IoU with the RoI's ground truth
__device__ inline float rt_try(const prcnn_rcnn_aug &p, int src, int i, float *box)
{
    const float *roi = p.rois + 7L * src;
    if (p.keep[i]) {
#pragma unroll
        for (int q = 0; q < 7; ++q) box[q] = roi[q];
    } else {
        rt_noised(roi, p.noise + 8L * i, p.method, box);
    }
    float a[RT_REC], b[RT_REC];
    rt_record(box, a);
    rt_record(p.gt + 7L * rt_clamp(p.assign[src], p.g), b);
    return rt_iou3d(a, b);
}

// grid (positions / 256, foreground RoIs): table[k][i] for k <= i <= T k + T - 1
__global__ void __launch_bounds__(RT_THREADS) rt_table_kernel(prcnn_rcnn_aug p)
{
    const int k = blockIdx.y, i = blockIdx.x * RT_THREADS + threadIdx.x, T = p.fg_times;
    if (k >= p.n_fg || i >= p.n_pool || i < k || i > T * k + T - 1) return;
    float box[7];
    p.table[(long)k * p.n_pool + i] = rt_try(p, rt_source(p, k), i, box);
}

// one wave: the walk over the foreground RoIs, then every sampled RoI's outputs
__global__ void __launch_bounds__(WAVE) rt_walk_kernel(prcnn_rcnn_aug p)
{
    __shared__ int s_start[RT_MAX_ROIS], s_cnt[RT_MAX_ROIS];
    const int lane = threadIdx.x, T = p.fg_times;
    int at = 0;                                   // (uniform in the wave)
    for (int k = 0; k < p.n_fg; ++k) {
        const int i = at + lane;
        const bool hit = lane < T && i < p.n_pool && !(p.table[(long)k * p.n_pool + i] < p.pos_thresh);   // the loop ends when temp_iou < pos_thresh fails
        const unsigned long long bal = __ballot(hit);
        const int cnt = bal ? min(__ffsll((long long)bal), T) : T;
        if (lane == 0) { s_start[k] = at; s_cnt[k] = cnt; }
        at += cnt;
    }
    if (lane == 0) p.used[0] = at + (p.n_rois - p.n_fg) * p.bg_times;
    __syncthreads();
    const int W = max(max(p.fg_times, p.bg_times), 1);
    for (int k = lane; k < p.n_rois; k += WAVE) {
        const bool fg = k < p.n_fg;
        const int start = fg ? s_start[k] : at + (k - p.n_fg) * p.bg_times, cnt = fg ? s_cnt[k] : p.bg_times;
        const int src = rt_source(p, k);
        const float *roi = p.rois + 7L * src;
        float box[7], iou = p.max_ov[src], last = 0.f;
        int keep = 1;
#pragma unroll
        for (int q = 0; q < 7; ++q) box[q] = roi[q];
        for (int j = 0; j < W; ++j) p.out_tried[(long)k * W + j] = NAN;
        if (cnt > 0) {
            const int i = min(start + cnt - 1, p.n_pool - 1);
            for (int j = 0; j + 1 < cnt; ++j) p.out_tried[(long)k * W + j] = p.table[(long)k * p.n_pool + start + j];   // (foreground only)
            last = rt_try(p, src, i, box);
            p.out_tried[(long)k * W + cnt - 1] = last;
            keep = p.keep[i] ? 1 : 0;
            if (!keep) iou = last;                // cnt == 0 or keep: the source IoU
        }
        const float *gb = p.gt + 7L * rt_clamp(p.assign[src], p.g);
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            p.out_rois[7L * k + q] = box[q];
            p.out_gt[7L * k + q] = gb[q];
            float e = box[q];                     // kitti_utils.enlarge_box3d: h, w, l + 2 * extra, y + extra
            if (q >= 3 && q < 6) e = __fadd_rn(e, __fmul_rn(p.pool_extra_width, 2.0f));
            if (q == 1) e = __fadd_rn(e, p.pool_extra_width);
            p.out_pool_rois[7L * k + q] = e;
        }
        p.out_iou[k] = iou;
        p.out_src[k] = src; p.out_cnt[k] = cnt; p.out_keep[k] = keep;
    }
}

// ------------------------------------------------------------------------------------------------------------------ (c) targets
// rotate_pc_along_y_torch: [x z] <- [x z] R^T, R = [[cos, -sin], [sin, cos]]
__device__ __forceinline__ void rt_rot(float &x, float &z, float c, float s)
{
    const float nx = __fadd_rn(__fmul_rn(x, c), __fmul_rn(z, -s));
    const float nz = __fadd_rn(__fmul_rn(x, s), __fmul_rn(z, c));
    x = nx; z = nz;
}
__device__ __forceinline__ float rt_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

struct RtFrame {                                  // what one RoI's points go through
    float c1, s1, scale, flip;                    // augmentation: rotation, scale, flip sign
    float cx, cy, cz, c2, s2;                     // canonical: centre, rotation by the RoI's heading
};

__global__ void __launch_bounds__(RT_THREADS) rt_targets_kernel(prcnn_rcnn_target_args t)
{
    __shared__ RtFrame sf;
    const long row = blockIdx.x;
    if (threadIdx.x == 0) {
        float roi[7], gb[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { roi[q] = t.rois_in[7 * row + q]; gb[q] = t.gt_in[7 * row + q]; }
        RtFrame f;
        f.c1 = 1.f; f.s1 = 0.f; f.scale = 1.f; f.flip = 1.f;
        const float PI = (float)M_PI;
        if (t.aug_data) {
            // rotation; `rand - 0.5 / 0.5` is rand - 1 as the reference writes it
            const float ang = __fmul_rn(__fsub_rn(t.aug_rand[row], 1.0f), t.rot_scale);
            float beta = atan2f(gb[2], gb[0]);
            const float g_alpha = __fadd_rn(__fadd_rn(__fdiv_rn(__fmul_rn(-rt_sign(beta), PI), 2.f), beta), gb[6]);
            beta = atan2f(roi[2], roi[0]);
            const float r_alpha = __fadd_rn(__fadd_rn(__fdiv_rn(__fmul_rn(-rt_sign(beta), PI), 2.f), beta), roi[6]);
            f.c1 = cosf(ang); f.s1 = sinf(ang);
            rt_rot(gb[0], gb[2], f.c1, f.s1);
            rt_rot(roi[0], roi[2], f.c1, f.s1);
            // the heading from the alpha kept before the rotation.  The reference recomputes it for ALL scenes inside its per-scene
            // loop; only the value after the last iteration survives, and that one reads the final (rotated) centres alone.
            beta = atan2f(gb[2], gb[0]);
            gb[6] = __fsub_rn(__fadd_rn(__fdiv_rn(__fmul_rn(rt_sign(beta), PI), 2.f), g_alpha), beta);
            beta = atan2f(roi[2], roi[0]);
            roi[6] = __fsub_rn(__fadd_rn(__fdiv_rn(__fmul_rn(rt_sign(beta), PI), 2.f), r_alpha), beta);
            // scale
            f.scale = __fadd_rn(1.0f, __fmul_rn(__fdiv_rn(__fsub_rn(t.aug_rand[t.rows + row], 0.5f), 0.5f), 0.05f));
#pragma unroll
            for (int q = 0; q < 6; ++q) { gb[q] = __fmul_rn(gb[q], f.scale); roi[q] = __fmul_rn(roi[q], f.scale); }
            // flip: the multiplication by sign(rand - 0.5), literally
            f.flip = rt_sign(__fsub_rn(t.aug_rand[2 * t.rows + row], 0.5f));
            const float is_p = f.flip == 1.f ? 1.f : 0.f, is_n = f.flip == -1.f ? 1.f : 0.f;
            gb[0] = __fmul_rn(gb[0], f.flip);
            gb[6] = __fadd_rn(__fmul_rn(is_p, gb[6]), __fmul_rn(is_n, __fsub_rn(__fmul_rn(rt_sign(gb[6]), PI), gb[6])));
            roi[0] = __fmul_rn(roi[0], f.flip);
            roi[6] = __fadd_rn(__fmul_rn(is_p, roi[6]), __fmul_rn(is_n, __fsub_rn(__fmul_rn(rt_sign(roi[6]), PI), roi[6])));
        }
        // canonical transformation: roi_ry = ry % 2 pi (the sign of the divisor)
        const float TWO_PI = (float)(2 * M_PI);
        float ry = fmodf(roi[6], TWO_PI);
        if (ry != 0.f && ry < 0.f) ry = __fadd_rn(ry, TWO_PI);
        f.cx = roi[0]; f.cy = roi[1]; f.cz = roi[2];
        f.c2 = cosf(roi[6]); f.s2 = sinf(roi[6]);          // the points turn by ry, the target box by roi_ry
        gb[0] = __fsub_rn(gb[0], roi[0]); gb[1] = __fsub_rn(gb[1], roi[1]); gb[2] = __fsub_rn(gb[2], roi[2]);
        gb[6] = __fsub_rn(gb[6], ry);
        rt_rot(gb[0], gb[2], cosf(ry), sinf(ry));
#pragma unroll
        for (int q = 0; q < 7; ++q) { t.rois_out[7 * row + q] = roi[q]; t.gt_out[7 * row + q] = gb[q]; }
        const float iou = t.gt_iou[row];
        const bool valid = t.empty[row] == 0;
        t.reg_valid[row] = (iou > t.reg_fg && valid) ? 1 : 0;
        long long lab = iou > t.cls_fg ? 1 : 0;
        if (!valid) lab = -1;
        if (iou > t.cls_bg && iou < t.cls_fg) lab = -1;
        t.cls_label[row] = lab;
        sf = f;
    }
    __syncthreads();
    const RtFrame f = sf;
    const int cf = t.cin - 3;
    const float *in = t.pooled + row * t.s * t.cin;
    for (int q = threadIdx.x; q < t.s; q += RT_THREADS) {
        float x = in[(long)q * t.cin], y = in[(long)q * t.cin + 1], z = in[(long)q * t.cin + 2];
        if (t.aug_data) {
            rt_rot(x, z, f.c1, f.s1);
            x = __fmul_rn(x, f.scale); y = __fmul_rn(y, f.scale); z = __fmul_rn(z, f.scale);
            x = __fmul_rn(x, f.flip);
        }
        x = __fsub_rn(x, f.cx); y = __fsub_rn(y, f.cy); z = __fsub_rn(z, f.cz);
        rt_rot(x, z, f.c2, f.s2);
        float *o = t.sampled_pts + (row * t.s + q) * 3;
        o[0] = x; o[1] = y; o[2] = z;
    }
    float *fo = t.pts_feature + row * t.s * cf;
    for (long e = threadIdx.x; e < (long)t.s * cf; e += RT_THREADS) {
        const long q = e / cf, c = e - q * cf;
        fo[e] = in[q * t.cin + 3 + c];
    }
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_rcnn_max_rois(void) { return RT_MAX_ROIS; }
extern "C" int prcnn_rcnn_max_tries(void) { return RT_MAX_TRIES; }

extern "C" int prcnn_rcnn_assign(int b, int m, int g, const float *rois, const float *gt, float fg_thresh, float bg_thresh, float bg_lo,
                                 float *max_ov, int *assign, unsigned char *cls, int *tile_cnt, int *lists, int *sizes, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && m > 0 && g > 0, "rcnn_assign: bad shape b=%d m=%d g=%d", b, m, g);
    PRCNN_REQUIRE(b <= 65535 && (long long)b * m * 7 < (1LL << 31) && (long long)b * g * 7 < (1LL << 31), "rcnn_assign: batch too large");
    PRCNN_REQUIRE(rois && gt && max_ov && assign && cls && tile_cnt && lists && sizes, "rcnn_assign: null pointer");
    if (b == 0) return PRCNN_OK;
    const int ntile = (m + WAVE - 1) / WAVE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rt_assign_kernel, tile_grid(ntile, b, RT_THREADS), dim3(RT_THREADS), 0, st, m, g, ntile, rois, gt, fg_thresh, bg_thresh,
                       bg_lo, max_ov, assign, cls, tile_cnt, sizes);
    hipLaunchKernelGGL(rt_lists_kernel, dim3(b), dim3(RT_THREADS), 0, st, m, ntile, cls, tile_cnt, lists, sizes);
    return check_launch("rcnn_assign");
}

extern "C" int prcnn_rcnn_aug_rois(const prcnn_rcnn_aug *p, void *stream)
{
    PRCNN_REQUIRE(p, "rcnn_aug_rois: null pointer");
    PRCNN_REQUIRE(p->m > 0 && p->g > 0 && p->n_rois > 0 && p->n_rois <= RT_MAX_ROIS && p->n_fg >= 0 && p->n_fg <= p->n_rois,
                  "rcnn_aug_rois: bad shape m=%d g=%d rois=%d fg=%d (at most %d RoIs)", p->m, p->g, p->n_rois, p->n_fg, RT_MAX_ROIS);
    PRCNN_REQUIRE(p->fg_times >= 0 && p->fg_times <= RT_MAX_TRIES && (p->bg_times == 0 || p->bg_times == 1), "rcnn_aug_rois: bad try counts");
    PRCNN_REQUIRE(p->method == 0 || p->method == 1, "rcnn_aug_rois: method");
    PRCNN_REQUIRE(p->n_pool >= p->n_fg * p->fg_times + (p->n_rois - p->n_fg) * p->bg_times, "rcnn_aug_rois: the pools are too short");
    PRCNN_REQUIRE(p->rois && p->gt && p->max_ov && p->assign && p->lists && p->pick && p->out_rois && p->out_pool_rois && p->out_gt &&
                  p->out_iou && p->out_src && p->out_cnt && p->out_keep && p->out_tried && p->used, "rcnn_aug_rois: null pointer");
    PRCNN_REQUIRE(p->n_pool == 0 || (p->keep && p->noise && p->table), "rcnn_aug_rois: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (p->n_fg > 0 && p->fg_times > 0)
        hipLaunchKernelGGL(rt_table_kernel, dim3((unsigned)ceil_div(p->n_fg * p->fg_times, RT_THREADS), (unsigned)p->n_fg), dim3(RT_THREADS), 0, st, *p);
    hipLaunchKernelGGL(rt_walk_kernel, dim3(1), dim3(WAVE), 0, st, *p);
    return check_launch("rcnn_aug_rois");
}

extern "C" int prcnn_rcnn_targets(const prcnn_rcnn_target_args *t, void *stream)
{
    PRCNN_REQUIRE(t, "rcnn_targets: null pointer");
    PRCNN_REQUIRE(t->rows >= 0 && t->rows < (1 << 30) && t->s > 0 && t->cin >= 3, "rcnn_targets: bad shape rows=%d s=%d cin=%d", t->rows, t->s, t->cin);
    PRCNN_REQUIRE(t->pooled && t->empty && t->rois_in && t->gt_in && t->gt_iou && t->rois_out && t->gt_out && t->sampled_pts &&
                  t->cls_label && t->reg_valid && (t->cin == 3 || t->pts_feature) && (!t->aug_data || t->aug_rand), "rcnn_targets: null pointer");
    if (t->rows == 0) return PRCNN_OK;
    hipLaunchKernelGGL(rt_targets_kernel, dim3((unsigned)t->rows), dim3(RT_THREADS), 0, (hipStream_t)stream, *t);
    return check_launch("rcnn_targets");
}
