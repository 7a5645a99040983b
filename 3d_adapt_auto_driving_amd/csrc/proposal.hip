// proposal.hip -- the RPN proposal layer in five steps (counterpart of
// pointrcnn/lib/rpn/proposal_layer.py:15-119 with decode_bbox_target of lib/utils/bbox_transform.py:24-121), and the per-point RCNN
// inputs (prcnn_point_aux).
//
// The reference does this per scene in Python: ~25 elementwise torch kernels for the decode, a sort,
// boolean-mask selections with two device->host syncs, and two NMS calls with host round trips; the
// batched torch formulation in net/proposal_layer.py still needs ~90 short launches.  Here:
//   1. rpn_decode_kernel     one lane per point: arg-max of the x / z / heading bins, residuals, box (same f32 operation order as the
//                            torch expression, no fma); not for boxes the RPN tail decoded already (prcnn_rpn_proposals_boxes)
//   2. score_order           (score_sort.hip) a scene's points by (score desc, index asc): one launch, or chunk sorts + merge rounds
//   3. band_select_kernel    one workgroup per scene: ordered compaction (wave ballot + LDS prefix) of the
//                            sorted proposals into the (0,40] m and (40,80] m tables, top 70 % / 30 % of
//                            RPN_PRE_NMS_TOP_N, with the reference's "no far points" fallback
//   4. nms_device            (nms_device.hip) all 2*B problems in one launch, stops at the post-NMS quota (rotated: nms_lazy_kernel;
//                            axis-aligned: nms_quota_kernel with a 256- or 512-row kept-box table)
//   5. assemble_rois_kernel  near keeps, then far keeps, zero padded -> rois (B, M, 7), scores (B, M); M <= 512
// No host synchronisation anywhere.
#include "nms_blocks.hpp"
#include "rpn_decode.hpp"
#include "score_sort.hpp"

namespace prcnn {

struct DecodeCfg {
    float loc_scope, loc_bin_size;
    int nbin;          // per_loc_bin_num = 2 * int(loc_scope / loc_bin_size)
    int num_head_bin;
    int xz_fine;
    float anchor[3];
    int channels;
};

// decode_bbox_target(xyz (N,3), reg, get_xz_fine, get_y_by_bin=False, get_ry_fine=False), then
// proposals[:, 1] += proposals[:, 3] / 2 (proposal_layer.py:31)
__global__ __launch_bounds__(256) void rpn_decode_kernel(long total, DecodeCfg c, const float *__restrict__ xyz,
                                                         const float *__restrict__ reg, float *__restrict__ boxes)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float *r = reg + i * c.channels;
    const float *p = xyz + i * 3;
    const int nb = c.nbin;
    const int xb = argmax_row(r, nb), zb = argmax_row(r + nb, nb);
    float px = rd_bin_centre(xb, c.loc_bin_size, c.loc_scope);
    float pz = rd_bin_centre(zb, c.loc_bin_size, c.loc_scope);
    int cur = 2 * nb;
    if (c.xz_fine) {
        px = rd_add_residual(px, r[2 * nb + xb], c.loc_bin_size);
        pz = rd_add_residual(pz, r[3 * nb + zb], c.loc_bin_size);
        cur = 4 * nb;
    }
    float py = __fadd_rn(p[1], r[cur]);
    cur += 1;
    const int rb = argmax_row(r + cur, c.num_head_bin);
    const float res_norm = r[cur + c.num_head_bin + rb];
    const float apc = (float)((2.0 * M_PI) / c.num_head_bin);            // python double -> f32 scalar
    const float apc_half = (float)(((2.0 * M_PI) / c.num_head_bin) / 2.0);
    const float two_pi = (float)(2.0 * M_PI), pi = (float)M_PI;
    float ry = torch_remainder(__fadd_rn(__fmul_rn((float)rb, apc), __fmul_rn(res_norm, apc_half)), two_pi);
    if (ry > pi) ry = __fsub_rn(ry, two_pi);
    cur += 2 * c.num_head_bin;
    const float h = rd_anchor_size(r[cur], c.anchor[0]);
    const float w = rd_anchor_size(r[cur + 1], c.anchor[1]);
    const float l = rd_anchor_size(r[cur + 2], c.anchor[2]);
    float *o = boxes + i * 7;
    o[0] = __fadd_rn(px, p[0]);
    o[1] = __fadd_rn(py, h / 2);
    o[2] = __fadd_rn(pz, p[2]);
    o[3] = h; o[4] = w; o[5] = l; o[6] = ry;
}

// tables: payload (b, 2, rows, 8) = box7 + score, bev (b, 2, rows, 5), counts (b, 2)
__global__ __launch_bounds__(1024) void band_select_kernel(
    int n, int rows, int pre_near, int pre_far, const float *__restrict__ boxes, const float *__restrict__ scores,
    const int *__restrict__ order, float *__restrict__ payload, float *__restrict__ bev, int *__restrict__ counts)
{
    __shared__ int wcnt[2][16];
    __shared__ int tot[2];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float *__restrict__ bx = boxes + (long)b * n * 7;
    const float *__restrict__ sc = scores + (long)b * n;
    const int *__restrict__ ord = order + (long)b * n;
    float *__restrict__ pay = payload + (long)b * 2 * rows * 8;
    float *__restrict__ bv = bev + (long)b * 2 * rows * 5;
    if (t < 2) tot[t] = 0;
    __syncthreads();

    auto emit = [&](int band, int slot, int k) {
        float *o = pay + ((long)band * rows + slot) * 8;
        const float *q = bx + (long)k * 7;
#pragma unroll
        for (int e = 0; e < 7; ++e) o[e] = q[e];
        o[7] = sc[k];
        bev_row(q, bv + ((long)band * rows + slot) * 5);
    };

    // pass 0: near band gets near ranks [0, pre_near), far band far ranks [0, pre_far)
    // pass 1 (only if the scene has no far point): far band gets near ranks [pre_near, pre_near + pre_far)
    for (int pass = 0; pass < 2; ++pass) {
        int near_seen = 0, far_seen = 0;
        for (int base = 0; base < n; base += 1024) {
            if (pass == 0 && near_seen >= pre_near && far_seen >= pre_far) break;
            if (pass == 1 && near_seen >= pre_near + pre_far) break;
            const int s = base + t;
            int k = -1;
            bool is_near = false, is_far = false;
            if (s < n) {
                k = ord[s];
                const float dist = bx[(long)k * 7 + 2];
                is_near = dist > 0.f && dist <= 40.0f;
                is_far = dist > 40.0f && dist <= 80.0f;
            }
            const unsigned long long mn = __ballot(is_near), mf = __ballot(is_far);
            if (lane == 0) { wcnt[0][w] = __popcll(mn); wcnt[1][w] = __popcll(mf); }
            __syncthreads();
            int nb = near_seen, fb = far_seen, nt = 0, ft = 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if (q < w) { nb += wcnt[0][q]; fb += wcnt[1][q]; }
                nt += wcnt[0][q]; ft += wcnt[1][q];
            }
            const unsigned long long below = (1ull << lane) - 1ull;
            if (is_near) {
                const int rank = nb + __popcll(mn & below);
                if (pass == 0 && rank < pre_near) emit(0, rank, k);
                if (pass == 1 && rank >= pre_near && rank < pre_near + pre_far) emit(1, rank - pre_near, k);
            }
            if (is_far && pass == 0) {
                const int rank = fb + __popcll(mf & below);
                if (rank < pre_far) emit(1, rank, k);
            }
            near_seen += nt; far_seen += ft;
            __syncthreads();
        }
        if (pass == 0) {
            if (t == 0) { tot[0] = near_seen; tot[1] = far_seen; }
            __syncthreads();
            // the scan stops early once both quotas are full, so "no far point" is only known if it ran
            // to the end; a scene with an empty far band never fills the far quota, hence it did
            if (tot[1] != 0) {
                if (t == 0) { counts[b * 2] = min(tot[0], pre_near); counts[b * 2 + 1] = min(tot[1], pre_far); }
                return;
            }
        } else if (t == 0) {
            counts[b * 2] = min(tot[0], pre_near);
            counts[b * 2 + 1] = max(0, min(near_seen, pre_near + pre_far) - pre_near);
        }
    }
}

__global__ __launch_bounds__(128) void assemble_rois_kernel(
    int rows, int keep_stride, int post_near, int post_far, const float *__restrict__ payload,
    const int *__restrict__ keep, const int *__restrict__ num, float *__restrict__ rois, float *__restrict__ scores)
{
    // one workgroup per scene, lane j takes RoIs j, j + 128, ...: one trip for the inference quotas (post <= 128), up to four for
    // the training ones (post <= 512)
    const int b = blockIdx.x;
    const int post = post_near + post_far;
    const int kn = min(num[b * 2], post_near), kf = min(num[b * 2 + 1], post_far);
    for (int j = threadIdx.x; j < post; j += 128) {
        int band = -1, slot = 0;
        if (j < kn) { band = 0; slot = keep[(b * 2) * keep_stride + j]; }
        else if (j < kn + kf) { band = 1; slot = keep[(b * 2 + 1) * keep_stride + (j - kn)]; }
        store_kept_or_zeros(band < 0 ? nullptr : payload + (((long)b * 2 + band) * rows + slot) * 8, rois + ((long)b * post + j) * 7,
                            scores + (long)b * post + j);
    }
}

// The per-point RCNN inputs of point_rcnn.py:44-52 / rcnn_net.py:131-137 in ONE launch (round 4; torch ran them as six: sigmoid, compare,
// cast, norm, divide, subtract): seg = sigmoid(score) > thresh as 0 / 1 floats, depth = |xyz|, depth_norm = depth / 70 - 0.5.
__global__ __launch_bounds__(256) void point_aux_kernel(long rows, float thresh, const float *__restrict__ scores,
                                                        const float *__restrict__ xyz, float *__restrict__ seg,
                                                        float *__restrict__ depth, float *__restrict__ depth_norm)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    seg[r] = rpn_seg_fg(scores[r], thresh) ? 1.0f : 0.0f;
    const float x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
    const float d = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
    depth[r] = d;
    depth_norm[r] = __fsub_rn(__fdiv_rn(d, 70.0f), 0.5f);
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_point_aux(long rows, float thresh, const float *scores, const float *xyz, float *seg, float *depth,
                               float *depth_norm, void *stream)
{
    PRCNN_REQUIRE(rows >= 0, "point_aux: bad sizes");
    if (rows == 0) return PRCNN_OK;
    PRCNN_REQUIRE(scores && xyz && seg && depth && depth_norm, "point_aux: null pointer");
    hipLaunchKernelGGL(point_aux_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, thresh, scores, xyz,
                       seg, depth, depth_norm);
    return check_launch("point_aux");
}

// the proposal layer behind the decode: boxes_in != NULL = every point's decoded box (b,n,7) as prcnn_rpn_tail_lin_boxes leaves it
// (round 5: the decode rides in the RPN tail kernel), else reg + xyz are decoded here first
static int rpn_proposals_any(int b, int n, const DecodeCfg *dc, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated_nms,
                             const float *xyz, const float *scores, const float *reg, const float *boxes_in, float *rois,
                             float *roi_scores, void *stream)
{
    PRCNN_REQUIRE(n <= SS_MAX_N, "rpn_proposals: n=%d > 65536 points per scene unsupported by the fused path", n);   // (the sort's limit; the band scan takes any n)
    const int pre_near = (int)(pre_nms_top_n * 0.7), pre_far = pre_nms_top_n - pre_near;
    const int post_near = (int)(post_nms_top_n * 0.7), post_far = post_nms_top_n - post_near;
    // 512 = TRAIN.RPN_POST_NMS_TOP_N of the shipped configurations: 358 near + 154 far, the axis-aligned NMS on the quota form's second
    // instantiation (nms_device.hip), the assembly in four trips; <= 128 launches what it always launched
    PRCNN_REQUIRE(post_nms_top_n >= 0 && post_nms_top_n <= 512 && post_near >= post_far && pre_near >= pre_far, "rpn_proposals: unsupported quotas");
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(scores && rois && roi_scores && (boxes_in || (xyz && reg)), "rpn_proposals: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rows = pre_near;
    ScratchPlan plan;
    const size_t o_boxes = plan.take(boxes_in ? 0 : (size_t)b * n * 7 * 4), o_order = plan.take((size_t)b * n * 4);
    const size_t o_pay = plan.take((size_t)b * 2 * rows * 8 * 4), o_bev = plan.take((size_t)b * 2 * rows * 5 * 4);
    const size_t o_cnt = plan.take((size_t)b * 2 * 4), o_keep = plan.take((size_t)b * 2 * post_near * 4), o_num = plan.take((size_t)b * 2 * 4);
    char *base = scratch_for(st, plan.need, 2);
    if (!base) { set_error("rpn_proposals: cannot allocate %zu bytes of scratch", plan.need); return PRCNN_ELAUNCH; }
    const float *boxes = boxes_in ? boxes_in : (const float *)(base + o_boxes);
    int *order = (int *)(base + o_order);
    float *payload = (float *)(base + o_pay), *bev = (float *)(base + o_bev);
    int *counts = (int *)(base + o_cnt), *keep = (int *)(base + o_keep), *num = (int *)(base + o_num);

    const long total = (long)b * n;
    if (!boxes_in)
        hipLaunchKernelGGL(rpn_decode_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, total, *dc, xyz, reg, (float *)(base + o_boxes));
    int rc = score_order(b, n, scores, order, st);
    if (rc != PRCNN_OK) return rc;
    // (round 4 tried the selection in two steps -- one scan over 16 consecutive positions per thread + table emission from LDS: 12 us instead of
    //  61 alone, 6460 / 6484 scenes/s against 6518 / 6522 at K = 96: the proposal stream's latency kernels do not bound a step.  Not kept.)
    hipLaunchKernelGGL(band_select_kernel, dim3(b), dim3(1024), 0, st, n, rows, pre_near, pre_far, boxes, scores, order,
                       payload, bev, counts);
    rc = check_launch("rpn_proposals");
    if (rc != PRCNN_OK) return rc;
    rc = nms_device(2 * b, rows, counts, bev, nms_thresh, rotated_nms, post_near, keep, num, st);
    if (rc != PRCNN_OK) return rc;
    hipLaunchKernelGGL(assemble_rois_kernel, dim3(b), dim3(128), 0, st, rows, post_near, post_near, post_far, payload, keep,
                       num, rois, roi_scores);
    return check_launch("rpn_proposals");
}

// xyz (b,n,3), scores (b,n) raw RPN scores, reg (b,n,channels) -> rois (b, post_top_n, 7), roi_scores (b, post_top_n)
// distance-based proposal (RPN_DISTANCE_BASED_PROPOSE), get_y_by_bin = False, get_ry_fine = False.
// post_top_n <= 512 (near int(0.7 post) <= 358, far <= 154; near >= far for pre and post): inference asks for <= 128, training for 512.
extern "C" int prcnn_rpn_proposals(int b, int n, int channels, float loc_scope, float loc_bin_size,
                                   int num_head_bin, int xz_fine, const float *anchor_size_host,
                                   int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated_nms,
                                   const float *xyz, const float *scores, const float *reg, float *rois,
                                   float *roi_scores, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n > 0 && channels > 0 && num_head_bin > 0 && loc_bin_size > 0, "rpn_proposals: bad sizes");
    PRCNN_REQUIRE(anchor_size_host, "rpn_proposals: anchor size missing");
    DecodeCfg c;
    c.loc_scope = loc_scope; c.loc_bin_size = loc_bin_size;
    c.nbin = (int)(loc_scope / loc_bin_size) * 2;
    c.num_head_bin = num_head_bin; c.xz_fine = xz_fine ? 1 : 0; c.channels = channels;
    for (int i = 0; i < 3; ++i) c.anchor[i] = anchor_size_host[i];
    const int expect = c.nbin * (c.xz_fine ? 4 : 2) + 1 + 2 * num_head_bin + 3;
    PRCNN_REQUIRE(channels == expect, "rpn_proposals: %d regression channels, layout needs %d", channels, expect);
    PRCNN_REQUIRE(b == 0 || (xyz && reg), "rpn_proposals: null pointer");
    return rpn_proposals_any(b, n, &c, pre_nms_top_n, post_nms_top_n, nms_thresh, rotated_nms, xyz, scores, reg, nullptr, rois, roi_scores,
                             stream);
}

// the same layer over boxes decoded already (prcnn_rpn_tail_lin_boxes): boxes (b,n,7), scores (b,n)
extern "C" int prcnn_rpn_proposals_boxes(int b, int n, int pre_nms_top_n, int post_nms_top_n, float nms_thresh, int rotated_nms,
                                         const float *scores, const float *boxes, float *rois, float *roi_scores, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n > 0, "rpn_proposals_boxes: bad sizes");
    PRCNN_REQUIRE(b == 0 || boxes, "rpn_proposals_boxes: null pointer");
    return rpn_proposals_any(b, n, nullptr, pre_nms_top_n, post_nms_top_n, nms_thresh, rotated_nms, nullptr, scores, nullptr, boxes, rois,
                             roi_scores, stream);
}

