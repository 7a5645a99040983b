// final_stage.hip -- the RCNN final stage (eval_rcnn.py:506-530, 611-629): decode the RCNN regression against its RoI, score
// threshold, order by raw score, rotated NMS over the BEV boxes, survivors in descending score order.  One workgroup per scene, one
// lane per RoI (m <= 128); the <= 128 scores are sorted with a bitonic network in LDS.  Two forms behind prcnn_rcnn_postprocess:
//   * rcnn_final_kernel: the whole stage of a scene in ONE workgroup (round 4), for nms_thresh >= 0 -- what the engine runs.  The four
//     launches of the other form (decode + sort, all-pairs suppression mask, resolve, gather: 88 us of the feature stream per step, most
//     of it launch gaps and half-empty waves) become one: decode and score-sort by the same prologue, the sorted BEV rows stay in LDS;
//     CANDIDATE pairs: every (row r, column c > r) whose boxes can touch at all (rbox_far_apart: bounding circles) goes onto a list
//     in LDS -- of the 4950 pairs of 100 boxes a few hundred; the rotated IoU (~600 VALU instructions, divergent) then runs over the
//     compacted list only, full waves; the greedy resolve over the row masks (iou3d.cpp:100-119) by one thread, then the gather.
//     Same expressions in the same (row, column) order as nms_dense_mask_kernel: the same keep list (a pair the filter drops has
//     overlap exactly 0 in the reference's arithmetic as well -- no vertex of the clipped polygon exists).
//   * four launches: rcnn_decode_select_kernel, nms_device's dense form (two launches), rcnn_final_gather_kernel.  It serves
//     nms_thresh < 0, where every pair suppresses and the candidate filter would answer differently.
#include "nms_blocks.hpp"
#include "rpn_decode.hpp"
#include "score_sort.hpp"

namespace prcnn {

struct RcnnCfg {
    float loc_scope, loc_bin_size, loc_y_scope, loc_y_bin_size, score_thresh;
    int nbin, nbin_y, num_head_bin, y_by_bin, channels;
    float anchor[3];
};

// decode_bbox_target of one RoI (bbox_transform.py:30-127 with get_xz_fine = get_ry_fine = True): r = its regression row, roi = its box
__device__ __forceinline__ void rcnn_decode_box(const RcnnCfg &c, const float *__restrict__ r, const float *__restrict__ roi, float (&box)[7])
{
    const int nb = c.nbin;
    const int xb = argmax_row(r, nb), zb = argmax_row(r + nb, nb);
    const float px = rd_add_residual(rd_bin_centre(xb, c.loc_bin_size, c.loc_scope), r[2 * nb + xb], c.loc_bin_size);      // get_xz_fine = True
    const float pz = rd_add_residual(rd_bin_centre(zb, c.loc_bin_size, c.loc_scope), r[3 * nb + zb], c.loc_bin_size);
    int cur = 4 * nb;
    float py;
    if (c.y_by_bin) {
        const int yb = argmax_row(r + cur, c.nbin_y);
        py = rd_add_residual(rd_bin_centre(yb, c.loc_y_bin_size, c.loc_y_scope), r[cur + c.nbin_y + yb], c.loc_y_bin_size);
        py = __fadd_rn(py, roi[1]);
        cur += 2 * c.nbin_y;
    } else {
        py = __fadd_rn(roi[1], r[cur]);
        cur += 1;
    }
    const int rb = argmax_row(r + cur, c.num_head_bin);
    const float res_norm = r[cur + c.num_head_bin + rb];
    // get_ry_fine = True: bins over +-pi/4 around the RoI heading
    const float apc = (float)((M_PI / 2) / c.num_head_bin);
    const float apc_half = (float)(((M_PI / 2) / c.num_head_bin) / 2.0);
    float ry = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn((float)rb, apc), apc_half), __fmul_rn(res_norm, apc_half)), (float)(M_PI / 4));
    cur += 2 * c.num_head_bin;
    const float h = rd_anchor_size(r[cur], c.anchor[0]);
    const float w = rd_anchor_size(r[cur + 1], c.anchor[1]);
    const float l = rd_anchor_size(r[cur + 2], c.anchor[2]);
    // rotate (px, pz) by -roi_ry back to the scene frame (rotate_pc_along_y_torch with -ry), add the RoI centre
    const float roi_ry = roi[6];
    const float cosa = cosf(-roi_ry), sina = sinf(-roi_ry);
    const float nx = __fadd_rn(__fmul_rn(px, cosa), __fmul_rn(pz, -sina));
    const float nz = __fadd_rn(__fmul_rn(px, sina), __fmul_rn(pz, cosa));
    box[0] = __fadd_rn(nx, roi[0]); box[1] = py; box[2] = __fadd_rn(nz, roi[2]);
    box[3] = h; box[4] = w; box[5] = l; box[6] = __fadd_rn(ry, roi_ry);
}

constexpr int RF_THREADS = 256, RF_MAX = 128;

// The prologue of both forms, on a workgroup of RF_MAX lanes or more.  Lane t < m decodes RoI t of scene b and writes the box to pred
// (and, with its raw score, to row t of s_box where the caller keeps such a table in LDS: LDS_BOX); lane t < RF_MAX sets key t --
// selected RoIs (sigmoid(raw) > score_thresh) first, by descending raw score; unselected and absent ones after them -- and the
// selected are counted into *nsel (zeroed and fenced by the caller).
template <bool LDS_BOX>
__device__ __forceinline__ void rcnn_decode_select(int b, int t, int m, const RcnnCfg &c, const float *__restrict__ rois,
                                                   const float *__restrict__ reg, const float *__restrict__ cls, float *__restrict__ pred,
                                                   float *s_box, unsigned long long *keys, int *nsel)
{
    float raw = 0.f;
    bool selected = false;
    if (t < m) {
        float box[7];
        rcnn_decode_box(c, reg + ((long)b * m + t) * c.channels, rois + ((long)b * m + t) * 7, box);
        raw = cls[(long)b * m + t];
        const float norm = 1.0f / (1.0f + expf(-raw));
        selected = norm > c.score_thresh;
        float *o = pred + ((long)b * m + t) * 7;
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            o[e] = box[e];
            if (LDS_BOX) s_box[t * 8 + e] = box[e];
        }
        if (LDS_BOX) s_box[t * 8 + 7] = raw;
    }
    if (t < RF_MAX) {
        keys[t] = (t < m && selected) ? sort_key(raw, (unsigned)t) : (~0ull - 127 + t);
        if (t < m && selected) atomicAdd(nsel, 1);
    }
}

__global__ __launch_bounds__(RF_MAX) void rcnn_decode_select_kernel(
    int m, RcnnCfg c, const float *__restrict__ rois, const float *__restrict__ reg, const float *__restrict__ cls,
    float *__restrict__ pred /* (b,m,7) decoded, RoI order */, float *__restrict__ sorted /* (b,m,8) box7+raw, score order */,
    float *__restrict__ bev /* (b,m,5) */, int *__restrict__ counts)
{
    __shared__ unsigned long long keys[RF_MAX];
    __shared__ int nsel;
    const int b = blockIdx.x, t = threadIdx.x;
    if (t == 0) nsel = 0;
    __syncthreads();
    rcnn_decode_select<false>(b, t, m, c, rois, reg, cls, pred, nullptr, keys, &nsel);
    __syncthreads();
    bitonic_sort_partner<RF_MAX>(keys, t);
    // slot t of the sorted table takes the box lane `src` decoded (its global write is ordered by the barriers above)
    if (t < m) {
        float *o = sorted + ((long)b * m + t) * 8;
        float *v = bev + ((long)b * m + t) * 5;
        if (t < nsel) {
            const int src = (int)(keys[t] & 0xffffffffu);
            const float *q = pred + ((long)b * m + src) * 7;
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = q[4]; o[5] = q[5]; o[6] = q[6];
            o[7] = cls[(long)b * m + src];
            bev_row(q, v);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
            for (int e = 0; e < 5; ++e) v[e] = 0.f;
        }
    }
    if (t == 0) counts[b] = nsel;
}

__global__ __launch_bounds__(RF_MAX) void rcnn_final_gather_kernel(int m, const float *__restrict__ sorted,
                                                                  const int *__restrict__ keep, const int *__restrict__ num,
                                                                  float *__restrict__ boxes, float *__restrict__ scores)
{
    const int b = blockIdx.x, j = threadIdx.x;
    if (j >= m) return;
    store_kept_or_zeros(j < num[b] ? sorted + ((long)b * m + keep[(long)b * m + j]) * 8 : nullptr, boxes + ((long)b * m + j) * 7,
                        scores + (long)b * m + j);
}

__global__ __launch_bounds__(RF_THREADS) void rcnn_final_kernel(
    int m, RcnnCfg c, float nms_thresh, const float *__restrict__ rois, const float *__restrict__ reg, const float *__restrict__ cls,
    float *__restrict__ pred /* (b,m,7) decoded, RoI order */, float *__restrict__ boxes /* (b,m,7) */, float *__restrict__ scores /* (b,m) */,
    int *__restrict__ num /* (b) */, int spb /* > 0: boxes = a sequence of BLOBS of spb scenes each, [spb m 7 boxes | spb m scores | spb num] */)
{
    if (spb > 0) {
        // (round 5) one blob per batch of spb scenes inside a launch over several batches: each batch's detections leave the device
        // with ONE copy (a pair of batches per launch used to cost three copies per batch)
        const int bl = blockIdx.x / spb, si = blockIdx.x - bl * spb;
        float *base = boxes + (long)bl * spb * (m * 8 + 1);
        // re-based so that the scene indexing below (b = blockIdx.x) lands on this scene's slices
        boxes = base + ((long)si - blockIdx.x) * m * 7;
        scores = base + (long)spb * m * 7 + ((long)si - blockIdx.x) * m;
        num = reinterpret_cast<int *>(base + (long)spb * m * 8) + (si - (int)blockIdx.x);
    }
    __shared__ unsigned long long keys[RF_MAX];
    __shared__ unsigned long long s_mask[RF_MAX][2];
    __shared__ float s_box[RF_MAX * 8];                  // decoded box + raw score, RoI order
    __shared__ float s_row[RF_MAX * 7];                  // BEV box + cos, sin of the heading, score order
    __shared__ int s_src[RF_MAX], s_keep[RF_MAX];
    __shared__ unsigned int s_pair[RF_MAX * (RF_MAX - 1) / 2];      // (r << 16) | c
    __shared__ int nsel, s_npair, s_nkeep;
    __shared__ float s_poly[POLY_LDS_FLOATS * RF_THREADS];          // the clipped polygons (72 KB): see PolyLds
    const int b = blockIdx.x, t = threadIdx.x;
    if (t == 0) { nsel = 0; s_npair = 0; }
    __syncthreads();
    rcnn_decode_select<true>(b, t, m, c, rois, reg, cls, pred, s_box, keys, &nsel);
    if (t < RF_MAX) { s_mask[t][0] = 0ull; s_mask[t][1] = 0ull; }
    __syncthreads();
    bitonic_sort_partner<RF_MAX>(keys, t);
    const int n = nsel;
    if (t < n) {                                         // slot t of the score order holds RoI `src`
        const int src = (int)(keys[t] & 0xffffffffu);
        s_src[t] = src;
        const float *q = s_box + src * 8;
        float *v = s_row + t * 7;
        bev_row(q, v);
        v[5] = cos_f32(q[6]); v[6] = sin_f32(q[6]);
    }
    __syncthreads();
    // candidate pairs: e = r (2 n - r - 1) / 2 + (c - r - 1) enumerates (r, c > r) row by row
    const int P = n * (n - 1) / 2;
    for (int e = t; e < P; e += RF_THREADS) {
        const float tn = (float)(2 * n - 1);
        int r = (int)((tn - sqrtf(tn * tn - 8.0f * (float)e)) * 0.5f);
        r = min(max(r, 0), n - 2);
        while (r > 0 && r * (2 * n - r - 1) / 2 > e) --r;
        while ((r + 1) * (2 * n - r - 2) / 2 <= e) ++r;
        const int cc = r + 1 + (e - r * (2 * n - r - 1) / 2);
        if (!rbox_far_apart(s_row + r * 7, s_row + cc * 7)) s_pair[atomicAdd(&s_npair, 1)] = ((unsigned)r << 16) | (unsigned)cc;
    }
    __syncthreads();
    const int np = s_npair;
    for (int i = t; i < np; i += RF_THREADS) {
        const unsigned int rc = s_pair[i];
        const int r = (int)(rc >> 16), cc = (int)(rc & 0xffffu);
        RBox C;
#pragma unroll
        for (int q = 0; q < 5; ++q) C.v[q] = s_row[cc * 7 + q];
        C.cosv = s_row[cc * 7 + 5]; C.sinv = s_row[cc * 7 + 6];
        if (suppresses<true, true>(s_row, r, C, nms_thresh, s_poly + t, RF_THREADS))
            atomicOr(&s_mask[r][cc >> 6], 1ull << (cc & 63));
    }
    __syncthreads();
    if (t == 0) {                                        // the host loop of iou3d.cpp:100-119 over the row masks: every survivor is wanted
        s_nkeep = resolve_mask128<false>(s_mask, n, n, [&](int slot, int cc) { s_keep[slot] = cc; });
        num[b] = s_nkeep;
    }
    __syncthreads();
    if (t < m)
        store_kept_or_zeros(t < s_nkeep ? s_box + s_src[s_keep[t]] * 8 : nullptr, boxes + ((long)b * m + t) * 7, scores + (long)b * m + t);
}

}  // namespace prcnn

using namespace prcnn;

// rois (b,m,7), rcnn_reg (b,m,channels), rcnn_cls (b,m) raw -> pred_boxes3d (b,m,7) decoded in RoI order,
// boxes (b,m,7) / scores (b,m) = survivors of score threshold + rotated NMS in descending score order, zero
// padded, num (b) i32.  get_xz_fine = get_ry_fine = True (eval_rcnn.py:516-523).  m <= 128.
static int rcnn_postprocess_any(int b, int m, int channels, float loc_scope, float loc_bin_size,
                                int num_head_bin, int y_by_bin, float loc_y_scope, float loc_y_bin_size,
                                const float *anchor_size_host, float score_thresh, float nms_thresh,
                                const float *rois, const float *rcnn_reg, const float *rcnn_cls,
                                float *pred_boxes3d, float *boxes, float *scores, int *num, int scenes_per_blob, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && m > 0 && m <= RF_MAX && channels > 0 && num_head_bin > 0, "rcnn_postprocess: bad sizes (m <= 128)");
    PRCNN_REQUIRE(anchor_size_host, "rcnn_postprocess: anchor size missing");
    RcnnCfg c;
    c.loc_scope = loc_scope; c.loc_bin_size = loc_bin_size; c.loc_y_scope = loc_y_scope; c.loc_y_bin_size = loc_y_bin_size;
    c.score_thresh = score_thresh;
    c.nbin = (int)(loc_scope / loc_bin_size) * 2;
    c.nbin_y = (int)(loc_y_scope / loc_y_bin_size) * 2;
    c.num_head_bin = num_head_bin; c.y_by_bin = y_by_bin ? 1 : 0; c.channels = channels;
    for (int i = 0; i < 3; ++i) c.anchor[i] = anchor_size_host[i];
    const int expect = c.nbin * 4 + (c.y_by_bin ? 2 * c.nbin_y : 1) + 2 * num_head_bin + 3;
    PRCNN_REQUIRE(channels == expect, "rcnn_postprocess: %d regression channels, layout needs %d", channels, expect);
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(rois && rcnn_reg && rcnn_cls && pred_boxes3d && boxes && scores && num, "rcnn_postprocess: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PRCNN_REQUIRE(scenes_per_blob == 0 || nms_thresh >= 0.f, "rcnn_postprocess_blobs: needs the one-workgroup final stage (nms_thresh >= 0)");
    if (nms_thresh >= 0.f) {
        hipLaunchKernelGGL(rcnn_final_kernel, dim3(b), dim3(RF_THREADS), 0, st, m, c, nms_thresh, rois, rcnn_reg, rcnn_cls, pred_boxes3d,
                           boxes, scores, num, scenes_per_blob);
        return check_launch("rcnn_postprocess");
    }
    ScratchPlan plan;
    const size_t o_sorted = plan.take((size_t)b * m * 8 * 4), o_bev = plan.take((size_t)b * m * 5 * 4);
    const size_t o_cnt = plan.take((size_t)b * 4), o_keep = plan.take((size_t)b * m * 4);
    char *base = scratch_for(st, plan.need, 3);
    if (!base) { set_error("rcnn_postprocess: cannot allocate %zu bytes of scratch", plan.need); return PRCNN_ELAUNCH; }
    float *sorted = (float *)(base + o_sorted), *bev = (float *)(base + o_bev);
    int *counts = (int *)(base + o_cnt), *keep = (int *)(base + o_keep);
    hipLaunchKernelGGL(rcnn_decode_select_kernel, dim3(b), dim3(RF_MAX), 0, st, m, c, rois, rcnn_reg, rcnn_cls, pred_boxes3d,
                       sorted, bev, counts);
    int rc = check_launch("rcnn_postprocess");
    if (rc != PRCNN_OK) return rc;
    rc = nms_device(b, m, counts, bev, nms_thresh, 1, m, keep, num, st);
    if (rc != PRCNN_OK) return rc;
    hipLaunchKernelGGL(rcnn_final_gather_kernel, dim3(b), dim3(RF_MAX), 0, st, m, sorted, keep, num, boxes, scores);
    return check_launch("rcnn_postprocess");
}

extern "C" int prcnn_rcnn_postprocess(int b, int m, int channels, float loc_scope, float loc_bin_size,
                                      int num_head_bin, int y_by_bin, float loc_y_scope, float loc_y_bin_size,
                                      const float *anchor_size_host, float score_thresh, float nms_thresh,
                                      const float *rois, const float *rcnn_reg, const float *rcnn_cls,
                                      float *pred_boxes3d, float *boxes, float *scores, int *num, void *stream)
{
    return rcnn_postprocess_any(b, m, channels, loc_scope, loc_bin_size, num_head_bin, y_by_bin, loc_y_scope, loc_y_bin_size,
                                anchor_size_host, score_thresh, nms_thresh, rois, rcnn_reg, rcnn_cls, pred_boxes3d, boxes, scores, num, 0,
                                stream);
}

// The same with the results as one BLOB per batch of scenes_per_blob scenes (b % scenes_per_blob == 0): blobs (b / spb, spb (8 m + 1))
// f32, each [spb m 7 boxes | spb m scores | spb num (i32 bits)] -- eval_rcnn.split_detections' layout per batch, so that a launch over a
// PAIR of batches still hands every batch's detections to the host with one copy.  Needs the one-workgroup final kernel (nms_thresh >= 0).
extern "C" int prcnn_rcnn_postprocess_blobs(int b, int m, int channels, float loc_scope, float loc_bin_size,
                                            int num_head_bin, int y_by_bin, float loc_y_scope, float loc_y_bin_size,
                                            const float *anchor_size_host, float score_thresh, float nms_thresh,
                                            const float *rois, const float *rcnn_reg, const float *rcnn_cls,
                                            float *pred_boxes3d, float *blobs, int scenes_per_blob, void *stream)
{
    PRCNN_REQUIRE(scenes_per_blob > 0 && b % scenes_per_blob == 0 && nms_thresh >= 0.f, "rcnn_postprocess_blobs: %d scenes in blobs of %d",
                  b, scenes_per_blob);
    PRCNN_REQUIRE(blobs || b == 0, "rcnn_postprocess_blobs: null pointer");
    return rcnn_postprocess_any(b, m, channels, loc_scope, loc_bin_size, num_head_bin, y_by_bin, loc_y_scope, loc_y_bin_size,
                                anchor_size_host, score_thresh, nms_thresh, rois, rcnn_reg, rcnn_cls, pred_boxes3d, blobs, blobs,
                                reinterpret_cast<int *>(blobs), scenes_per_blob, stream);
}
