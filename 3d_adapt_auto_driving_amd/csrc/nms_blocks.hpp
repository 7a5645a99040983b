// nms_blocks.hpp -- what the greedy-NMS kernels of nms_device.hip, iou3d.hip and final_stage.hip have in common: the problem header of
// a batched launch, the staging of row boxes in LDS, and the two serial resolves that restate the host loop of iou3d.cpp:100-119 (over
// a 64-row block's diagonal words; over the two-word row masks of a problem of <= 128 boxes).  Also the declaration of nms_device and,
// for its callers (proposal.hip, final_stage.hip), the BEV row they feed it and the output slot they fill from its keep list.
#pragma once
#include "common.hpp"
#include "rbox_iou.hpp"

namespace prcnn {

constexpr int NMS_MAX_N = 65536;   // boxes per problem: the removed bitmap lives in LDS (8 KiB)
constexpr int ND_MAX = 128;        // boxes per problem of the dense form: a row's suppression mask is two words

// nms_device.hip: problem p = the first counts[p] (or n_max) of boxes (nprob, n_max, 5), sorted by descending score -> keep (nprob, max_keep)
// = the first max_keep entries of the reference's keep list, -1 padded; num_keep (nprob)
int nms_device(int nprob, int n_max, const int *counts, const float *boxes, float thresh, int rotated,
               int max_keep, int *keep, int *num_keep, hipStream_t st);

// kernel<true> or kernel<false>, by the host's `rotated`
template <class K>
static inline K by_rotation(int rotated, K rot, K flat) { return rotated ? rot : flat; }

// what goes in: the BEV row of a box7 (x, y, z, h, w, l, ry) -> (x - l/2, z - w/2, x + l/2, z + w/2, ry), boxes3d_to_bev_torch (kitti_utils.py:134-147)
__device__ __forceinline__ void bev_row(const float *q, float *v)
{
    const float hl = q[5] / 2, hw = q[4] / 2;
    v[0] = q[0] - hl; v[1] = q[2] - hw; v[2] = q[0] + hl; v[3] = q[2] + hw; v[4] = q[6];
}
// what comes out: an output slot (box `o`, score `*s`) gets its kept row q = box7 + score, or zeros where there is none (q = nullptr)
__device__ __forceinline__ void store_kept_or_zeros(const float *q, float *o, float *s)
{
    if (q) {
#pragma unroll
        for (int e = 0; e < 7; ++e) o[e] = q[e];
        *s = q[7];
    } else {                                      // (one branch: `q ? q[e] : 0.f` per element compiled to 10 - 11 more instructions in the two gather kernels)
#pragma unroll
        for (int e = 0; e < 7; ++e) o[e] = 0.f;
        *s = 0.f;
    }
}

// problem header: the box count, clamped, and where the problem's boxes and its row of the keep table begin (in elements)
struct NmsProblem {
    int n;
    long boxes, keep;
};
__device__ __forceinline__ NmsProblem nms_problem(int prob, int n_max, const int *__restrict__ counts, int max_keep)
{
    const int n = counts ? counts[prob] : n_max;
    return {min(max(n, 0), n_max), (long)prob * n_max * 5, (long)prob * max_keep};
}

// row staging: thread t < rows copies BEV row r0 + t into its 7-float slot of s_row, with cos / sin of the heading when ROTATED
template <bool ROTATED>
__device__ __forceinline__ void stage_rows(float *s_row, const float *__restrict__ boxes, int r0, int rows, int t)
{
    if (t < rows) {
        const float *p = boxes + (long)(r0 + t) * 5;
#pragma unroll
        for (int q = 0; q < 5; ++q) s_row[t * 7 + q] = p[q];
        if (ROTATED) {
            s_row[t * 7 + 5] = cos_f32(p[4]);
            s_row[t * 7 + 6] = sin_f32(p[4]);
        }
    }
}

// Serial resolve of a block of <= 64 rows, one thread: row cl is kept unless bit cl of `gone` is set (dropped by a row kept in an earlier
// block) or s_diag[cl] (the rows r < cl of the block that suppress it) meets a kept row.  on_keep(slot, cl) per kept row, in order, until
// max_keep are kept.  -> the new count; kept = the block's kept rows.
template <class OnKeep>
__device__ __forceinline__ int resolve_block64(unsigned long long gone, const unsigned long long *s_diag, int rows, int nk,
                                               int max_keep, unsigned long long &kept, OnKeep on_keep)
{
    kept = 0ull;
    for (int cl = 0; cl < rows && nk < max_keep; ++cl) {
        if ((gone >> cl) & 1ull) continue;
        if (s_diag[cl] & kept) continue;
        kept |= 1ull << cl;
        on_keep(nk++, cl);
    }
    return nk;
}

// Serial resolve of a problem of n <= ND_MAX boxes over its row masks (mask[r] = the columns c > r that row r suppresses), one thread:
// on_keep(slot, c) per kept box, in order, until max_keep are kept (QUOTA = false: every survivor is wanted, no test).  -> the number kept.
template <bool QUOTA = true, class OnKeep>
__device__ __forceinline__ int resolve_mask128(const unsigned long long (*mask)[2], int n, int max_keep, OnKeep on_keep)
{
    unsigned long long gone0 = 0ull, gone1 = 0ull;
    int nk = 0;
    for (int c = 0; c < n && (!QUOTA || nk < max_keep); ++c) {
        const bool gone = c < 64 ? (gone0 >> c) & 1ull : (gone1 >> (c - 64)) & 1ull;
        if (gone) continue;
        on_keep(nk++, c);
        gone0 |= mask[c][0];
        gone1 |= mask[c][1];
    }
    return nk;
}

}  // namespace prcnn
