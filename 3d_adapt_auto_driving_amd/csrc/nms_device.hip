// nms_device.hip -- the batched, device-resident greedy NMS (this project's extension of the reference's iou3d module): nms_device and
// its entry prcnn_nms_device.  The proposal layer (proposal.hip) and the four-launch final stage (final_stage.hip) call it.
//
// Design.  The reference builds the full n x n/64 suppression mask on the device, copies it to the host and reduces it serially
// there (3 round trips per scene in eval_rcnn).  Here one workgroup per problem walks the score-sorted boxes in blocks of 64 rows
// and evaluates IoUs LAZILY: for row block r it computes, for every still-alive later column, the 64-bit word "which rows of block r
// suppress me" (rows staged in LDS, one column per lane), resolves the 64 rows of the block serially against the already-known
// words (same order as the host loop), then kills the columns suppressed by the rows that were kept.  It stops as soon as `max_keep`
// boxes are kept -- the proposal layer only ever uses the first 70/30 -- and the kept list is, by construction, the prefix of the
// reference's list.  No host round trip, no mask in HBM.  Three forms, chosen by shape in nms_device: dense (n_max <= 128), quota
// (axis-aligned, max_keep <= 512), lazy (everything else).
#include "nms_blocks.hpp"

namespace prcnn {

constexpr int NMS_THREADS = 512;
constexpr int NMS_RCH = 8;         // rows per work item

// ---- quota form: max_keep <= NMS_QUOTA_MAX, or <= NMS_QUOTA_WIDE in its second instantiation (the proposal layer keeps 70 + 30 of up to 6300 + 2700 boxes per scene) ------------
// The lazy kernel below lets the kept rows of a block knock out EVERY later column before it moves on: 6236 columns x 64
// rows of IoUs after the first block of a 6300-box problem whose quota is reached inside the second block (0.22 ms, the
// longest kernel of the proposal stream).  Here the kept boxes (at most max_keep of them) stay in LDS and a block's 64 columns
// are tested against them when the block is staged: 64 x kept IoUs per block, nothing for columns that are never reached.
// Same decisions: a column is dropped iff an earlier KEPT row overlaps it (row, column argument order as nms_kernel :285).
// CAP = rows of the kept-box table, a template parameter: <NMS_QUOTA_MAX> is the inference form (70 + 30 kept; 7 KiB of table, 9.3 KiB
// of LDS in all), <NMS_QUOTA_WIDE> the training form (RPN_POST_NMS_TOP_N = 512: 358 + 154 kept at thresh 0.85, where little is
// suppressed and the lazy kernel's step D is at its worst; 14 KiB of table, 16.3 KiB of LDS).  One 512-thread workgroup per problem and
// 2 * B problems per launch: the grid never fills a CU's 160 KiB, so neither footprint bounds occupancy.  Same code for both.
constexpr int NMS_QUOTA_MAX = 256;
constexpr int NMS_QUOTA_WIDE = 512;

template <int CAP>
__global__ __launch_bounds__(NMS_THREADS) void nms_quota_kernel(
    int n_max, const int *__restrict__ counts, const float *__restrict__ boxes_all, float thresh,
    int max_keep, int *__restrict__ keep_all, int *__restrict__ num_keep_all)
{
    __shared__ float s_row[64 * 7];             // the 64 row boxes of the block
    __shared__ float s_kbox[CAP * 7];           // the kept boxes so far (same 7-float slots as s_row); max_keep <= CAP (nms_device)
    __shared__ unsigned long long s_diag[64];   // word(c): rows of the block with IoU > thresh, r < c
    __shared__ unsigned long long s_gone;       // columns of the block dropped by earlier kept rows
    __shared__ int s_nkeep;

    const int prob = blockIdx.x, t = threadIdx.x;
    const NmsProblem pb = nms_problem(prob, n_max, counts, max_keep);
    const int n = pb.n;
    const float *__restrict__ boxes = boxes_all + pb.boxes;
    int *__restrict__ keep = keep_all + pb.keep;
    for (int i = t; i < max_keep; i += NMS_THREADS) keep[i] = -1;
    if (t == 0) s_nkeep = 0;
    __syncthreads();

    const int nblocks = (n + 63) / 64;
    for (int rb = 0; rb < nblocks; ++rb) {
        const int r0 = rb * 64;
        const int rows = min(64, n - r0);
        const int nk0 = s_nkeep;                 // kept before this block
        stage_rows<false>(s_row, boxes, r0, rows, t);
        if (t < 64) s_diag[t] = 0ull;
        if (t == 0) s_gone = 0ull;
        __syncthreads();
        // A: the block's columns against the kept boxes of earlier blocks; B: against the earlier rows of the block itself.
        //    item = (column, chunk): 512 threads = 64 columns x 8 chunks
        {
            const int cl = t & 63, ch = t >> 6;
            if (cl < rows) {
                RBox C;
#pragma unroll
                for (int q = 0; q < 5; ++q) C.v[q] = s_row[cl * 7 + q];
                C.cosv = 1.f; C.sinv = 0.f;
                bool gone = false;
                for (int k = ch; k < nk0 && !gone; k += 8) gone = aabox_iou(&s_kbox[k * 7], C.v) > thresh;
                if (gone) atomicOr(&s_gone, 1ull << cl);
                const int rlo = ch * NMS_RCH, rhi = min(rlo + NMS_RCH, cl);
                unsigned long long w = 0;
                for (int r = rlo; r < rhi; ++r)
                    if (aabox_iou(&s_row[r * 7], C.v) > thresh) w |= 1ull << r;
                if (w) atomicOr(&s_diag[cl], w);
            }
        }
        __syncthreads();
        // C: serial resolve of the 64 rows; a kept row joins the kept-box table
        if (t == 0) {
            unsigned long long kept;
            s_nkeep = resolve_block64(s_gone, s_diag, rows, nk0, max_keep, kept, [&](int slot, int cl) {
#pragma unroll
                for (int q = 0; q < 5; ++q) s_kbox[slot * 7 + q] = s_row[cl * 7 + q];
                keep[slot] = r0 + cl;
            });
        }
        __syncthreads();
        if (s_nkeep >= max_keep) break;
    }
    if (t == 0) num_keep_all[prob] = s_nkeep;
}

// ---- lazy form (the design above): any n <= NMS_MAX_N, any quota, rotated or not ----
template <bool ROTATED>
__global__ __launch_bounds__(NMS_THREADS) void nms_lazy_kernel(
    int n_max, const int *__restrict__ counts, const float *__restrict__ boxes_all, float thresh,
    int max_keep, int *__restrict__ keep_all, int *__restrict__ num_keep_all)
{
    __shared__ float s_row[64 * 7];             // the 64 row boxes of the block (+cos,sin)
    __shared__ unsigned long long s_diag[64];   // word(c): rows of the block with IoU > thresh, r < c
    __shared__ unsigned long long s_kept;       // rows of the block that survive
    __shared__ unsigned int s_removed[NMS_MAX_N / 32];
    __shared__ int s_nkeep;

    const int prob = blockIdx.x, t = threadIdx.x;
    const NmsProblem pb = nms_problem(prob, n_max, counts, max_keep);
    const int n = pb.n;
    const float *__restrict__ boxes = boxes_all + pb.boxes;
    int *__restrict__ keep = keep_all + pb.keep;
    const int nblocks = (n + 63) / 64;

    for (int i = t; i < 2 * nblocks; i += NMS_THREADS) s_removed[i] = 0u;       // two words per block: step C reads a block's pair
    for (int i = t; i < max_keep; i += NMS_THREADS) keep[i] = -1;
    if (t == 0) s_nkeep = 0;
    __syncthreads();

    for (int rb = 0; rb < nblocks; ++rb) {
        const int r0 = rb * 64;
        const int rows = min(64, n - r0);
        // A: stage the row boxes
        stage_rows<ROTATED>(s_row, boxes, r0, rows, t);
        if (t < 64) s_diag[t] = 0ull;
        __syncthreads();

        // B: the block's own 64 columns; item = (column, chunk of NMS_RCH rows)
        {
            const int cl = t & 63, ch = t >> 6;  // 512 threads = 64 columns x 8 chunks
            if (cl < rows && !((s_removed[(r0 + cl) >> 5] >> ((r0 + cl) & 31)) & 1u)) {
                const int rlo = ch * NMS_RCH, rhi = min(rlo + NMS_RCH, cl);  // rows before the column
                if (rlo < rhi) {
                    const RBox C = load_col<ROTATED>(boxes + (long)(r0 + cl) * 5);
                    unsigned long long w = 0;
                    for (int r = rlo; r < rhi; ++r)
                        if (suppresses<ROTATED>(s_row, r, C, thresh)) w |= 1ull << r;
                    if (w) atomicOr(&s_diag[cl], w);
                }
            }
        }
        __syncthreads();

        // C: serial resolve of the 64 rows; the block's gone word is its two words of the removed bitmap (r0 is a multiple of 64)
        if (t == 0) {
            unsigned long long kept;
            const unsigned long long gone = ((unsigned long long)s_removed[2 * rb + 1] << 32) | s_removed[2 * rb];
            s_nkeep = resolve_block64(gone, s_diag, rows, s_nkeep, max_keep, kept, [&](int slot, int cl) { keep[slot] = r0 + cl; });
            s_kept = kept;
        }
        __syncthreads();
        if (s_nkeep >= max_keep) break;

        // D: kept rows knock out later columns
        const unsigned long long kept = s_kept;
        const int c_first = r0 + 64;
        const long items = (long)max(0, n - c_first) * (64 / NMS_RCH);
        for (long e = t; e < items; e += NMS_THREADS) {
            const int c = c_first + (int)(e / (64 / NMS_RCH));
            const int ch = (int)(e % (64 / NMS_RCH));
            const unsigned int chunk_bits = (unsigned int)((kept >> (ch * NMS_RCH)) & ((1u << NMS_RCH) - 1u));
            if (!chunk_bits) continue;
            if ((s_removed[c >> 5] >> (c & 31)) & 1u) continue;  // monotone flag: a stale 0 only costs work
            const RBox C = load_col<ROTATED>(boxes + (long)c * 5);
            for (int q = 0; q < NMS_RCH; ++q) {
                if (!((chunk_bits >> q) & 1u)) continue;
                if (suppresses<ROTATED>(s_row, ch * NMS_RCH + q, C, thresh)) {
                    atomicOr(&s_removed[c >> 5], 1u << (c & 31));
                    break;
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) num_keep_all[prob] = s_nkeep;
}

// ---- dense form for small problems (n <= ND_MAX: the FINAL rotated NMS of a scene runs over <= 100 boxes, eval_rcnn.py:626) --------
// The lazy kernel above is one workgroup per problem walking 64-row blocks: for 100 boxes its critical path is ~24 rotated IoUs
// evaluated one after the other by the same thread (175 us, the longest kernel of the final stage).  Here the reference's own
// split is used (iou3d_kernel.cu:250-292 + iou3d.cpp:100-119): every pair (row r, column c > r) is one IoU evaluated by its own
// thread -- 8 rows x 32 column lanes per workgroup, ~1.5 IoUs per thread -- into a 128-bit suppression mask per row, and one wave
// per problem then runs the host loop over the masks.  Same argument order (row, column), same expression: same keep list.
constexpr int ND_ROWS = 8, ND_LANES = 32;

template <bool ROTATED>
__global__ __launch_bounds__(ND_ROWS * ND_LANES) void nms_dense_mask_kernel(
    int n_max, const int *__restrict__ counts, const float *__restrict__ boxes_all, float thresh,
    unsigned long long *__restrict__ mask_all)
{
    __shared__ float s_row[ND_ROWS * 7];
    __shared__ unsigned long long s_mask[ND_ROWS][2];
    __shared__ float s_poly[ROTATED ? POLY_LDS_FLOATS * ND_ROWS * ND_LANES : 1];      // the clipped polygons (72 KB): see PolyLds
    const int prob = blockIdx.y, r0 = blockIdx.x * ND_ROWS;
    const NmsProblem pb = nms_problem(prob, n_max, counts, 0);
    const int n = pb.n;
    if (r0 >= n) return;
    const float *__restrict__ boxes = boxes_all + pb.boxes;
    const int t = threadIdx.x, rl = t / ND_LANES, cl = t % ND_LANES;
    const int rows = min(ND_ROWS, n - r0);
    stage_rows<ROTATED>(s_row, boxes, r0, rows, t);
    if (t < ND_ROWS * 2) s_mask[t >> 1][t & 1] = 0ull;
    __syncthreads();
    if (rl < rows) {
        unsigned long long w0 = 0ull, w1 = 0ull;
        for (int c = r0 + rl + 1 + cl; c < n; c += ND_LANES) {
            const RBox C = load_col<ROTATED>(boxes + (long)c * 5);
            if (suppresses<ROTATED, ROTATED>(s_row, rl, C, thresh, s_poly + t, ND_ROWS * ND_LANES)) {
                if (c < 64) w0 |= 1ull << c; else w1 |= 1ull << (c - 64);
            }
        }
        if (w0) atomicOr(&s_mask[rl][0], w0);
        if (w1) atomicOr(&s_mask[rl][1], w1);
    }
    __syncthreads();
    if (t < rows * 2) mask_all[((long)prob * ND_MAX + r0 + (t >> 1)) * 2 + (t & 1)] = s_mask[t >> 1][t & 1];
}

// one wave per problem: the host loop of iou3d.cpp:100-119 over the row masks
__global__ __launch_bounds__(64) void nms_dense_resolve_kernel(
    int n_max, const int *__restrict__ counts, const unsigned long long *__restrict__ mask_all, int max_keep,
    int *__restrict__ keep_all, int *__restrict__ num_keep_all)
{
    __shared__ unsigned long long s_m[ND_MAX][2];
    const int prob = blockIdx.x, t = threadIdx.x;
    const NmsProblem pb = nms_problem(prob, n_max, counts, max_keep);
    const int n = pb.n;
    int *__restrict__ keep = keep_all + pb.keep;
    for (int i = t; i < 2 * n; i += 64) s_m[i >> 1][i & 1] = mask_all[((long)prob * ND_MAX) * 2 + i];
    for (int i = t; i < max_keep; i += 64) keep[i] = -1;
    __syncthreads();
    if (t == 0) num_keep_all[prob] = resolve_mask128(s_m, n, max_keep, [&](int slot, int c) { keep[slot] = c; });
}

int nms_device(int nprob, int n_max, const int *counts, const float *boxes, float thresh,
               int rotated, int max_keep, int *keep, int *num_keep, hipStream_t st)
{
    PRCNN_REQUIRE(nprob >= 0 && n_max >= 0 && max_keep >= 0, "nms: bad sizes");
    PRCNN_REQUIRE(n_max <= NMS_MAX_N, "nms: %d boxes > %d unsupported", n_max, NMS_MAX_N);
    if (nprob == 0) return PRCNN_OK;
    PRCNN_REQUIRE(num_keep && (keep || max_keep == 0) && (boxes || n_max == 0), "nms: null pointer");
    if (n_max >= 1 && n_max <= ND_MAX) {
        // small problems (the final stage: <= 100 boxes per scene): all pairs at once + a one-wave resolve
        unsigned long long *mask = (unsigned long long *)scratch_for(st, (size_t)nprob * ND_MAX * 2 * sizeof(unsigned long long), 10);
        if (!mask) { set_error("nms: cannot allocate the mask scratch"); return PRCNN_ELAUNCH; }
        hipLaunchKernelGGL(by_rotation(rotated, nms_dense_mask_kernel<true>, nms_dense_mask_kernel<false>), dim3(ceil_div(n_max, ND_ROWS), nprob),
                           dim3(ND_ROWS * ND_LANES), 0, st, n_max, counts, boxes, thresh, mask);
        hipLaunchKernelGGL(nms_dense_resolve_kernel, dim3(nprob), dim3(64), 0, st, n_max, counts, mask, max_keep, keep, num_keep);
        return check_launch("nms(dense)");
    }
    auto kernel = by_rotation(rotated, nms_lazy_kernel<true>, nms_lazy_kernel<false>);
    if (!rotated && max_keep >= 1 && max_keep <= NMS_QUOTA_MAX) kernel = nms_quota_kernel<NMS_QUOTA_MAX>;
    else if (!rotated && max_keep > NMS_QUOTA_MAX && max_keep <= NMS_QUOTA_WIDE) kernel = nms_quota_kernel<NMS_QUOTA_WIDE>;       // the proposal layer's training quotas (<= 358 + 154)
    hipLaunchKernelGGL(kernel, dim3(nprob), dim3(NMS_THREADS), 0, st, n_max, counts, boxes, thresh, max_keep, keep, num_keep);
    return check_launch("nms");
}

}  // namespace prcnn

extern "C" int prcnn_nms_device(int nprob, int n_max, const int *counts, const float *boxes, float thresh,
                                int rotated, int max_keep, int *keep, int *num_keep, void *stream)
{
    return prcnn::nms_device(nprob, n_max, counts, boxes, thresh, rotated, max_keep, keep, num_keep, (hipStream_t)stream);
}
