// rotate_iou.hip -- rotated IoU matrix of the KITTI AP evaluator (K18) for gfx950.
//
// Reference behaviour restated: evaluate/rotate_iou.py:16-291 (numba.cuda).  Boxes are in centre
// format [cx, cy, w, h, angle].  numba's typing is followed: f32 (op) f32 stays f32, an f32
// divided by an integer literal is evaluated in f64 and rounded when stored to an f32 array, the
// polygon area accumulates in f64.  One lane per (box, query) pair; the matrix is small
// (tens..hundreds per side per part, eval2.py:352-380) so no tiling is needed.
#include "rotate_iou_pair.hpp"

namespace prcnn {

__global__ __launch_bounds__(256) void rotate_iou_kernel(int n, int k, const float *__restrict__ boxes,
                                                         const float *__restrict__ qboxes,
                                                         float *__restrict__ iou, int criterion)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)n * k) return;
    const int i = (int)(e / k), j = (int)(e - (long)i * k);
    iou[e] = pair_value(boxes + 5 * i, qboxes + 5 * j, criterion);
}

// Block-diagonal form: segment s pairs boxes[box_off[s]..box_off[s+1]) with qboxes[q_off[s]..q_off[s+1]) only
// and writes its row-major (n_s, k_s) block at out_off[s].  The reference evaluates ~50 dense "parts" of ~75
// images each to amortise launches (eval2.py:352-424) and discards the cross-image pairs; here every image
// is a segment and the whole split is one launch that computes only the pairs the evaluator reads.
__global__ __launch_bounds__(256) void rotate_iou_segmented_kernel(int nseg, const long long *__restrict__ out_off,
                                                                   const int *__restrict__ box_off,
                                                                   const int *__restrict__ q_off,
                                                                   const float *__restrict__ boxes,
                                                                   const float *__restrict__ qboxes,
                                                                   float *__restrict__ iou, int criterion)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= out_off[nseg]) return;
    int lo = 0, hi = nseg;                       // last s with out_off[s] <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (out_off[mid] <= e) lo = mid; else hi = mid;
    }
    const int k = q_off[lo + 1] - q_off[lo];
    const long long local = e - out_off[lo];
    const int i = (int)(local / k), j = (int)(local - (long long)i * k);
    iou[e] = pair_value(boxes + 5 * (long)(box_off[lo] + i), qboxes + 5 * (long)(q_off[lo] + j), criterion);
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_rotate_iou_eval(int n, int k, const float *boxes, const float *query_boxes,
                                     float *iou, int criterion, void *stream)
{
    PRCNN_REQUIRE(n >= 0 && k >= 0, "rotate_iou_eval: bad sizes");
    PRCNN_REQUIRE(criterion >= -1 && criterion <= 2, "rotate_iou_eval: criterion %d not in -1..2", criterion);
    if (n == 0 || k == 0) return PRCNN_OK;
    PRCNN_REQUIRE(boxes && query_boxes && iou, "rotate_iou_eval: null pointer");
    hipLaunchKernelGGL(rotate_iou_kernel, dim3(ceil_div((long)n * k, 256)), dim3(256), 0, (hipStream_t)stream,
                       n, k, boxes, query_boxes, iou, criterion);
    return check_launch("rotate_iou_eval");
}

/* Block-diagonal rotated IoU: nseg segments; box_off / q_off (nseg+1) i32 prefix offsets into boxes / query_boxes,
 * out_off (nseg+1) i64 prefix of n_s*k_s; all three in DEVICE memory; total = out_off[nseg] given by the host. */
extern "C" int prcnn_rotate_iou_eval_segmented(int nseg, long long total, const long long *out_off, const int *box_off,
                                               const int *q_off, const float *boxes, const float *query_boxes,
                                               float *iou, int criterion, void *stream)
{
    PRCNN_REQUIRE(nseg >= 0 && total >= 0, "rotate_iou_eval_segmented: bad sizes");
    PRCNN_REQUIRE(criterion >= -1 && criterion <= 2, "rotate_iou_eval_segmented: criterion %d not in -1..2", criterion);
    if (nseg == 0 || total == 0) return PRCNN_OK;
    PRCNN_REQUIRE(out_off && box_off && q_off && boxes && query_boxes && iou, "rotate_iou_eval_segmented: null pointer");
    PRCNN_REQUIRE(total <= 0x7fffffffLL * 256, "rotate_iou_eval_segmented: %lld pairs exceed the launch grid", total);
    hipLaunchKernelGGL(rotate_iou_segmented_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, nseg, out_off, box_off, q_off, boxes, query_boxes, iou, criterion);
    return check_launch("rotate_iou_eval_segmented");
}
