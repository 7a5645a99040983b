// eval_match.hip -- the evaluator's output transformations on the device (gfx950).
//
// evaluate/evaluate.py:130-230 asks one thing of the overlap matrix: for every detection the best-overlapping ground-truth box of its
// image and that overlap in BEV (np.max / np.argmax over axis 1), and the same for every ground-truth box (axis 0).
//
//   prcnn_bev_best_match   one launch over the segmented layout of prcnn_rotate_iou_eval_segmented; the (n x k) pair matrix is never
//                          written.  A ROW task is one box against the queries of its segment, a COLUMN task one query against the
//                          boxes of its segment; each task belongs to a group of MATCH_LANES lanes that stride the other side, keep a
//                          running (value, index) and finish with an in-wave argmax butterfly that breaks ties towards the lower
//                          index.  The pair value is rotate_iou_pair.hpp's pair_value with the arguments in the matrix kernel's order,
//                          so every value equals the matrix entry bit for bit.  Every pair is evaluated twice (once per side): the
//                          price of having no cross-task traffic at all.
//                          MATCH_LANES = 16: a KITTI val image is about 10 x 6, an RPN-mode folder a few hundred on a side.  Sixteen
//                          lanes keep 6..10 of 16 lanes busy on the former (a whole wave per row would keep 6..10 of 64) and cost a
//                          long row only four times the trips of a whole wave, with four rows in flight per wave instead.
//   prcnn_eval_align       evaluate.py:187-230 (align_size / align_front), f64, one thread per detection, -ffp-contract=off.
//                          np.linalg.norm of a 3-vector is sqrt(x.dot(x)), and that dot is OpenBLAS ddot: a forward chain of fused
//                          multiply-adds, first term a plain product (measured against numpy on 200 000 vectors: 0 differences; the
//                          unfused sum differs on 11 %).
#include "rotate_iou_pair.hpp"

namespace prcnn {

#define MATCH_LANES 16

// np.argmax order on (value, index): a NaN beats every number (np.max propagates it, np.argmax stops at the first), equal values go
// to the lower index.
__device__ __forceinline__ bool match_better(float v, int j, float bv, int bj)
{
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || j < bj);
    return v > bv || (v == bv && j < bj);
}

// last s in [0, nseg) with off[s] <= i: the segment that holds row i (empty segments share their offset with the next one)
__device__ __forceinline__ int segment_of(const int *__restrict__ off, int nseg, int i)
{
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void bev_best_match_kernel(int nseg, int n, int k, const int *__restrict__ box_off,
                                                             const int *__restrict__ q_off, const float *__restrict__ boxes,
                                                             const float *__restrict__ qboxes, int criterion,
                                                             float *__restrict__ row_val, int *__restrict__ row_idx,
                                                             float *__restrict__ col_val, int *__restrict__ col_idx)
{
    const long task = (long)blockIdx.x * (256 / MATCH_LANES) + threadIdx.x / MATCH_LANES;
    const int lane = threadIdx.x % MATCH_LANES;
    const long total = (long)n + (col_val ? k : 0);
    const bool active = task < total;                      // whole groups are active or not; nobody leaves before the butterfly
    const bool is_col = active && task >= n;
    const int self = active ? (int)(is_col ? task - n : task) : 0;
    int lo = 0, hi = 0;
    if (active) {
        const int s = segment_of(is_col ? q_off : box_off, nseg, self);
        const int *other = is_col ? box_off : q_off;
        lo = other[s];
        hi = other[s + 1];
    }
    const float *mine = (is_col ? qboxes : boxes) + 5 * (long)self;
    float bv = -INFINITY;
    int bj = 0x7fffffff;
    for (int j = lo + lane; j < hi; j += MATCH_LANES) {
        const float v = is_col ? pair_value(boxes + 5 * (long)j, mine, criterion) : pair_value(mine, qboxes + 5 * (long)j, criterion);
        if (match_better(v, j, bv, bj)) { bv = v; bj = j; }
    }
#pragma unroll
    for (int d = MATCH_LANES / 2; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(bv, d, MATCH_LANES);
        const int oj = __shfl_xor(bj, d, MATCH_LANES);
        if (match_better(ov, oj, bv, bj)) { bv = ov; bj = oj; }
    }
    if (active && lane == 0) {
        const bool any = hi > lo;
        (is_col ? col_val : row_val)[self] = any ? bv : 0.f;
        (is_col ? col_idx : row_idx)[self] = any ? bj - lo : -1;
    }
}

__global__ __launch_bounds__(256) void eval_align_kernel(int nseg, int n, const int *__restrict__ box_off, const int *__restrict__ q_off,
                                                         double *__restrict__ location, double *__restrict__ dimensions,
                                                         const double *__restrict__ alpha_in, const double *__restrict__ rotation_y,
                                                         const double *__restrict__ gt_dimensions, const float *__restrict__ row_val,
                                                         const int *__restrict__ row_idx, int mode, int *__restrict__ branch)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int code = -1;
    if ((double)row_val[j] > 0.2 && row_idx[j] >= 0) {             // the f32 maximum widened, against the f64 literal
        const int s = segment_of(box_off, nseg, j);
        const double *g = gt_dimensions + 3 * (long)(q_off[s] + row_idx[j]);
        double *dim = dimensions + 3 * (long)j, *loc = location + 3 * (long)j;
        code = 0;
        if (mode == 1) {
            double sq = loc[0] * loc[0];                           // np.linalg.norm: sqrt(ddot(x, x))
            sq = fma(loc[1], loc[1], sq);
            sq = fma(loc[2], loc[2], sq);
            const double dist = sqrt(sq);
            const double a = atan2(sin(alpha_in[j]), cos(alpha_in[j]));
            const double ry = rotation_y[j];
            const double pi = 3.141592653589793;
            if (fabs(sin(a)) * dist > dim[2] / 2.0) {
                const double shift = (dim[2] - g[2]) / 2.0;
                const double angle = 0 < a ? -ry : -ry + pi;
                code |= 1 | (0 < a ? 2 : 0);
                loc[0] += shift * cos(angle);
                loc[2] += shift * sin(angle);
            }
            if (fabs(cos(a)) * dist > dim[1] / 2.0) {
                const double shift = (dim[1] - g[1]) / 2.0;
                const bool inner = -pi / 2.0 < a && a < pi / 2.0;
                const double angle = inner ? -ry - pi / 2.0 : -ry + pi / 2.0;
                code |= 4 | (inner ? 8 : 0);
                loc[0] += shift * cos(angle);
                loc[2] += shift * sin(angle);
            }
        }
        dim[0] = g[0]; dim[1] = g[1]; dim[2] = g[2];
    }
    if (branch) branch[j] = code;
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_bev_best_match(int nseg, int n, int k, const int *box_off, const int *q_off, const float *boxes,
                                    const float *query_boxes, int criterion, float *row_val, int *row_idx, float *col_val,
                                    int *col_idx, void *stream)
{
    PRCNN_REQUIRE(nseg >= 0 && n >= 0 && k >= 0, "bev_best_match: bad sizes");
    PRCNN_REQUIRE(criterion >= -1 && criterion <= 2, "bev_best_match: criterion %d not in -1..2", criterion);
    PRCNN_REQUIRE((col_val == nullptr) == (col_idx == nullptr), "bev_best_match: col_val and col_idx go together");
    const long total = (long)n + (col_val ? k : 0);
    if (total == 0) return PRCNN_OK;
    PRCNN_REQUIRE(nseg > 0 && box_off && q_off, "bev_best_match: boxes without segments");
    PRCNN_REQUIRE(n == 0 || (boxes && row_val && row_idx), "bev_best_match: null row pointer");
    PRCNN_REQUIRE(k == 0 || query_boxes, "bev_best_match: null query pointer");
    hipLaunchKernelGGL(bev_best_match_kernel, dim3(ceil_div(total, 256 / MATCH_LANES)), dim3(256), 0, (hipStream_t)stream, nseg, n, k,
                       box_off, q_off, boxes, query_boxes, criterion, row_val, row_idx, col_val, col_idx);
    return check_launch("bev_best_match");
}

extern "C" int prcnn_eval_align(int nseg, int n, const int *box_off, const int *q_off, double *location, double *dimensions,
                                const double *alpha, const double *rotation_y, const double *gt_dimensions, const float *row_val,
                                const int *row_idx, int mode, int *branch, void *stream)
{
    PRCNN_REQUIRE(nseg >= 0 && n >= 0, "eval_align: bad sizes");
    PRCNN_REQUIRE(mode == 0 || mode == 1, "eval_align: mode %d is neither 0 (align_size) nor 1 (align_front)", mode);
    if (n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(nseg > 0 && box_off && q_off && location && dimensions && alpha && rotation_y && row_val && row_idx,
                  "eval_align: null pointer");
    hipLaunchKernelGGL(eval_align_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, nseg, n, box_off, q_off, location,
                       dimensions, alpha, rotation_y, gt_dimensions, row_val, row_idx, mode, branch);
    return check_launch("eval_align");
}
