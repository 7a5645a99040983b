// point_chains.hpp -- the per-point arithmetic of the KITTI loaders that more than one unit needs (csrc/input_stage.hip,
// csrc/aug_scene.hip): lidar -> rectified camera frame -> image, and the in-image / depth test, as the reference's numpy code
// evaluates them (pinned by tests/golden g11).  Moved out of input_stage.hip unchanged.
#pragma once
#include "common.hpp"

namespace prcnn {

struct SceneCalib {          // row-major, as calibration.py holds them
    float v2c[12];           // 3x4
    float r0[9];             // 3x3
    float p2[12];            // 3x4
    float img_h, img_w;
};

// lidar -> rectified frame -> image, validity, near / far class of ONE raw point, in the arithmetic the reference's numpy code
// performs (pinned by tests/golden g11, reference-executed): ``np.dot`` of float32 operands is a chain of fused multiply-adds
// over the inner index, first term a plain product -- for the tiny (4,3) = V2C^T . R0^T product of Calibration.lidar_to_rect
// (calibration.py:51-59) as well as for the (n,4) . (4,3) products; rect_to_img divides by the rect depth (0 -> 1e-9,
// calibration.py:66-68) and subtracts P2[2][3] for the depth; get_valid_flag (kitti_rcnn_dataset.py:201-222) compares in f32.
struct LidarToRect {
    float m[4][3];           // np.dot(V2C.T, R0.T)
    __device__ void set(const SceneCalib &cb)
    {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float acc = __fmul_rn(cb.v2c[i], cb.r0[3 * j]);                       // V2C^T[i][0] * R0^T[0][j]
                acc = __fmaf_rn(cb.v2c[4 + i], cb.r0[3 * j + 1], acc);
                m[i][j] = __fmaf_rn(cb.v2c[8 + i], cb.r0[3 * j + 2], acc);
            }
    }
    __device__ __forceinline__ float row(int j, float px, float py, float pz) const
    {
        float acc = __fmul_rn(px, m[0][j]);
        acc = __fmaf_rn(py, m[1][j], acc);
        acc = __fmaf_rn(pz, m[2][j], acc);
        return __fadd_rn(acc, m[3][j]);                                               // fma(1, m, acc)
    }
};

// A cloud of ONE point: numpy hands a (1, 4) . (4, 3) product to the BLAS's gemv kernels instead of gemm, and they sum in another
// order (OpenBLAS, as the fixtures' numpy ships it; csrc/gt_database.hip found the first form, csrc/aug_scene.hip the second).
// [p 1] . M with M contiguous (lidar_to_rect): two fused pairs, then their sum
__device__ __forceinline__ float gemv_row(float x, float y, float z, float m0, float m1, float m2, float m3)
{
    return __fadd_rn(__fmaf_rn(x, m0, __fmul_rn(y, m1)), __fmaf_rn(z, m2, m3));
}
// [p 1] . P2^T, a transposed operand (rect_to_img): the same two pairs without fused operations
__device__ __forceinline__ float gemv_row_t(float x, float y, float z, float m0, float m1, float m2, float m3)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(x, m0), __fmul_rn(y, m1)), __fadd_rn(__fmul_rn(z, m2), m3));
}

// rect_to_img (calibration.py:61-71) + the image half of get_valid_flag (kitti_rcnn_dataset.py:201-209): the point projects into the
// image and its rect depth is >= 0, compared in f32
__device__ __forceinline__ bool in_image(const SceneCalib &cb, float x, float y, float z)
{
    float hu = __fmul_rn(x, cb.p2[0]); hu = __fmaf_rn(y, cb.p2[1], hu); hu = __fmaf_rn(z, cb.p2[2], hu); hu = __fadd_rn(hu, cb.p2[3]);
    float hv = __fmul_rn(x, cb.p2[4]); hv = __fmaf_rn(y, cb.p2[5], hv); hv = __fmaf_rn(z, cb.p2[6], hv); hv = __fadd_rn(hv, cb.p2[7]);
    float hw = __fmul_rn(x, cb.p2[8]); hw = __fmaf_rn(y, cb.p2[9], hw); hw = __fmaf_rn(z, cb.p2[10], hw); hw = __fadd_rn(hw, cb.p2[11]);
    const float zz = (z == 0.f) ? 1e-9f : z;
    const float u = __fdiv_rn(hu, zz), v = __fdiv_rn(hv, zz);
    const float depth = __fsub_rn(hw, cb.p2[11]);
    return u >= 0.f && u < cb.img_w && v >= 0.f && v < cb.img_h && depth >= 0.f;
}

}  // namespace prcnn
