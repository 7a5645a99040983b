// point_chains.hpp -- the per-point arithmetic of the KITTI loaders that more than one unit needs (csrc/input_stage.hip,
// csrc/gt_database.hip, csrc/aug_scene.hip, csrc/train_input.hip): lidar -> rectified camera frame -> image, the in-image / depth
// test, and the valid-point filter built from them, as the reference's numpy code evaluates them (pinned by tests/golden g11).
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
// kitti_io.Calibration.lidar_to_rect of one raw point with the host's M = np.dot(V2C.T, R0.T), (4, 3) row-major (csrc/gt_database.hip,
// csrc/road_planes.hip): product, two fused multiply-adds, one add; ``single``: the cloud has ONE point (the gemv form above)
__device__ __forceinline__ void lidar_to_rect_m(const float *m, const float4 p, bool single, float v[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (single) {
            v[j] = gemv_row(p.x, p.y, p.z, m[j], m[3 + j], m[6 + j], m[9 + j]);
            continue;
        }
        float a = __fmul_rn(p.x, m[j]);
        a = __fmaf_rn(p.y, m[3 + j], a);
        a = __fmaf_rn(p.z, m[6 + j], a);
        v[j] = __fadd_rn(a, m[9 + j]);
    }
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

// The valid-point filter of ONE raw point (generate_aug_scene.py:241-249, kitti_rcnn_dataset.py:251-274 get_rpn_sample): -> its rect
// coordinates and whether it is in the image, at depth >= 0 and inside ``scope`` (x, y, z ranges; null: no range test).  ``single``:
// the scene has ONE point, so numpy took the gemv forms above.  ``is_rect``: the point is in the rect frame already.  The reference
// compares the f32 coordinates with a float64 scope (70.4 is not an f32): compared in double.
__device__ __forceinline__ bool rect_valid_point(const float4 p, const SceneCalib &cb, bool single, bool is_rect, const double *scope,
                                                 float &x, float &y, float &z)
{
    x = p.x; y = p.y; z = p.z;
    if (!is_rect) {
        LidarToRect l2r;
        l2r.set(cb);
        if (single) {
            x = gemv_row(p.x, p.y, p.z, l2r.m[0][0], l2r.m[1][0], l2r.m[2][0], l2r.m[3][0]);
            y = gemv_row(p.x, p.y, p.z, l2r.m[0][1], l2r.m[1][1], l2r.m[2][1], l2r.m[3][1]);
            z = gemv_row(p.x, p.y, p.z, l2r.m[0][2], l2r.m[1][2], l2r.m[2][2], l2r.m[3][2]);
        } else {
            x = l2r.row(0, p.x, p.y, p.z); y = l2r.row(1, p.x, p.y, p.z); z = l2r.row(2, p.x, p.y, p.z);
        }
    }
    bool ok;
    if (single) {
        const float hu = gemv_row_t(x, y, z, cb.p2[0], cb.p2[1], cb.p2[2], cb.p2[3]);
        const float hv = gemv_row_t(x, y, z, cb.p2[4], cb.p2[5], cb.p2[6], cb.p2[7]);
        const float hw = gemv_row_t(x, y, z, cb.p2[8], cb.p2[9], cb.p2[10], cb.p2[11]);
        const float zz = (z == 0.f) ? 1e-9f : z;
        const float u = __fdiv_rn(hu, zz), v = __fdiv_rn(hv, zz);
        ok = u >= 0.f && u < cb.img_w && v >= 0.f && v < cb.img_h && __fsub_rn(hw, cb.p2[11]) >= 0.f;
    } else {
        ok = in_image(cb, x, y, z);
    }
    if (scope)
        ok = ok && (double)x >= scope[0] && (double)x <= scope[1] && (double)y >= scope[2] && (double)y <= scope[3] &&
             (double)z >= scope[4] && (double)z <= scope[5];
    return ok;
}

}  // namespace prcnn
