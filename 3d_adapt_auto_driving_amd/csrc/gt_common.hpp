// gt_common.hpp -- the point-in-box test of the GT-database, augmented-scene and training-input kernels (csrc/gt_database.hip,
// csrc/aug_scene.hip, csrc/train_input.hip, csrc/placement.hpp): roipool3d.cpp:82-95 as csrc/roipool_host.hip restates it, over a
// staged box record.  Moved out of gt_database.hip unchanged (the arithmetic is described there; pinned by tests/golden g18).
#pragma once
#include "common.hpp"
#include <math.h>

namespace prcnn {

constexpr int GT_CHUNK = 64;                     // boxes per LDS chunk (gt_database.py BOX_CHUNK mirrors it)
constexpr int GT_REC = 8;                        // floats per staged box: cx, cy, cz, h/2, l/2, w/2, cos, sin

// box [x, y_bottom, z, h, w, l, ry] with its host-made (cos ry, sin ry) and its height h (the caller may have enlarged it) -> record
__device__ __forceinline__ void gt_box_record(const float *bx, float h, float cosv, float sinv, float *o)
{
    const float hh = __fmul_rn(h, 0.5f);
    o[0] = bx[0]; o[1] = __fsub_rn(bx[1], hh); o[2] = bx[2];
    o[3] = hh; o[4] = __fmul_rn(bx[5], 0.5f); o[5] = __fmul_rn(bx[4], 0.5f);
    o[6] = cosv; o[7] = sinv;
}

__device__ __forceinline__ bool gt_inside(const float *o, const float4 r)
{
    const float dx = __fsub_rn(r.x, o[0]), dy = __fsub_rn(r.y, o[1]), dz = __fsub_rn(r.z, o[2]);
    const bool reject = fabsf(dx) > 10.0f || fabsf(dy) > o[3] || fabsf(dz) > 10.0f;
    const float xr = __fadd_rn(__fmul_rn(dx, o[6]), __fmul_rn(dz, -o[7]));
    const float zr = __fadd_rn(__fmul_rn(dx, o[7]), __fmul_rn(dz, o[6]));
    return !reject && xr >= -o[4] && xr <= o[4] && zr >= -o[5] && zr <= o[5];
}

}  // namespace prcnn
