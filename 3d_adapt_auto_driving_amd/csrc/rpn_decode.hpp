// rpn_decode.hpp -- the arithmetic of the bin-based box decode (decode_bbox_target, lib/utils/bbox_transform.py:24-127), written once for
// its three sites: rpn_decode_kernel (csrc/proposal.hip) and rcnn_decode_box (csrc/final_stage.hip), one lane per row, from the stored regression rows, and the
// decode inside the fused RPN tail (csrc/rpn_tail.hip rpn_tail_lin_kernel<true, *>: four lanes per row, from the rows where they stand in
// LDS; the RL_DEC_* blocks below).  One rounding per operation everywhere (__f*_rn: no contraction whatever the flags), in the
// reference's order.
#pragma once
#include "common.hpp"
#include <math.h>

namespace prcnn {

// centre of bin `bin` of a localisation target with bins of `size` over [-scope, scope): bin * size + size / 2 - scope
__device__ __forceinline__ float rd_bin_centre(int bin, float size, float scope)
{
    return __fsub_rn(__fadd_rn(__fmul_rn((float)bin, size), size / 2), scope);
}
// + the bin's normalised residual: centre + residual * size
__device__ __forceinline__ float rd_add_residual(float centre, float residual, float size) { return __fadd_rn(centre, __fmul_rn(residual, size)); }
// size from its anchor-normalised residual: v * a + a
__device__ __forceinline__ float rd_anchor_size(float v, float a) { return __fadd_rn(__fmul_rn(v, a), a); }
// arg-max over a row, first maximum, a NaN counts as the largest value (torch.argmax): does V displace the running best BV?  (A macro:
// as a function returning bool it compiled to other compares inside rpn_tail_lin_kernel<true, *>'s first stage, 2840 -> 2813 opcodes.)
#define RD_ARGMAX_TAKES(V, BV) ((V) > (BV) || ((V) != (V) && (BV) == (BV)))

// the arg-max of the two one-lane-per-row decoders, over n values in memory
__device__ __forceinline__ int argmax_row(const float *p, int n)
{
    int best = 0;
    float bv = p[0];
    for (int i = 1; i < n; ++i)                    // first maximum; a NaN counts as the largest value (torch.argmax)
        if (RD_ARGMAX_TAKES(p[i], bv)) { bv = p[i]; best = i; }
    return best;
}

// torch.remainder for f32: fmod, then shifted into the sign of the divisor
__device__ __forceinline__ float torch_remainder(float a, float b)
{
    float m = fmodf(a, b);
    if (m != 0.f && ((b < 0.f) != (m < 0.f))) m += b;
    return m;
}

// fmodf(a, (float)(2 pi)) WITHOUT the library's loop (the fused decode rides inside a hand-scheduled MFMA stage: no control flow).
// The remainder of two floats is exact in f32's own format, so it can be taken in f64: three reduction steps modulo b 2^80, b 2^40
// and b (b = the f32 value of 2 pi) -- each one q = trunc(r * (1 / B)), r = fma(-q, B, r): q < 2^46 is an exact integer that misses the
// true quotient by at most one, the fma's true result is a multiple of B's last bit below 2 B and therefore exact, and every step
// keeps r congruent to a modulo b -- then two corrective steps into [0, b), a's sign put back (a zero remainder takes it too, as
// fmod's does).  inf -> NaN and NaN -> NaN as fmodf.  Checked against fmodf in tests/test_gpu_packed.py through the fused decode:
// huge quotients up to 3e38, negatives, +-0, denormals, inf, NaN.
__device__ __forceinline__ float fmod_two_pi(float a)
{
    constexpr double B0 = (double)(float)(2.0 * M_PI), B1 = B0 * 1099511627776.0 /* 2^40 */, B2 = B1 * 1099511627776.0;
    constexpr double I0 = 1.0 / B0, I1 = 1.0 / B1, I2 = 1.0 / B2;
    double r = __builtin_fabs((double)a);
    r = __builtin_fma(-__builtin_trunc(r * I2), B2, r);
    r = __builtin_fma(-__builtin_trunc(r * I1), B1, r);
    r = __builtin_fma(-__builtin_trunc(r * I0), B0, r);
    r = r < 0.0 ? r + B0 : r;
    r = r < 0.0 ? r + B0 : r;
    r = r >= B0 ? r - B0 : r;
    r = r >= B0 ? r - B0 : r;
    return __builtin_copysignf((float)r, a);
}

#ifdef RPN_DECODE_SELFTEST          // the unit that owns the test entry prcnn_selftest_fmod_two_pi defines this
__global__ __launch_bounds__(256) void fmod_two_pi_selftest_kernel(long n, const float *__restrict__ a, float *__restrict__ mine,
                                                                   float *__restrict__ lib)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mine[i] = fmod_two_pi(a[i]);
    lib[i] = fmodf(a[i], (float)(2.0 * M_PI));
}
#endif

// ---- the decode inside the fused tail: the regression head's 76 outputs of a row are decoded where they stand in LDS (tile T1) --
// arg-max over the 12 x bins / 12 z bins / 12 heading bins, residual look-ups, anchor sizes: decode_bbox_target with get_xz_fine, then
// proposal_layer.py:31's y shift, in rpn_decode_kernel's f32 operation order -- and the 7-float box leaves instead of the 304-byte row.
// Four lanes per row (x | z | heading | y + sizes), 16 rows per wave, no control flow.  The layout is the shipped one only
// (12 + 12 + 12 + 12 + 1 + 12 + 12 + 3 = 76 channels: every cfgs/*.yaml); other layouts keep `reg`.
constexpr int RD_NB = 12;           // per_loc_bin_num = 2 * int(LOC_SCOPE / LOC_BIN_SIZE) = 2 * int(3.0 / 0.5), = NUM_HEAD_BIN

// the layouts the fused decode serves (prcnn_rpn_tail_boxes_supported)
static inline bool rd_layout_served(int channels, float loc_scope, float loc_bin_size, int num_head_bin, int xz_fine)
{
    return loc_bin_size > 0.f && (int)(loc_scope / loc_bin_size) * 2 == RD_NB && num_head_bin == RD_NB && xz_fine && channels == 6 * RD_NB + 4;
}

// lane = (row 16 w + lane / 4, part lane % 4); part 0: x, 1: z, 2: heading, 3: y + sizes.  Names expected in scope: a (RpnTailArgs), w,
// lane, T1 and RT_ROWS / RT_LD (mfma_stream.hpp); RL_DEC_STATE declares what the four steps keep between the k-groups they ride on.
#define RL_DEC_STATE                                                                                      \
    const int dpart = lane & 3;                                                                           \
    const float *drow = T1 + (16 * w + (lane >> 2)) * RT_LD;                                              \
    /* 12 values from here: bins | bins | bins | .. h w l */                                              \
    const int dstart = dpart == 0 ? 0 : dpart == 1 ? RD_NB : dpart == 2 ? 4 * RD_NB + 1 : 6 * RD_NB + 4 - RD_NB; \
    /* + bin: residual (part 3: the y offset) */                                                          \
    const int dexb = dpart == 0 ? 2 * RD_NB : dpart == 1 ? 3 * RD_NB : dpart == 2 ? 5 * RD_NB + 1 : 4 * RD_NB; \
    const int dxo = dpart == 0 ? 0 : dpart == 1 ? 2 : dpart == 2 ? 0 : 1;      /* which coordinate of the point */ \
    const int dbo = dpart == 0 ? 0 : dpart == 1 ? 2 : dpart == 2 ? 6 : 1;      /* which slot of the box */ \
    float dv[RD_NB], dp = 0.f, dex = 0.f, dout = 0.f, dh = 0.f, dw = 0.f, dl = 0.f;                       \
    int dbi = 0;
#define RL_DEC_READ(TT)                                                                                   \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < RD_NB; ++i) dv[i] = drow[dstart + i];                        \
        unsigned int gr_ = (unsigned int)(TT) * RT_ROWS + 16 * w + (lane >> 2);                           \
        if (gr_ >= (unsigned int)a.rows) gr_ = (unsigned int)a.rows - 1u;                                  \
        dp = a.xyz[gr_ * 3u + dxo];                                                                        \
    }
#define RL_DEC_ARGMAX                                                                                     \
    {                                                                                                     \
        float bv_ = dv[0];                                                                                \
        dbi = 0;                                                                                          \
        _Pragma("unroll") for (int i = 1; i < RD_NB; ++i) {                                                \
            const bool tk_ = RD_ARGMAX_TAKES(dv[i], bv_);                                                  \
            bv_ = tk_ ? dv[i] : bv_;                                                                      \
            dbi = tk_ ? i : dbi;                                                                          \
        }                                                                                                 \
        dex = drow[dexb + (dpart < 3 ? dbi : 0)];                                                          \
    }
#define RL_DEC_MATH                                                                                       \
    {                                                                                                     \
        const float fb_ = (float)dbi, bin_ = a.loc_bin_size;                                               \
        const float loc_ = __fadd_rn(rd_add_residual(rd_bin_centre(dbi, bin_, a.loc_scope), dex, bin_), dp); \
        const float apc_ = (float)((2.0 * M_PI) / RD_NB), apch_ = (float)(((2.0 * M_PI) / RD_NB) / 2.0);   \
        const float two_pi_ = (float)(2.0 * M_PI), pi_ = (float)M_PI;                                      \
        float ry_ = fmod_two_pi(__fadd_rn(__fmul_rn(fb_, apc_), __fmul_rn(dex, apch_)));                   \
        ry_ = (ry_ != 0.f && ry_ < 0.f) ? __fadd_rn(ry_, two_pi_) : ry_;                                   \
        ry_ = ry_ > pi_ ? __fsub_rn(ry_, two_pi_) : ry_;                                                   \
        dh = rd_anchor_size(dv[RD_NB - 3], a.anchor[0]);                                                   \
        dw = rd_anchor_size(dv[RD_NB - 2], a.anchor[1]);                                                   \
        dl = rd_anchor_size(dv[RD_NB - 1], a.anchor[2]);                                                   \
        const float y_ = __fadd_rn(__fadd_rn(dp, dex), dh / 2);                                            \
        dout = dpart < 2 ? loc_ : dpart == 2 ? ry_ : y_;                                                   \
    }
#define RL_DEC_STORE(TT, live)                                                                            \
    {                                                                                                     \
        const unsigned int gr_ = (unsigned int)(TT) * RT_ROWS + 16 * w + (lane >> 2);                     \
        if ((live) && gr_ < (unsigned int)a.rows) {                                                        \
            float *o_ = a.boxes + gr_ * 7u;                                                                \
            o_[dbo] = dout;                                                                                \
            if (dpart == 3) { o_[3] = dh; o_[4] = dw; o_[5] = dl; }                                        \
        }                                                                                                 \
    }
// spread over four k-groups of the NEXT tile's first stage, like the row stores it replaces
#define RL_DECODE(g, TT, live)                                                                            \
    if ((g) == 1) RL_DEC_READ(TT)                                                                         \
    else if ((g) == 3) RL_DEC_ARGMAX                                                                      \
    else if ((g) == 5) RL_DEC_MATH                                                                        \
    else if ((g) == 7) RL_DEC_STORE(TT, live)

}  // namespace prcnn
