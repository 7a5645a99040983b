// fps_common.hpp -- what the furthest-point-sampling units share (fps.hip, fps_spec.hip, fps_prefix.hip, point_groups.hip,
// roi_geometry.hip): the arg-max order of the reference's block reduction (the head of fps.hip states it) as wave reductions, the
// squared distance in both arithmetics, the tie-key codec, and the few host functions that one unit calls in another.
#pragma once
#include "common.hpp"
#include <math.h>

namespace prcnn {

// (v, key) beats (bv, bkey): larger value, ties -> smaller key.  Branchless on purpose: the
// short-circuit form compiles to exec-mask branches inside the hot loop.
__device__ __forceinline__ bool better(float v, uint32_t key, float bv, uint32_t bkey)
{
    return (v > bv) | ((v == bv) & (key < bkey));
}

__device__ __forceinline__ void take_if_better(float v, uint32_t key, float &bv, uint32_t &bkey)
{
    const bool t = better(v, key, bv, bkey);
    bv = t ? v : bv;
    bkey = t ? key : bkey;
}

template <int CTRL>
__device__ __forceinline__ int dpp_mov(int x)
{
    return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false);
}

template <int CTRL>
__device__ __forceinline__ void step_dpp(float &v, uint32_t &key)
{
    const float ov = __int_as_float(dpp_mov<CTRL>(__float_as_int(v)));
    const uint32_t ok = (uint32_t)dpp_mov<CTRL>((int)key);
    take_if_better(ov, ok, v, key);
}

// every lane of each 16-lane row ends up with the row's best (v, key): DPP only, no LDS
__device__ __forceinline__ void row16_argmax(float &v, uint32_t &key)
{
    step_dpp<0xB1>(v, key);   // quad_perm [1,0,3,2]  (lane ^ 1)
    step_dpp<0x4E>(v, key);   // quad_perm [2,3,0,1]  (lane ^ 2)
    step_dpp<0x141>(v, key);  // row_half_mirror: the two quads of an 8-lane group meet
    step_dpp<0x140>(v, key);  // row_mirror: the 8-lane halves of a 16-lane row meet
}

// wave-uniform best of the 64 lanes: rows reduced with DPP, the 4 row results read into SGPRs
__device__ __forceinline__ void wave_argmax(float &v, uint32_t &key)
{
    row16_argmax(v, key);
    float rv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    uint32_t rk = (uint32_t)__builtin_amdgcn_readlane((int)key, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float ov = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
        const uint32_t ok = (uint32_t)__builtin_amdgcn_readlane((int)key, r);
        take_if_better(ov, ok, rv, rk);
    }
    v = rv;
    key = rk;
}

// ---- two-pass arg-max: first the maximum VALUE (one v_max_f32 per candidate, one per DPP step), then the smallest key
// among the candidates that hold it (compare + select + v_min_u32).  Same total order as take_if_better -- larger value
// first, ties to the smaller key -- with a third of the instructions and much shorter dependency chains.
// The DPP permutation rides ON the max / min instruction (v_max_f32_dpp): one instruction per butterfly step.  Written as
// update_dpp + fmaxf the compiler emits v_mov, v_mov_dpp, a canonicalising v_max and the v_max -- 20 instructions for the four
// steps of a reduction that sits on the critical path of every FPS iteration.  (s_nop 1: a DPP operand written by the
// previous VALU instruction needs two wait states; the hazard recogniser does not look into inline assembly.)
#define PRCNN_DPP_OP(OP, TY, CTRL_TEXT)                                                                                       \
    asm("s_nop 1\n\t" OP " %0, %1, %1 " CTRL_TEXT " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v))
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v)
{
    float r;
    if constexpr (CTRL == 0xB1) PRCNN_DPP_OP("v_max_f32_dpp", float, "quad_perm:[1,0,3,2]");
    else if constexpr (CTRL == 0x4E) PRCNN_DPP_OP("v_max_f32_dpp", float, "quad_perm:[2,3,0,1]");
    else if constexpr (CTRL == 0x141) PRCNN_DPP_OP("v_max_f32_dpp", float, "row_half_mirror");
    else if constexpr (CTRL == 0x140) PRCNN_DPP_OP("v_max_f32_dpp", float, "row_mirror");
    else r = fmax_raw(v, __int_as_float(dpp_mov<CTRL>(__float_as_int(v))));
    return r;
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_min(uint32_t v)
{
    uint32_t r;
    if constexpr (CTRL == 0xB1) PRCNN_DPP_OP("v_min_u32_dpp", uint32_t, "quad_perm:[1,0,3,2]");
    else if constexpr (CTRL == 0x4E) PRCNN_DPP_OP("v_min_u32_dpp", uint32_t, "quad_perm:[2,3,0,1]");
    else if constexpr (CTRL == 0x141) PRCNN_DPP_OP("v_min_u32_dpp", uint32_t, "row_half_mirror");
    else if constexpr (CTRL == 0x140) PRCNN_DPP_OP("v_min_u32_dpp", uint32_t, "row_mirror");
    else {
        const uint32_t o = (uint32_t)dpp_mov<CTRL>((int)v);
        r = o < v ? o : v;
    }
    return r;
}
__device__ __forceinline__ float wave_max_f32(float v)        // wave-uniform result
{
    v = dpp_max<0xB1>(v); v = dpp_max<0x4E>(v); v = dpp_max<0x141>(v); v = dpp_max<0x140>(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)  // wave-uniform result
{
    v = dpp_min<0xB1>(v); v = dpp_min<0x4E>(v); v = dpp_min<0x141>(v); v = dpp_min<0x140>(v);
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    const uint32_t a = r0 < r1 ? r0 : r1, b = r2 < r3 ? r2 : r3;
    return a < b ? a : b;
}
// (value, key) of a wave as ONE unsigned 64-bit word whose integer order is the arg-max order: the value's bits made
// monotone (negative floats flipped, positive ones offset), the key complemented so that the smaller key is the larger
// word.  The workgroup's winner is then a single LDS atomic max per wave instead of an exchange + a 16-entry reduction.
__device__ __forceinline__ unsigned long long pack_candidate(float v, uint32_t key)
{
    const uint32_t b = (uint32_t)__float_as_int(v);
    const uint32_t mono = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)mono << 32) | (unsigned long long)(~key);
}
__device__ __forceinline__ void unpack_candidate(unsigned long long w, float &v, uint32_t &key)
{
    const uint32_t mono = (uint32_t)(w >> 32);
    const uint32_t b = (mono & 0x80000000u) ? (mono & 0x7fffffffu) : ~mono;
    v = __int_as_float((int)b);
    key = ~(uint32_t)w;
}

// The squared distance of sampling_gpu.cu:133, `(x2-x1)*(x2-x1) + (y2-y1)*(y2-y1) + (z2-z1)*(z2-z1)`.
// HIPCC = false: the source's arithmetic, one rounding per operation (the parity contract).
// HIPCC = true (prcnn_set_fps_arithmetic(1), round 4): the arithmetic of the reference's KERNEL BINARY as hipcc 7.2 builds that file
// for gfx950 with its default contraction -- read off the disassembly of oracle/_ref/pointnet2_kernels_ref.so, the same in all
// eleven block-size instantiations: v_pk_mul (dx^2, dz^2), v_fma dy*dy + dx^2, v_add + dz^2, i.e. (fma(dy, dy, dx*dx)) + dz*dz.
// With it the picks equal the reference kernel's on every cloud of tests/test_gpu_reference_kernels.py, near-ties included.
template <bool HIPCC>
__device__ __forceinline__ float fps_dist(float px, float py, float pz, float ox, float oy, float oz)
{
    if (!HIPCC) return sqdist3(px, py, pz, ox, oy, oz);
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    return __fadd_rn(__fmaf_rn(dy, dy, __fmul_rn(dx, dx)), __fmul_rn(dz, dz));
}

struct KeyCodec {
    int log2bs;  // virtual block = 1 << log2bs
    int sh;      // bits reserved for k >> log2bs
    int hipcc;   // 1: distances as the reference's hipcc-built binary computes them (fps_dist<true>); wave-uniform
    __device__ __forceinline__ uint32_t encode(int k) const
    {
        const uint32_t low = (uint32_t)k & ((1u << log2bs) - 1u);
        const uint32_t rev = log2bs ? (__brev(low) >> (32 - log2bs)) : 0u;
        return (rev << sh) | ((uint32_t)k >> log2bs);
    }
    __device__ __forceinline__ int decode(uint32_t key) const
    {
        const uint32_t hi = key >> sh;
        const uint32_t rev = log2bs ? (__brev(hi) >> (32 - log2bs)) : 0u;
        return (int)(((key & ((1u << sh) - 1u)) << log2bs) | rev);
    }
};

// ---- host side: what one unit calls in another (a kernel is launched by the unit that defines it: no relocatable device code)
// The tie-key layout of a cloud of n points: the reference's block size opt_n_threads(n) and the bits of k div bs above it; the
// arithmetic is the process-wide mode of prcnn_set_fps_arithmetic (fps.hip)
int fps_codec(int n, KeyCodec *kc);
// prcnn_fps_new_xyz behind its argument checks; rejected: see fps_any (fps.hip)
int fps_new_xyz_any(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream, const int *rejected);
// fps_order_kernel (fps.hip): perm (b, n) <- the clouds' Morton order; rejected (NULL: none): clouds to leave alone
void launch_fps_order(int b, int n, const float *xyz, int *perm, const int *rejected, hipStream_t st);
// fps_spec.hip: the speculative kernels behind fps_any's dispatch (sizes checked there).  fps2_capacity: how many workgroups of the
// two-workgroup kernel the device holds at once
int fps2_capacity();
int launch_fps_spec(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, float *new_xyz, const int *rejected, hipStream_t st);
int launch_fps_spec2(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, float *new_xyz, hipStream_t st);

}  // namespace prcnn
