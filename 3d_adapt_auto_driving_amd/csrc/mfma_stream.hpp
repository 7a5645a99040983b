// mfma_stream.hpp -- what the kernels share that keep a 64-row tile in LDS across several 128-wide layers and stream each layer's
// 128 x 32 weight slice per wave from L2 (csrc/rpn_tail.hip, csrc/rcnn_entrance.hip): the tile's shape, the panel stage with its slots
// for side work, the staged epilogue and the way a tile's rows leave LDS (the last two also serve csrc/rows_layer.hip).
//
// Names the macros expect in scope, and nothing else:
//   RT_LOAD_W, RT_STAGE*   j, h (lane & 31, lane >> 5), lane_off (= RT_LANE_OFF(32 * w + j)), acc0 and -- with RT_BOTH_HALVES -- acc1
//                          (f32x16 accumulators of rows 0-31 / 32-63); the weight matrix's buffer resource is the argument RS / rs
//   RT_EPILOGUE            j, h, w (the wave), acc0, acc1
//   RT_LANE_OFF            h;   RT_STORE_ROWS8: chunk, r0 (tid & 31, tid >> 5)
// Summation order: oracle/mlp_oracle.c (orc_rows_layer_mfma).
#pragma once
#include "common.hpp"

namespace prcnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int RT_ROWS = 64;          // rows per tile
constexpr int RT_LD = 128 + 4;       // LDS row stride in floats

// a lane's byte offset into a k-major weight matrix of 128 columns: row 64 h (its k half), column COL.  (A macro: as a function it moved
// a few LDS reads and MFMAs of rpn_tail_kernel and rpn_tail_lin_kernel<false, false> against each other.)
#define RT_LANE_OFF(COL) (((unsigned int)(64 * h) * 128u + (unsigned int)(COL)) * 4u)

// s_waitcnt vmcnt(0): said explicitly before every prefetch so that the compiler's wait-count bookkeeping knows nothing older
// is outstanding and puts no wait between the prefetch and the MFMAs that hide it (a vmcnt above 63 cannot be encoded)
#define RT_VM_DRAIN __builtin_amdgcn_s_waitcnt(0x0F70);
#define RT_LOAD_W(dst, rs, krow)                                                                          \
    _Pragma("unroll") for (int s = 0; s < 64; ++s)                                                        \
        dst[s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, lane_off, (unsigned int)((krow) + s) * 512u, 0)); \
    __builtin_amdgcn_sched_barrier(0);
// One 128-deep panel: 16 k-groups of 8 MFMAs.  A wave issues in order, so everything that is not an MFMA is placed where
// the matrix pipe is busy anyway:
//   * the A operands of group g+1 are read from LDS before the MFMAs of group g (a ds_read in front of its first use idles
//     the pipe for an LDS round trip per group);
//   * the 64 weight loads of the NEXT panel stage (wn <- rows krow.. of the weight buffer) go out four per group, behind
//     this group's first MFMAs, instead of 64 in a row in front of the stage (their issue alone was ~10 % of a stage);
//   * FIRST: the accumulators start from the inline constant 0 in the first MFMA (no 32 v_mov per stage);
//   * H2: RT_BOTH_HALVES keeps, RT_ONE_HALF drops the text of rows 32-63 (a1, acc1), as PL_STAGE_GROUPS does (layer_tile.hpp);
//   * LOAD2(g): a second load stream of the caller, issued with the group's weight loads (RT_NO_HOOK: none).
#define RT_BOTH_HALVES(...) __VA_ARGS__
#define RT_ONE_HALF(...)
#define RT_MFMA(H2, wf, c, s, c0, c1)                                                                     \
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.c, wf[s], c0, 0, 0, 0);                                \
    H2(acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.c, wf[s], c1, 0, 0, 0);)
#define RT_STAGE_X(T, wf, wn, RS, krow, FIRST, HOOK, LOFF, H2, LOAD2)                                     \
    {                                                                                                     \
        f32x4 a0 = *reinterpret_cast<const f32x4 *>((T) + j * RT_LD + 64 * h);                            \
        H2(f32x4 a1 = *reinterpret_cast<const f32x4 *>((T) + (32 + j) * RT_LD + 64 * h);)                 \
        _Pragma("unroll") for (int g = 0; g < 16; ++g) {                                                  \
            f32x4 n0 = a0;                                                                                \
            H2(f32x4 n1 = a1;)                                                                            \
            if (g < 15) {                                                                                 \
                n0 = *reinterpret_cast<const f32x4 *>((T) + j * RT_LD + 64 * h + 4 * (g + 1));            \
                H2(n1 = *reinterpret_cast<const f32x4 *>((T) + (32 + j) * RT_LD + 64 * h + 4 * (g + 1));) \
            }                                                                                             \
            __builtin_amdgcn_sched_barrier(0);                                                            \
            if ((FIRST) && g == 0) {                                                                      \
                const f32x16 zero = {0};                                                                  \
                RT_MFMA(H2, wf, x, 0, zero, zero)                                                         \
            } else {                                                                                      \
                RT_MFMA(H2, wf, x, 4 * g + 0, acc0, acc1)                                                 \
            }                                                                                             \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                 \
                wn[4 * g + q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(                     \
                    RS, (LOFF), (unsigned int)((krow) + 4 * g + q) * 512u, 0));                           \
            LOAD2(g)                                                                                      \
            __builtin_amdgcn_sched_barrier(0);                                                            \
            HOOK(g)                                                                                       \
            RT_MFMA(H2, wf, y, 4 * g + 1, acc0, acc1)                                                     \
            RT_MFMA(H2, wf, z, 4 * g + 2, acc0, acc1)                                                     \
            RT_MFMA(H2, wf, w, 4 * g + 3, acc0, acc1)                                                     \
            a0 = n0;                                                                                      \
            H2(a1 = n1;)                                                                                  \
        }                                                                                                 \
    }
//   * HOOK(g): side work of the caller issued behind the first two MFMAs of k-group g (g is a compile-time constant after
//     unrolling): a wave has ~14 free issue cycles behind every MFMA (profiles/r02_stage_stamps.md), enough for a few
//     instructions per group that would otherwise sit in a phase of their own in front of a stage
//   * LOFF: the lane's byte offset for the NEXT stage's weight slice (RT_STAGE_HOOK: lane_off, the slice this wave owns in every layer;
//     rpn_tail_lin_kernel's narrow last stage gives its waves other column blocks)
#define RT_NO_HOOK(g)
#define RT_STAGE_HOOK_LO(T, wf, wn, RS, krow, FIRST, HOOK, LOFF) RT_STAGE_X(T, wf, wn, RS, krow, FIRST, HOOK, LOFF, RT_BOTH_HALVES, RT_NO_HOOK)
#define RT_STAGE_HOOK(T, wf, wn, RS, krow, FIRST, HOOK) RT_STAGE_HOOK_LO(T, wf, wn, RS, krow, FIRST, HOOK, lane_off)
#define RT_STAGE(T, wf, wn, RS, krow, FIRST) RT_STAGE_HOOK(T, wf, wn, RS, krow, FIRST, RT_NO_HOOK)
// act(acc + bias) of this wave's 64 x 32 block -> tile T (the next layer's A operand, or the rows on their way out)
#define RT_EPILOGUE(T, bias, RELU)                                                                        \
    {                                                                                                     \
        const float bcol = (bias);                                                                        \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                  \
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;                                               \
            const float v0 = acc0[r] + bcol, v1 = acc1[r] + bcol;                                         \
            (T)[row * RT_LD + 32 * w + j] = (RELU) ? fmaxf(v0, 0.f) : v0;                                 \
            (T)[(32 + row) * RT_LD + 32 * w + j] = (RELU) ? fmaxf(v1, 0.f) : v1;                          \
        }                                                                                                 \
    }

// A tile's rows between memory and LDS: thread (chunk, r0) = (tid & 31, tid >> 5) moves 16 bytes at column 4 chunk of the tile rows
// r0 + 8 i, i < 8.  Tile T -> the rows ROW of the 128-wide matrix `out`, ROW an expression in i (and row = r0 + 8 i) that names the
// i-th of the thread's eight rows: a tile's own, a tile map's, a row list's.  V = float4 or f32x4, as each kernel was written: the same
// 16 bytes, but the allocation moves with the type (rows_layer_kernel<2, ..> 242 -> 256 VGPRs with f32x4, rcnn_entrance_kernel 235 -> 241
// with float4).  A macro: as a function over an array of row numbers it moved the LDS reads of rows_layer_kernel's panel (198 -> 162).
#define RT_STORE_ROWS8(V, T, out, ROW)                                                                      \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                       \
        const int row = r0 + 8 * i;                                                                       \
        *reinterpret_cast<V *>((out) + (ROW) * 128 + 4 * chunk) = *reinterpret_cast<const V *>((T) + row * RT_LD + 4 * chunk); \
    }

}  // namespace prcnn
