// layer_tile.hpp -- what the f32 MFMA layer kernels of csrc/packed_layer.hip share: the problem record, the tile's shape, the 128-deep
// panel stage with a slot for side work, and the two ways a tile's results leave the accumulators.
//
// A tile is 64 rows x 128 k in LDS, rows padded to PL_LD = 132 floats; a workgroup of four waves computes 64 rows x 128 columns, wave w
// the columns 32 w .. 32 w + 31.  Lane (j, h) = (lane & 31, lane >> 5) supplies row j (acc0) and row 32 + j (acc1) of the A operand and
// column j of the B operand; h picks the k half: at step s the instruction's two k values are s (h = 0) and s + 64 (h = 1), so a lane
// holds wf[s] = W[k0 + s + 64 h][n0 + 32 w + j] for s = 0..63 and its four consecutive steps are 16 contiguous bytes of its row in LDS.
// C/D layout: column = j, row = (r & 3) + 8 (r >> 2) + 4 h for accumulator register r (+ 32 for acc1).
// For moving rows between memory and LDS a thread is (chunk, r0) = (tid & 31, tid >> 5): 16 bytes at column 4 chunk of rows r0 + 8 i.
// Summation order: panels in order, inside a panel k = s, s + 64 for s = 0..63 -- oracle/mlp_oracle.c orc_rows_layer_mfma.
//
// Macro or function, by the compiled kernels: the stages, the weight load, the tile fetch and PL_SADD are macros that expect j, h, chunk,
// r0, acc0 / acc1 and the buffer names (wrs, ars, lane_off, a_lane, row_bytes, a_row_bytes) in scope -- the side work is text that lands
// between two MFMAs of an unrolled loop, and packed_layer_persist_kernel sits at the register ceiling (251 VGPRs; 256 and 12 bytes of
// scratch with the addend), where the allocation moves with the form of these blocks (the fetch as a function: + 2 VGPRs in the pipe and
// stream kernels).  The epilogues are functions: with them inlined every kernel's MFMA stream is the hand-written one's.
#pragma once
#include "common.hpp"
#include "segmax.hpp"

namespace prcnn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int PL_ROWS = 64;
constexpr int PL_LD = 128 + 4;

// One layer problem; a launch of the batched kernels carries up to PL_MAX_BATCH of them (blockIdx.z picks): the independent scales of
// an MSG level run side by side in ONE launch instead of one small latency-bound launch each.
constexpr int PL_MAX_BATCH = 4;
struct PLProblem {
    const unsigned int *hdr; long rows_host; int K, N; const float *A; long lda; const float *W; const float *bias; int do_relu;
    float *out; long ldo; const unsigned int *rowinfo; const int *tilecloud; int m, out_col, n_store;
    int lds_pool;               // SEGMAX: tiles with many centres pool through the dead LDS tile (segmax.hpp); needs 16-byte aligned output rows
    // interpolation addend (prcnn_packed_layer_interp): out[r] = relu((A[r] @ W + bias) + ((w0 G[i0] + w1 G[i1]) + w2 G[i2])),
    // G (clouds, add_m, N-wide rows, leading dimension add_ldg), idx / weight (rows, 3), row r belongs to cloud r / add_n
    const float *addG; const int *addIdx; const float *addW; int add_n, add_m; long add_ldg;
};
struct PLBatch { PLProblem p[PL_MAX_BATCH]; };

#define PL_LOAD_W(dst, kk)                                                                              \
    _Pragma("unroll") for (int s = 0; s < 64; ++s)                                                      \
        dst[s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, lane_off, (unsigned int)((kk) + s) * row_bytes, 0));
// s_waitcnt vmcnt(0) (expcnt / lgkmcnt left alone): said explicitly so that the compiler's wait-count bookkeeping knows nothing
// older than the prefetch issued next is outstanding, and puts no wait between that prefetch and the MFMAs that hide it
#define PL_VM_DRAIN __builtin_amdgcn_s_waitcnt(0x0F70);
// (the scalar offsets of the 64 weight loads and the 8 row loads RUN -- one s_add each, opaque to the optimiser: written as products
//  of constants with row_bytes the compiler hoists all 72 of them into SGPRs of their own, and a kernel with anything else to keep in
//  scalar registers -- the persistent one -- spills them into VGPR lanes: 248 v_readlane / v_writelane inside the MFMA stream)
#define PL_SADD(x, y) asm volatile("s_add_u32 %0, %0, %1" : "+s"(x) : "s"(y) : "scc");

// rows r0 + 8 i (i < NI) of a tile, 16 bytes per thread and row, from the buffer `ars` at scalar offset soff into the LDS tile T
#define PL_FETCH_TILE(T, NI, soff)                                                                      \
    _Pragma("unroll") for (int i = 0; i < (NI); ++i)                                                    \
        *reinterpret_cast<f32x4 *>((T) + (r0 + 8 * i) * PL_LD + 4 * chunk) = __builtin_bit_cast(        \
            f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, a_lane, (soff) + (unsigned int)(8 * i) * a_row_bytes, 0));

// ---- one 128-deep panel = 16 k-groups of 8 MFMAs ---------------------------------------------------------------------
// A wave issues in order, and while it streams MFMAs the other waves of its SIMD get next to no VALU / address-generation
// slots (s_memtime stamps, profiles/r02_stage_stamps.md: two co-resident workgroups take turns, the time of a launch is the
// SUM of every wave's MFMA time and of its non-MFMA issue time).  So everything that is not an MFMA is placed INSIDE the
// MFMA stream of the wave that needs it, where the matrix pipe is busy anyway, and costs no VALU:
//   * the A operands of k-group g+1 are read from LDS before the MFMAs of group g;
//   * SIDE: the caller's side work of k-group g (g is a compile-time constant after unrolling), issued behind the group's first two
//     MFMAs and fenced from the other six; STATE declares what it keeps across groups.  PL_NO_SIDE: nothing, and no fence (with a
//     fence the plain stage's LDS reads are scheduled elsewhere in all six kernels that use it: same counts, another order);
//   * H2: PL_BOTH_HALVES keeps, PL_ONE_HALF drops the text of rows 32-63 (a1, acc1);
//   * PL_STAGE_HEAD reads the first group's operands, PL_STAGE_GROUPS is the rest.
#define PL_BOTH_HALVES(...) __VA_ARGS__
#define PL_ONE_HALF(...)
#define PL_MFMA(H2, wf, c, s)                                                                           \
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.c, wf[4 * g + s], acc0, 0, 0, 0);                    \
    H2(acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.c, wf[4 * g + s], acc1, 0, 0, 0);)
#define PL_STAGE_HEAD(T, H2)                                                                            \
    const float *a0p = (T) + j * PL_LD + 64 * h;                                                        \
    H2(const float *a1p = (T) + (32 + j) * PL_LD + 64 * h;)                                             \
    f32x4 a0 = *reinterpret_cast<const f32x4 *>(a0p);                                                   \
    H2(f32x4 a1 = *reinterpret_cast<const f32x4 *>(a1p);)
#define PL_STAGE_GROUPS(wf, H2, STATE, SIDE)                                                            \
    {                                                                                                   \
        STATE                                                                                           \
        _Pragma("unroll") for (int g = 0; g < 16; ++g) {                                                \
            f32x4 n0_ = a0;                                                                             \
            H2(f32x4 n1_ = a1;)                                                                         \
            if (g < 15) {                                                                               \
                n0_ = *reinterpret_cast<const f32x4 *>(a0p + 4 * (g + 1));                              \
                H2(n1_ = *reinterpret_cast<const f32x4 *>(a1p + 4 * (g + 1));)                          \
            }                                                                                           \
            __builtin_amdgcn_sched_barrier(0);                                                          \
            PL_MFMA(H2, wf, x, 0)                                                                       \
            SIDE                                                                                        \
            PL_MFMA(H2, wf, y, 1) PL_MFMA(H2, wf, z, 2) PL_MFMA(H2, wf, w, 3)                           \
            a0 = n0_;                                                                                   \
            H2(a1 = n1_;)                                                                               \
        }                                                                                               \
    }
#define PL_STAGE_SIDE(T, wf, STATE, SIDE) { PL_STAGE_HEAD(T, PL_BOTH_HALVES) PL_STAGE_GROUPS(wf, PL_BOTH_HALVES, STATE, SIDE) }
#define PL_FENCE __builtin_amdgcn_sched_barrier(0);
#define PL_NO_SIDE
#define PL_STAGE(T, wf) PL_STAGE_SIDE(T, wf, PL_NO_SIDE, PL_NO_SIDE)
// side work: the NEXT PANEL comes in behind this one -- its 8 rows of A as buffer loads from ARS (running scalar row offsets; rows
// past the end read as zero through the buffer's bounds check, no per-lane clamping) in groups 0-7, written to the OTHER LDS tile TN
// in groups 8-15; its 64 weights wn <- rows kn.. of the weight buffer at lane offset LOFF, six per group in groups 0-10.  Nothing is
// left for the end of the stage but one barrier.
#define PL_NEXT_PANEL_STATE(kn)                                                                         \
    f32x4 ar[8];                                                                                        \
    unsigned int wo_ = (unsigned int)(kn) * row_bytes;                                                  \
    unsigned int ao_ = (unsigned int)(kn) * 4u;                                                         \
    const unsigned int a8_ = 8u * a_row_bytes;
#define PL_NEXT_PANEL(TN, wn, ARS, LOFF)                                                                \
    if (g < 8) {                                                                                        \
        ar[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128((ARS), a_lane, ao_, 0)); \
        PL_SADD(ao_, a8_)                                                                               \
    } else                                                                                              \
        *reinterpret_cast<f32x4 *>((TN) + (r0 + 8 * (g - 8)) * PL_LD + 4 * chunk) = ar[g - 8];          \
    _Pragma("unroll") for (int q = 0; q < 6; ++q)                                                       \
        if (6 * g + q < 64) {                                                                           \
            wn[6 * g + q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, (LOFF), wo_, 0)); \
            PL_SADD(wo_, row_bytes)                                                                     \
        }                                                                                               \
    PL_FENCE
#define PL_STAGE_PREFETCH_X(T, TN, wf, wn, kn, ARS, LOFF) PL_STAGE_SIDE(T, wf, PL_NEXT_PANEL_STATE(kn), PL_NEXT_PANEL(TN, wn, ARS, LOFF))
#define PL_STAGE_PREFETCH(T, TN, wf, wn, kn) PL_STAGE_PREFETCH_X(T, TN, wf, wn, kn, ars, lane_off)
// side work: the NEXT ROW TILE of a K = 128 layer comes in behind this one (packed_layer_stream_kernel: the weights stay) -- 8 rows
// per thread as buffer loads at scalar offset `soff` in k-groups 0-7, written to the other LDS tile in k-groups 8-15
#define PL_NEXT_ROWS(TN, soff)                                                                          \
    if (g < 8)                                                                                          \
        ar[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                        \
            ars, a_lane, (soff) + (unsigned int)(8 * g) * a_row_bytes, 0));                             \
    else                                                                                                \
        *reinterpret_cast<f32x4 *>((TN) + (r0 + 8 * (g - 8)) * PL_LD + 4 * chunk) = ar[g - 8];          \
    PL_FENCE
#define PL_STAGE_ROWS(T, TN, wf, soff) PL_STAGE_SIDE(T, wf, f32x4 ar[8];, PL_NEXT_ROWS(TN, soff))

// The 32-row tiles (packed_layer_pipe32_kernel) use the two parts with PL_ONE_HALF: one accumulator (acc0) per wave, 64 MFMAs each
// waiting for the one before it; the head stands in front of that kernel's branch and both arms are fenced, as it was written.
// side work: the next panel of a 32-row tile -- 4 rows in groups 0-3, to LDS in groups 8-11, the weights six per group
#define PL32_NEXT_PANEL(TN, wn, kn)                                                                     \
    if (g < 4)                                                                                          \
        ar[g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(                        \
            ars, a_lane, (unsigned int)(8 * g) * a_row_bytes + (unsigned int)(kn) * 4u, 0));            \
    else if (g >= 8 && g < 12)                                                                          \
        *reinterpret_cast<f32x4 *>((TN) + (r0 + 8 * (g - 8)) * PL_LD + 4 * chunk) = ar[g - 8];          \
    _Pragma("unroll") for (int q = 0; q < 6; ++q)                                                       \
        if (6 * g + q < 64)                                                                             \
            wn[6 * g + q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(                       \
                wrs, lane_off, (unsigned int)((kn) + 6 * g + q) * row_bytes, 0));

// ---- epilogues
// DIRECT: act(acc + bcol) straight from the accumulators as buffer stores into the tile's own rows of `out`, lane (column `col` =
// n0 + 32 w + j, rows (r & 3) + 8 (r >> 2) + 4 h [+ 32]) -- no LDS staging, no barrier; rows past the end of a ragged last tile are
// outside the buffer and dropped by its bounds check: no per-lane compare, no 64-bit address arithmetic, and above all no wait in
// front of a store (a store under a per-lane condition made the compiler wait for vmcnt(0) -- i.e. for the store before it -- 32
// times per item).  Whole 128-column blocks without an addend only.
__device__ __forceinline__ void pl_store_direct(const f32x16 &acc0, const f32x16 &acc1, float bcol, int do_relu, float *out, long ldo,
                                                long t, long rows, unsigned int col)
{
    const int h = (threadIdx.x & 63) >> 5;
    const long left = rows - t * PL_ROWS;
    const unsigned int o_row_bytes = (unsigned int)ldo * 4u;
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(out + t * PL_ROWS * ldo), 0, (int)((left < PL_ROWS ? left : PL_ROWS) * (long)o_row_bytes), 0x00020000);
    const unsigned int o_lane = (unsigned int)(4 * h) * o_row_bytes + col * 4u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int so = (unsigned int)((r & 3) + 8 * (r >> 2)) * o_row_bytes;
        const float v0 = acc0[r] + bcol, v1 = acc1[r] + bcol;
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(do_relu ? fmaxf(v0, 0.f) : v0), ors, o_lane, so, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(do_relu ? fmaxf(v1, 0.f) : v1), ors, o_lane, so + 32u * o_row_bytes, 0);
    }
}

// STAGED, second half: the TR-row result tile in LDS -> rows t TR .. of out, columns n0 .. n0 + 127 cut at n_store (a head's last
// layer: N padded to 128 for the MFMA tiles, 1 / 46 / 76 real outputs): 16-byte stores when the row layout allows them, else scalar
// ones; rows >= `rows` are not stored.  with_add: + the interpolated coarse-level product, then the activation -- (w0 g0 + w1 g1) +
// w2 g2 per component with one rounding per operation (the order of three_interpolate, interpolate_gpu.cu:92-94), added to (acc +
// bias).
template <int TR>
__device__ __forceinline__ void pl_store_rows(const float *tile, long t, long rows, int n0, const PLProblem &pb, bool with_add)
{
    const int chunk = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    float *out = pb.out;
    const long ldo = pb.ldo;
    const int n_store = pb.n_store;
#pragma unroll
    for (int i = 0; i < TR / 8; ++i) {
        const int row = r0 + 8 * i;
        const long g = t * TR + row;
        if (g < rows) {
            const int c0 = n0 + 4 * chunk;
            float4 v = *reinterpret_cast<const float4 *>(tile + row * PL_LD + 4 * chunk);
            if (with_add) {
                const int *ix = pb.addIdx + g * 3;
                const float *wv = pb.addW + g * 3;
                const long cb = (g / pb.add_n) * (long)pb.add_m;
                const float4 g0 = *reinterpret_cast<const float4 *>(pb.addG + (cb + ix[0]) * pb.add_ldg + c0);
                const float4 g1 = *reinterpret_cast<const float4 *>(pb.addG + (cb + ix[1]) * pb.add_ldg + c0);
                const float4 g2 = *reinterpret_cast<const float4 *>(pb.addG + (cb + ix[2]) * pb.add_ldg + c0);
                const float w0 = wv[0], w1 = wv[1], w2 = wv[2];
                v.x = __fadd_rn(v.x, __fadd_rn(__fadd_rn(__fmul_rn(w0, g0.x), __fmul_rn(w1, g1.x)), __fmul_rn(w2, g2.x)));
                v.y = __fadd_rn(v.y, __fadd_rn(__fadd_rn(__fmul_rn(w0, g0.y), __fmul_rn(w1, g1.y)), __fmul_rn(w2, g2.y)));
                v.z = __fadd_rn(v.z, __fadd_rn(__fadd_rn(__fmul_rn(w0, g0.z), __fmul_rn(w1, g1.z)), __fmul_rn(w2, g2.z)));
                v.w = __fadd_rn(v.w, __fadd_rn(__fadd_rn(__fmul_rn(w0, g0.w), __fmul_rn(w1, g1.w)), __fmul_rn(w2, g2.w)));
                if (pb.do_relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
            }
            if (c0 + 4 <= n_store && (ldo & 3) == 0) {
                *reinterpret_cast<float4 *>(out + g * ldo + c0) = v;
            } else {
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (c0 + q < n_store) out[g * ldo + c0 + q] = e[q];
            }
        }
    }
}

// act(acc + bias) of the 64 x 128 block (t, n0) of problem pb: SEGMAX = false -> staged through the (dead) LDS tile for coalesced
// stores (pl_store_rows; the activation waits for the addend where there is one); SEGMAX = true -> segmented max over the tile's rows
// by centre, atomicMax into out[centre][out_col + n0 + ..]
template <bool SEGMAX>
__device__ __forceinline__ void pl_epilogue(const f32x16 &acc0, const f32x16 &acc1, float *tile, int *ctr, long t, long rows, int n0,
                                            const PLProblem &pb)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, h = lane >> 5;
    const int chunk = tid & 31;
    const float bcol = pb.bias[n0 + 32 * w + j];
    if constexpr (SEGMAX) {
        if (tid < PL_ROWS) {
            const unsigned int info = pb.rowinfo[t * PL_ROWS + tid];
            ctr[tid] = pb.tilecloud[t] * pb.m + (int)(info >> 16);
        }
        __syncthreads();
        const int myc = ctr[lane], prevc = ctr[lane ? lane - 1 : 0];
        const unsigned long long start = __ballot(lane == 0 || myc != prevc);
        if (!pb.lds_pool || __popcll(start) <= PK_LDS_MIN) {
            pk_segmented_max(acc0, acc1, ctr, start, h, pb.out, (int)pb.ldo, pb.out_col + n0 + 32 * w + j, bcol);
        } else {
            // many centres in the tile: row-major through the panel tile, which is dead (every wave is past the barrier above)
            const float4 bias4 = *reinterpret_cast<const float4 *>(pb.bias + n0 + 4 * chunk);
            pk_park(acc0, acc1, tile, PL_LD, 32 * w + j, h);
            lds_barrier();
            pk_segmented_max_lds(tile, PL_LD, ctr, tid, pb.out, (int)pb.ldo, pb.out_col + n0, bias4);
        }
    } else {
        const bool with_add = pb.addG != nullptr;
        const int do_relu = pb.do_relu;
        __syncthreads();                                   // the panel tile is dead: stage the results through it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v0 = acc0[r] + bcol, v1 = acc1[r] + bcol;
            tile[row * PL_LD + 32 * w + j] = (do_relu && !with_add) ? fmaxf(v0, 0.f) : v0;
            tile[(32 + row) * PL_LD + 32 * w + j] = (do_relu && !with_add) ? fmaxf(v1, 0.f) : v1;
        }
        __syncthreads();
        pl_store_rows<PL_ROWS>(tile, t, rows, n0, pb, with_add);
    }
}

}  // namespace prcnn
