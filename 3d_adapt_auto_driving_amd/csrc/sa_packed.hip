// sa_packed.hip -- set-abstraction MLP over the DISTINCT grouped rows only (the row lists of csrc/ball_pack.hip).
//
// The fused gather -> layer 1 -> layer 2 (MFMA) -> layer 3 (MFMA) -> max kernel of sa_mlp_fused.hip over the list's 64-row tiles: a
// tile now holds rows of SEVERAL centres, so the max over nsample becomes a segmented max -- done in the accumulator registers with a
// wave-uniform boundary mask, or through LDS when the tile holds many centres (segmax.hpp) -- and partial maxima reach the output with
// atomicMax (outputs are >= 0 after ReLU, so the integer order of the bit patterns is the float order).
//
// Every row's result is the same k-ordered fma chain as in sa_mlp_fused.hip (a row's MFMA result does not depend on the
// other rows of its tile), so the output is BIT-IDENTICAL to the unpacked kernel's; only duplicates are skipped.
//
// The three kernels share their blocks (sa_tile.hpp) and the order of a tile's stages, one line each in the tile loop:
//   builder (layer 1 into A1) | next tile's list entries | layer 2 panel | its epilogue into Y1 | next tile's P rows | layer 3 panel | pool
// They differ in the weight-register layout and in which wave owns which block, and stay three kernels for that.
#include "common.hpp"
#include "sa_tile.hpp"
#include "segmax.hpp"

namespace prcnn {

#ifndef PK_PF
#define PK_PF 4                    // rows of P per thread the 128-wide kernel gathers one tile ahead
#endif
constexpr int PK_TILES_PER_WG = 8;

// Round 5: ONE launch serves up to two PROBLEMS (the two scales of an MSG level: their own row lists, weights and output slices):
// workgroup x works on problem x % nprob and draws its tiles from that problem's counter (words 0 and 2 of the launch's ticket record).
// On the sparse launches of the real step (1-2 tiles per CU) a launch is mostly ramp: two of them side by side cost one ramp.
struct SaPkProblem {
    int n, m;
    const unsigned int *hdr;
    const float4 *rowdxyz, *P, *wxyz;
    const unsigned int *rowinfo;
    const int *tilecloud;
    const float *w2t, *b2, *w3t, *b3;
    float *out;
    int out_stride, out_col, lds_pool;
    int c1, c2;                       // the real widths of layers 1 and 2 (the arrays are zero-padded to 128 whatever they are)
};
struct SaPkBatch {
    int nprob;
    SaPkProblem p[2];
};

// ---- the builder: layer 1 of the tile's rows into A1, R rows per thread (r0 + (64 / R) i), and the output row of every tile row into
// cc.  The first NPF rows of P were gathered one tile ahead (pb), the others are gathered here.
template <int R, int NPF>
__device__ __forceinline__ void sa_pk_build(const SaRowCodec &cd, const float4 *__restrict__ P, const unsigned int (&info)[R],
                                            const float4 (&pb)[NPF], int cloud, int n, int m, int chunk, int r0, const float4 wx,
                                            const float4 wy, const float4 wz, const float4 *dcur, float *A1, int *cc)
{
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int row = r0 + (PK_ROWS / R) * i;
        const float4 d = dcur[row];
        const float4 base = i < NPF ? pb[i < NPF ? i : 0] : sa_gather_p(cd, P, info[i], cloud, n, chunk);
        const float4 v = affine_relu4(base, wx, wy, wz, d.x, d.y, d.z);
        *reinterpret_cast<float4 *>(A1 + row * PK_LD + 4 * chunk) = v;
        if (chunk == 0) cc[row] = (int)(cd.cloud(info[i], cloud) * m + cd.centre(info[i]));
    }
}

// ---- the pool of a 128-wide tile: segmented max of this wave's 64 x 32 block, in registers -- or, for a tile of many centres, through
// LDS, row-major (segmax.hpp).  A1 is free (last read in layer 2, two barriers ago).
__device__ __forceinline__ void sa_pk_pool128(const f32x16 &acc0, const f32x16 &acc1, const int *cc, float *A1, int lds_pool,
                                              const float *__restrict__ b3, float bias3, float *__restrict__ out, int out_stride, int out_col,
                                              int tid, int lane, int w, int j, int h)
{
    const unsigned long long start = sa_segment_starts(cc, lane);
    if (!lds_pool || __popcll(start) <= PK_LDS_MIN) {
        pk_segmented_max(acc0, acc1, cc, start, h, out, out_stride, out_col + 32 * w + j, bias3);
    } else {
        const float4 bias4 = *reinterpret_cast<const float4 *>(b3 + 4 * (tid & 31));
        pk_park(acc0, acc1, A1, PK_LD, 32 * w + j, h);
        lds_barrier();
        pk_segmented_max_lds(A1, PK_LD, cc, tid, out, out_stride, out_col, bias4);
        lds_barrier();                                 // the next builder rewrites A1
    }
}

// ------------------------------------------------------------------------------------------------ C3 = 128, layers 64-64 / 64-96
// Round 5, third session: the two scales of RPN SA2 (64-64-128 and 64-96-128 after the per-point layer; tools/cfgs/default.yaml's
// SA_CONFIG.MLPS[1]) arrive zero-padded to 128-128-128, and the padded kernel spends 256 MFMAs per wave and tile where 96 / 160 carry
// non-zero operands.  A padded chain is  acc = fma(a[s], w[s], acc); acc = fma(a[s + 64], w[s + 64], acc)  for s = 0..63 (the
// instruction's two k values in that order); with zeros at k >= K a second step is  fma(0, 0, acc) = acc,  so the chain IS the
// chain over the real k in this order:  K = 64: k = 0, 1, 2, ... 63;  K = 96: k = 0, 64, 1, 65, ... 31, 95, then 32, 33, ... 63.
// Fed to the instruction as pairs -- K = 64: step s takes k = 2s (lanes 0-31) and 2s + 1 (lanes 32-63), 32 steps;  K = 96:
// steps 0-31 as before (s, s + 64), then 16 steps (32 + 2u, 33 + 2u) -- the result is the padded chain's, bit for bit (an
// accumulator of -0 would come out of fma(0, 0, -0) as +0: no chain that starts from +0 gets there short of products below
// 1e-45).  Layer 2 of the 64-wide scale has 2 x 2 blocks of 32 x 32: one per wave; the 96-wide one leaves wave 3 idle.  The tile
// builder works on 64 channels: 16 float4 chunks x 16 row slots, four rows per thread, ALL of them gathered one tile ahead.
template <int C2>
__device__ __forceinline__ void sa_pk128_narrow(const SaPkProblem &q, unsigned int *__restrict__ ticket, int tiles_per_wg, float *lds,
                                                unsigned int *slot, int (*ctr)[PK_ROWS], float4 (*dxyz_s)[PK_ROWS])
{
    static_assert(C2 == 64 || C2 == 96, "layer 2 of RPN SA2");
    float *A1 = lds, *Y1 = lds + PK_ROWS * PK_LD;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int n = q.n, m = q.m;
    const unsigned int *__restrict__ hdr = q.hdr;
    const float4 *__restrict__ rowdxyz = q.rowdxyz;
    const float4 *__restrict__ P = q.P, *__restrict__ wxyz = q.wxyz;
    const unsigned int *__restrict__ rowinfo = q.rowinfo;
    const int *__restrict__ tilecloud = q.tilecloud;
    const float *__restrict__ w2t = q.w2t, *__restrict__ b2 = q.b2, *__restrict__ w3t = q.w3t, *__restrict__ b3 = q.b3;
    float *__restrict__ out = q.out;
    const int out_stride = q.out_stride, out_col = q.out_col, lds_pool = q.lds_pool;
    const SaRowCodec cd(hdr, false);                                  // (the batch entry refuses lists without tilecloud)
    const long tiles = cd.tiles;

    __syncthreads();                                                  // (a second attempt reuses the slots and the tile buffers)
    long t = sa_first_ticket(slot, ticket, tid);
    if (t >= tiles) return;

    constexpr int S3 = C2 / 2;                                        // MFMA steps of layer 3
    const int cb2 = C2 == 64 ? (w & 1) : w, rb2 = w >> 1;             // layer 2: column block; C2 == 64: row block as well
    float wf2[32], wf3[S3];
#pragma unroll
    for (int s = 0; s < 32; ++s) wf2[s] = w2t[(long)(2 * s + h) * PK_C + 32 * cb2 + j];
#pragma unroll
    for (int s = 0; s < S3; ++s) {
        const int k = C2 == 64 ? 2 * s + h : (s < 32 ? s + 64 * h : 32 + 2 * (s - 32) + h);
        wf3[s] = w3t[(long)k * 128 + 32 * w + j];
    }
    const float bias2 = b2[32 * cb2 + j], bias3 = b3[32 * w + j];

    const int chunk = tid & 15, r0 = tid >> 4;
    const float4 wx = wxyz[chunk], wy = wxyz[32 + chunk], wz = wxyz[64 + chunk];
    unsigned int info[4];
    int cloud = 0;
    float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f);
    sa_fetch_rows<4>(cd, rowinfo, tilecloud, rowdxyz, t, r0, tid, info, cloud, d0);
    if (tid < PK_ROWS) dxyz_s[0][tid] = d0;
    float4 pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);
    __syncthreads();

    for (int served = 0; served < tiles_per_wg && t < tiles; ++served) {
        sa_next_ticket(slot, ticket, tid, served, tiles_per_wg);
        int *cc = ctr[served & 1];
        sa_pk_build<4, 4>(cd, P, info, pb, cloud, n, m, chunk, r0, wx, wy, wz, dxyz_s[served & 1], A1, cc);
        __syncthreads();
        const long t_next = slot[(served + 1) & 1];
        float4 dnext = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t_next < tiles) sa_fetch_rows<4>(cd, rowinfo, tilecloud, rowdxyz, t_next, r0, tid, info, cloud, dnext);   // in flight during layer 2

        // ---- layer 2: K = 64 as 32 steps of (2s, 2s + 1)
        if (C2 == 64) {
            f32x16 acc = {0};
            SA_PAIRS1(A1, rb2, 0, wf2, 0, 16, acc)
            SA_STORE_RELU(Y1, rb2, 32 * cb2 + j, acc, bias2)
        } else if (w < 3) {
            f32x16 acc0 = {0}, acc1 = {0};
            SA_PAIRS2(A1, 0, wf2, 0, 16, acc0, acc1)
            SA_STORE_RELU2(Y1, 32 * w + j, acc0, acc1, bias2)
        }
        if (tid < PK_ROWS && t_next < tiles) dxyz_s[(served + 1) & 1][tid] = dnext;   // ordered before the next builder by the barrier below
        if (t_next < tiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);      // in flight during layer 3
        }
        __syncthreads();

        // ---- layer 3 (K = C2) + segmented max over the tile's rows
        {
            f32x16 acc0 = {0}, acc1 = {0};
            if (C2 == 96) SA_PANEL2(Y1, wf3, 8, acc0, acc1)
            constexpr int K0 = C2 == 96 ? 32 : 0, S0 = C2 == 96 ? 32 : 0;       // the (2u, 2u + 1) steps: k from K0, weights from S0
            SA_PAIRS2(Y1, K0, wf3, S0, (S3 - S0) / 2, acc0, acc1)
            sa_pk_pool128(acc0, acc1, cc, A1, lds_pool, b3, bias3, out, out_stride, out_col, tid, lane, w, j, h);
        }
        t = t_next;
    }
}

// ------------------------------------------------------------------------------------------------ C3 = 128
// Two workgroups per CU (see sa_mlp_fused.hip for the MFMA mapping; identical here).
template <int NPROB, bool NARROW = false>
__global__ __launch_bounds__(256, 2) void sa_packed_mlp128_kernel(const SaPkBatch batch, unsigned int *__restrict__ rec, int tiles_per_wg)
{
    __shared__ float lds[2 * PK_ROWS * PK_LD];
    __shared__ unsigned int slot[2];
    __shared__ int ctr[2][PK_ROWS];
    // the centre-relative coordinates of a tile's rows stream from HBM (16 B per row, read once): they are fetched ONE TILE
    // AHEAD by wave 0 and parked here, so that the builder finds them in LDS instead of waiting for memory
    __shared__ float4 dxyz_s[2][PK_ROWS];
    float *A1 = lds, *Y1 = lds + PK_ROWS * PK_LD;

    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    // a workgroup starts on problem x % nprob and, when that problem's tiles have run out, moves on to the other one (it reloads the
    // weights once): the tile counts live on the device, so the split of the launch's workgroups between the problems cannot be
    // chosen on the host -- LiDAR-shaped scenes give the two scales of RPN SA2 27 % and 73 % of the rows
    // (NPROB = 1, every single-problem launch: no loop, the kernel of rounds 2-4 register for register)
    const int pi0 = NPROB > 1 ? (int)(blockIdx.x % (unsigned)NPROB) : 0;
#pragma unroll 1
    for (int attempt = 0; attempt < NPROB; ++attempt) {
    const int pi = NPROB > 1 ? __builtin_amdgcn_readfirstlane(pi0 + attempt < NPROB ? pi0 + attempt : pi0 + attempt - NPROB) : 0;   // provably uniform: the problem's fields stay in SGPRs
    const SaPkProblem &q = batch.p[pi];
    if (NARROW) {                                                     // the scales of RPN SA2: every problem of the launch has c1 = 64, c2 in {64, 96}
        if (q.c2 == 64) sa_pk128_narrow<64>(q, rec + 2 * pi, tiles_per_wg, lds, slot, ctr, dxyz_s);
        else sa_pk128_narrow<96>(q, rec + 2 * pi, tiles_per_wg, lds, slot, ctr, dxyz_s);
        continue;
    }
    const int n = q.n, m = q.m;
    const unsigned int *__restrict__ hdr = q.hdr;
    const float4 *__restrict__ rowdxyz = q.rowdxyz;
    const float4 *__restrict__ P = q.P /* (b,n,128) */, *__restrict__ wxyz = q.wxyz /* (3,128) */;
    const unsigned int *__restrict__ rowinfo = q.rowinfo;
    const int *__restrict__ tilecloud = q.tilecloud;
    const float *__restrict__ w2t = q.w2t, *__restrict__ b2 = q.b2, *__restrict__ w3t = q.w3t, *__restrict__ b3 = q.b3;
    float *__restrict__ out = q.out;
    const int out_stride = q.out_stride, out_col = q.out_col, lds_pool = q.lds_pool;
    unsigned int *__restrict__ ticket = rec + 2 * pi;                 // this problem's draw counter
    const SaRowCodec cd(hdr, tilecloud == nullptr);                   // tilecloud == NULL: a list whose ROWS carry their cloud
    const long tiles = cd.tiles;

    // first ticket BEFORE the weights are fetched: the grid is sized for the worst case (every ball full) and most
    // workgroups of a sparse launch leave right here
    __syncthreads();                                                  // (a second attempt reuses the slots and the tile buffers)
    long t = sa_first_ticket(slot, ticket, tid);
    if (t >= tiles) continue;

    float wf2[64], wf3[64];
    SA_LOAD_PANEL(wf2, w2t, PK_C, 32 * w + j)
    SA_LOAD_PANEL(wf3, w3t, 128, 32 * w + j)
    const float bias2 = b2[32 * w + j], bias3 = b3[32 * w + j];

    const int chunk = tid & 31, r0 = tid >> 5;
    const float4 wx = wxyz[chunk], wy = wxyz[32 + chunk], wz = wxyz[64 + chunk];

    unsigned int info[8];
    int cloud = 0;
    float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f);
    sa_fetch_rows<8>(cd, rowinfo, tilecloud, rowdxyz, t, r0, tid, info, cloud, d0);
    if (tid < PK_ROWS) dxyz_s[0][tid] = d0;
    // half of the tile's 8 rows of P per thread are gathered ONE TILE AHEAD (behind layer 3's MFMAs; all 8 do not fit the
    // register budget next to the 128 resident weights: 164 bytes of spills, slower on sparse tiles): the builder's wait for its
    // gathers was 12-15k of a tile's 50k cycles (s_memtime stamps, profiles/r02_stage_stamps.md)
    float4 pb[PK_PF];
#pragma unroll
    for (int i = 0; i < PK_PF; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);
    __syncthreads();

    for (int served = 0; served < tiles_per_wg && t < tiles; ++served) {
        sa_next_ticket(slot, ticket, tid, served, tiles_per_wg);
        int *cc = ctr[served & 1];
        sa_pk_build<8, PK_PF>(cd, P, info, pb, cloud, n, m, chunk, r0, wx, wy, wz, dxyz_s[served & 1], A1, cc);
        __syncthreads();
        const long t_next = slot[(served + 1) & 1];
        float4 dnext = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t_next < tiles) sa_fetch_rows<8>(cd, rowinfo, tilecloud, rowdxyz, t_next, r0, tid, info, cloud, dnext);   // in flight during layer 2

        // ---- layer 2
        {
            f32x16 acc0 = {0}, acc1 = {0};
            SA_PANEL2(A1, wf2, 16, acc0, acc1)
            SA_STORE_RELU2(Y1, 32 * w + j, acc0, acc1, bias2)
        }
        if (tid < PK_ROWS && t_next < tiles) dxyz_s[(served + 1) & 1][tid] = dnext;   // ordered before the next builder by the barrier below
        if (t_next < tiles) {
#pragma unroll
            for (int i = 0; i < PK_PF; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);   // in flight during layer 3
        }
        __syncthreads();

        // ---- layer 3 + segmented max over the tile's rows
        {
            f32x16 acc0 = {0}, acc1 = {0};
            SA_PANEL2(Y1, wf3, 16, acc0, acc1)
            sa_pk_pool128(acc0, acc1, cc, A1, lds_pool, b3, bias3, out, out_stride, out_col, tid, lane, w, j, h);
        }
        // A1 is rewritten by the next builder only (every wave has left layer 2); Y1 after the next tile's first barrier;
        // the centre list alternates between two buffers, so a slow wave still reads this tile's list while the others
        // already write the next one.
        t = t_next;
    }
    }   // attempt
    if (tid == 0) ticket_release3(rec);          // the launch's last workgroup zeroes the counters for the record's next user
}

// ------------------------------------------------------------------------------------------------ C3 = 256
// Eight waves (sa_mlp_fused256_kernel's mapping): wave (wp, wg) owns column panel wp of layer 2 for row half wg, and column
// panel wp of column tile wg of layer 3 for both row halves.
__global__ __launch_bounds__(512, 1) void sa_packed_mlp256_kernel(
    int n, int m, const unsigned int *__restrict__ hdr, const float4 *__restrict__ rowdxyz,
    const float4 *__restrict__ P, const float4 *__restrict__ wxyz, const unsigned int *__restrict__ rowinfo,
    const int *__restrict__ tilecloud, const float *__restrict__ w2t, const float *__restrict__ b2,
    const float *__restrict__ w3t /* (128,256) */, const float *__restrict__ b3, float *__restrict__ out, int out_stride,
    int out_col, unsigned int *__restrict__ ticket, int tiles_per_wg, int lds_pool)
{
    __shared__ float lds[2 * PK_ROWS * PK_LD];
    __shared__ unsigned int slot[2];
    __shared__ int ctr[2][PK_ROWS];
    __shared__ float4 dxyz_s[2][PK_ROWS];             // next tile's coordinates, fetched one tile ahead (see the 128 kernel)
    float *A1 = lds, *Y1 = lds + PK_ROWS * PK_LD;
    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6, wp = w & 3, wg = w >> 2;
    const int j = lane & 31, h = lane >> 5;
    const SaRowCodec cd(hdr, tilecloud == nullptr);
    const long tiles = cd.tiles;

    long t = sa_first_ticket(slot, ticket, tid);
    if (t >= tiles) { if (tid == 0) ticket_release(ticket); return; }

    float wf2[64], wf3[64];
    SA_LOAD_PANEL(wf2, w2t, PK_C, 32 * wp + j)
    SA_LOAD_PANEL(wf3, w3t, 256, 128 * wg + 32 * wp + j)
    const float bias2 = b2[32 * wp + j], bias3 = b3[128 * wg + 32 * wp + j];

    const int chunk = tid & 31, r0 = tid >> 5;       // rows r0 + 16 i, i < 4
    const float4 wx = wxyz[chunk], wy = wxyz[32 + chunk], wz = wxyz[64 + chunk];

    unsigned int info[4];
    int cloud = 0;
    float4 d0 = make_float4(0.f, 0.f, 0.f, 0.f);
    sa_fetch_rows<4>(cd, rowinfo, tilecloud, rowdxyz, t, r0, tid, info, cloud, d0);
    if (tid < PK_ROWS) dxyz_s[0][tid] = d0;
    // the tile's 4 rows of P per thread are gathered ONE TILE AHEAD (behind layer 3's MFMAs): the builder used to wait for them,
    // a quarter of a tile's cycles (s_memtime stamps of the 128-wide kernel, profiles/r02_stage_stamps.md)
    float4 pb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);
    __syncthreads();

    for (int served = 0; served < tiles_per_wg && t < tiles; ++served) {
        sa_next_ticket(slot, ticket, tid, served, tiles_per_wg);
        int *cc = ctr[served & 1];
        sa_pk_build<4, 4>(cd, P, info, pb, cloud, n, m, chunk, r0, wx, wy, wz, dxyz_s[served & 1], A1, cc);
        __syncthreads();
        const long t_next = slot[(served + 1) & 1];
        float4 dnext = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t_next < tiles) sa_fetch_rows<4>(cd, rowinfo, tilecloud, rowdxyz, t_next, r0, tid, info, cloud, dnext);

        // ---- layer 2: rows [32 wg, 32 wg + 32) x columns [32 wp, 32 wp + 32)
        {
            f32x16 acc = {0};
            SA_PANEL1(A1, wg, wf2, acc)
            SA_STORE_RELU(Y1, wg, 32 * wp + j, acc, bias2)
        }
        if (tid < PK_ROWS && t_next < tiles) dxyz_s[(served + 1) & 1][tid] = dnext;
        if (t_next < tiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pb[i] = sa_gather_p(cd, P, info[i], cloud, n, chunk);      // in flight during layer 3
        }
        __syncthreads();

        // ---- layer 3: all 64 rows x columns [128 wg + 32 wp, +32), then the segmented max
        {
            f32x16 acc0 = {0}, acc1 = {0};
            SA_PANEL2(Y1, wf3, 16, acc0, acc1)
            const unsigned long long start = sa_segment_starts(cc, lane);
            if (!lds_pool || __popcll(start) <= PK_LDS_MIN) {
                pk_segmented_max(acc0, acc1, cc, start, h, out, out_stride, out_col + 128 * wg + 32 * wp + j, bias3);
            } else {
                // many centres in the tile: through LDS, row-major (segmax.hpp), one 64 x 128 tile per column tile: A1 is free
                // (last read in layer 2), Y1 once every wave has left layer 3
                float *Z = wg ? Y1 : A1;
                const float4 bias4 = *reinterpret_cast<const float4 *>(b3 + 128 * wg + 4 * (tid & 31));
                lds_barrier();
                pk_park(acc0, acc1, Z, PK_LD, 32 * wp + j, h);
                lds_barrier();
                pk_segmented_max_lds(Z, PK_LD, cc, tid & 255, out, out_stride, out_col + 128 * wg, bias4);
                lds_barrier();                                 // the next builder rewrites A1
            }
        }
        t = t_next;
    }
    if (tid == 0) ticket_release(ticket);          // the launch's last workgroup zeroes the counter for the word's next user
}

}  // namespace prcnn

using namespace prcnn;

// Workgroups of a launch whose problems have max_tiles tiles at most each; *per_wg <- the tiles a workgroup serves before it retires.
// Persistent workgroups: at most 512 per launch, shared by its `share` problems or halves (the 256-wide kernel's workgroups are two
// of the 128-wide one's) (round 4: 1024 / 512 until then -- the sweep 256 / 384 / 512 / 640 / 768 / 1024 at K = 96 gave 6546 / 6633 /
// 6639 / 6625 / 6638 / 6591 scenes/s, LiDAR-shaped 4752 / 4788 / 4775 / 4753 / 4729 / 4733: two resident workgroups per CU hold the LDS
// of 512, a second round only queues), each drawing tiles from the ticket counter until none is left, so the 128 weight registers per
// lane are loaded once per workgroup.  (Until round 2 a workgroup served at most 8 tiles and the grid was sized for the worst case --
// every ball full: in the sparse launches of the real step, ~2300 live tiles of 102400, some 2300 DIFFERENT workgroups each fetched
// 128 KB of weights to serve one tile.  RCNN SA1 at the B = 8 shape: 244 -> 160 us.)  PRCNN_SA_GRID=<n> overrides the cap,
// PRCNN_SA_GRID=0 restores the 8-tiles-per-workgroup launch.
static long sa_pk_grid(long max_tiles, int share, int *per_wg)
{
    static const int env_grid = getenv("PRCNN_SA_GRID") ? atoi(getenv("PRCNN_SA_GRID")) : 512;
    *per_wg = PK_TILES_PER_WG;
    long grid = (max_tiles + PK_TILES_PER_WG - 1) / PK_TILES_PER_WG;
    if (env_grid > 0) {
        const long cap = (env_grid + share - 1) / share;
        if (grid > cap) grid = cap;
        *per_wg = 1 << 30;
    }
    return grid;
}

// One problem of either entry (`what` names it in the refusals): checked, its output slice zeroed, *p <- the kernels' view of it.
// *live <- 0 when there is nothing to launch for it: only the single entry accepts such a problem, and a list without tilecloud.
static int sa_pk_problem(const char *what, bool single, const prcnn_sa_problem &q, hipStream_t st, SaPkProblem *p, int *live)
{
    *live = 0;
    PRCNN_REQUIRE(q.n <= 65536 && q.m <= 65536, "%s: cloud too large for the 16-bit row descriptors", what);
    PRCNN_REQUIRE(q.out_stride >= q.out_col + q.c3 && q.out_col >= 0, "%s: bad output slice", what);
    if (single && (long)q.b * q.m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(single || ((long)q.b * q.m > 0 && q.max_tiles > 0), "%s: empty problem (use prcnn_sa_packed_mlp)", what);
    PRCNN_REQUIRE(q.P && q.wxyz && q.rowinfo && q.rowdxyz && (q.tilecloud || single) && q.hdr && q.w2t && q.b2 && q.w3t && q.b3 && q.out,
                  "%s: null pointer", what);
    // tilecloud == NULL: the rows carry their cloud (descriptor (cloud << 16) | (centre << 9) | point; prcnn_rcnn_roi_geometry_packs)
    PRCNN_REQUIRE(q.tilecloud || (q.n <= 512 && q.m <= 128 && q.b <= 65536), "%s: a list without tilecloud holds clouds of <= 512 points, <= 128 centres", what);
    PRCNN_REQUIRE((((uintptr_t)q.P | (uintptr_t)q.wxyz) & 15) == 0, "%s: 16-byte alignment required", what);
    if (!q.out_is_zero && hipMemset2DAsync(q.out + q.out_col, (size_t)q.out_stride * sizeof(float), 0, (size_t)q.c3 * sizeof(float), (size_t)q.b * q.m, st) != hipSuccess) {
        set_error("%s: cannot zero the output slice", what);
        return PRCNN_ELAUNCH;
    }
    if (q.max_tiles == 0) return PRCNN_OK;
    // row-major pooling through LDS needs 16-byte aligned output rows (else every tile stays on the register form)
    const int lds_pool = (((uintptr_t)q.out | (uintptr_t)q.b3) & 15) == 0 && q.out_stride % 4 == 0 && q.out_col % 4 == 0;
    *p = SaPkProblem{q.n, q.m, q.hdr, (const float4 *)q.rowdxyz, (const float4 *)q.P, (const float4 *)q.wxyz, q.rowinfo, q.tilecloud,
                     q.w2t, q.b2, q.w3t, q.b3, q.out, q.out_stride, q.out_col, lds_pool, 128, 128};
    *live = 1;
    return PRCNN_OK;
}

// The fused set-abstraction MLP over packed rows (prcnn_ball_pack): P (b,n,128) = features @ W1f^T + b1, wxyz (3,128),
// w2t (128,128), w3t (128,c3) k-major, c3 in {128, 256}; out[(b*m rows)][out_col .. out_col + c3), row stride out_stride.
// The output slice is zeroed by this call and then receives max over each centre's distinct rows of relu(layer 3).
// max_tiles = b * ceil(m * nsample / 64) sizes the grid (the real tile count stays on the device, in hdr[0]).
extern "C" int prcnn_sa_packed_mlp(int b, int n, int m, int c3, long max_tiles, const float *P, const float *wxyz,
                                   const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud,
                                   const unsigned int *hdr, const float *w2t, const float *b2, const float *w3t,
                                   const float *b3, float *out, int out_stride, int out_col, int out_is_zero, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && max_tiles >= 0, "sa_packed_mlp: bad sizes");
    PRCNN_REQUIRE(c3 == 128 || c3 == 256, "sa_packed_mlp: unsupported output width %d (128 | 256)", c3);
    hipStream_t st = (hipStream_t)stream;
    const prcnn_sa_problem q = {b, n, m, c3, max_tiles, P, wxyz, rowinfo, rowdxyz, tilecloud, hdr, w2t, b2, w3t, b3, out, out_stride, out_col, out_is_zero, 0, 0};
    SaPkBatch batch;
    int live;
    const int rc = sa_pk_problem("sa_packed_mlp", true, q, st, &batch.p[0], &live);
    if (rc != PRCNN_OK || !live) return rc;
    int per_wg;
    const int grid = (int)sa_pk_grid(max_tiles, c3 == 128 ? 1 : 2, &per_wg);
    unsigned int *ticket = next_ticket(st);
    if (!ticket) { set_error("sa_packed_mlp: cannot set up the tile ticket"); return PRCNN_ELAUNCH; }
    if (c3 == 128) {
        batch.nprob = 1;
        batch.p[1] = batch.p[0];
        hipLaunchKernelGGL(sa_packed_mlp128_kernel<1>, dim3(grid), dim3(256), 0, st, batch, ticket, per_wg);
    } else
        hipLaunchKernelGGL(sa_packed_mlp256_kernel, dim3(grid), dim3(512), 0, st, n, m, hdr, (const float4 *)rowdxyz, (const float4 *)P,
                           (const float4 *)wxyz, rowinfo, tilecloud, w2t, b2, w3t, b3, out, out_stride, out_col, ticket, per_wg, batch.p[0].lds_pool);
    return check_launch("sa_packed_mlp");
}

// Up to two 128-wide problems (the scales of one MSG level) in ONE launch of sa_packed_mlp128_kernel: see the kernel.  Same arguments
// per problem as prcnn_sa_packed_mlp (c3 = 128), every output slice zero already or zeroed here.
extern "C" int prcnn_sa_packed_mlp_batch(int nprob, const prcnn_sa_problem *pr, void *stream)
{
    PRCNN_REQUIRE(nprob >= 1 && nprob <= 2 && pr, "sa_packed_mlp_batch: 1 or 2 problems");
    hipStream_t st = (hipStream_t)stream;
    SaPkBatch batch;
    batch.nprob = nprob;
    long most = 0;
    int narrow = 0;
    for (int i = 0; i < nprob; ++i) {
        const prcnn_sa_problem &q = pr[i];
        PRCNN_REQUIRE(q.b >= 0 && q.n >= 0 && q.m >= 0 && q.max_tiles >= 0 && q.c3 == 128, "sa_packed_mlp_batch: bad sizes (c3 = 128 only)");
        int live;
        const int rc = sa_pk_problem("sa_packed_mlp_batch", false, q, st, &batch.p[i], &live);
        if (rc != PRCNN_OK) return rc;
        // the real widths of a zero-padded problem (0 = 128): 64-64 and 64-96 have kernels of their own (round 5)
        PRCNN_REQUIRE((q.c1 == 0 || (q.c1 >= 1 && q.c1 <= 128)) && (q.c2 == 0 || (q.c2 >= 1 && q.c2 <= 128)), "sa_packed_mlp_batch: bad widths c1=%d c2=%d", q.c1, q.c2);
        if (nprob == 2 && q.c1 == 64 && (q.c2 == 64 || q.c2 == 96)) { batch.p[i].c1 = 64; batch.p[i].c2 = q.c2; ++narrow; }
        most = q.max_tiles > most ? q.max_tiles : most;
    }
    if (nprob == 1) batch.p[1] = batch.p[0];
    int per_wg;
    const long grid1 = sa_pk_grid(most, nprob, &per_wg);
    unsigned int *ticket = next_ticket(st);
    if (!ticket) { set_error("sa_packed_mlp_batch: cannot set up the tile ticket"); return PRCNN_ELAUNCH; }
    if (nprob == 1) hipLaunchKernelGGL(sa_packed_mlp128_kernel<1>, dim3((unsigned)grid1), dim3(256), 0, st, batch, ticket, per_wg);
    else if (narrow == 2) hipLaunchKernelGGL((sa_packed_mlp128_kernel<2, true>), dim3((unsigned)(grid1 * nprob)), dim3(256), 0, st, batch, ticket, per_wg);
    else hipLaunchKernelGGL(sa_packed_mlp128_kernel<2>, dim3((unsigned)(grid1 * nprob)), dim3(256), 0, st, batch, ticket, per_wg);
    return check_launch("sa_packed_mlp_batch");
}
