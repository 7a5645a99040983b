// sa_tile.hpp -- what the set-abstraction tile kernels share (csrc/sa_mlp_fused.hip: one centre per tile; csrc/sa_packed.hip: the
// distinct rows of csrc/ball_pack.hip's lists; csrc/rows_layer.hip and csrc/rcnn_entrance.hip: the per-point layers in front of them): the tile's shape, the 128-deep MFMA panels over a weight panel held in registers, the
// epilogues, the ticket draws and the row-descriptor codec of the packed lists.
//
// A tile is 64 rows x 128 channels in LDS, rows padded to 132 floats.  Lane (j, h) = (lane & 31, lane >> 5) of a wave supplies row j
// (and 32 + j) of the A operand and column j of the B operand; h picks the k half: at step s the instruction's two k values are s and
// s + 64.  A lane's four consecutive steps are 16 contiguous bytes of its row: one ds_read_b128 per four MFMAs and row half.
// C/D layout: column = j, row = (r & 3) + 8 (r >> 2) + 4 h for accumulator register r.
// The panels, the weight load and the epilogues are macros that expect j and h in scope, like PL_STAGE_SIDE (layer_tile.hpp) and
// RT_STAGE* (mfma_stream.hpp): sa_packed_mlp128_kernel sits at the register ceiling, and its register allocation moves with the form
// of these blocks (the epilogue as a function: 248 -> 256 VGPRs and 28 bytes of scratch; the weight load as a function: another
// schedule of the whole kernel).  Their COL argument is pasted unparenthesised on purpose: the address sums then associate as in the
// kernels' own text, (row * LD + 32 w) + j, and the compiled code is the hand-written one's.  The rest are functions.
#pragma once
#include "common.hpp"

namespace prcnn {

constexpr int PK_C = 128;            // C1 = C2 (narrower levels are zero-padded by the caller)
constexpr int PK_ROWS = 64;          // rows per tile (= nsample of the unpacked kernels)
constexpr int PK_LD = PK_C + 4;      // LDS row stride in floats

#define SA_MFMA(a, b, acc) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
// acc0 / acc1 (rows 0-31 / 32-63) += T[64][k] @ wf over the k of NG k-groups (16: all 128; 8: k = 0..31 and 64..95)
#define SA_PANEL2(T, wf, NG, acc0, acc1)                                                                  \
    {                                                                                                     \
        const float *a0p = (T) + j * PK_LD + 64 * h;                                                      \
        const float *a1p = (T) + (32 + j) * PK_LD + 64 * h;                                               \
        _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                \
            const float4 a0 = *reinterpret_cast<const float4 *>(a0p + 4 * g);                             \
            const float4 a1 = *reinterpret_cast<const float4 *>(a1p + 4 * g);                             \
            SA_MFMA(a0.x, wf[4 * g + 0], acc0) SA_MFMA(a1.x, wf[4 * g + 0], acc1)                         \
            SA_MFMA(a0.y, wf[4 * g + 1], acc0) SA_MFMA(a1.y, wf[4 * g + 1], acc1)                         \
            SA_MFMA(a0.z, wf[4 * g + 2], acc0) SA_MFMA(a1.z, wf[4 * g + 2], acc1)                         \
            SA_MFMA(a0.w, wf[4 * g + 3], acc0) SA_MFMA(a1.w, wf[4 * g + 3], acc1)                         \
        }                                                                                                 \
    }
// acc += T[32 RB .. 32 RB + 32)[128] @ wf: one row half
#define SA_PANEL1(T, RB, wf, acc)                                                                         \
    {                                                                                                     \
        const float *ap = (T) + (32 * (RB) + j) * PK_LD + 64 * h;                                         \
        _Pragma("unroll") for (int g = 0; g < 16; ++g) {                                                  \
            const float4 a = *reinterpret_cast<const float4 *>(ap + 4 * g);                               \
            SA_MFMA(a.x, wf[4 * g + 0], acc) SA_MFMA(a.y, wf[4 * g + 1], acc)                             \
            SA_MFMA(a.z, wf[4 * g + 2], acc) SA_MFMA(a.w, wf[4 * g + 3], acc)                             \
        }                                                                                                 \
    }
// The pair steps of the narrow kernel: step u takes k = K0 + 2u (h = 0) and K0 + 2u + 1 (h = 1), weights from wf[S0 + u], NG groups of
// two steps; one row half (RB) or both
#define SA_PAIRS1(T, RB, K0, wf, S0, NG, acc)                                                             \
    {                                                                                                     \
        const float *ap = (T) + (32 * (RB) + j) * PK_LD + (K0) + h;                                       \
        _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                \
            SA_MFMA(ap[4 * g], wf[(S0) + 2 * g], acc) SA_MFMA(ap[4 * g + 2], wf[(S0) + 2 * g + 1], acc)   \
        }                                                                                                 \
    }
#define SA_PAIRS2(T, K0, wf, S0, NG, acc0, acc1)                                                          \
    {                                                                                                     \
        const float *a0p = (T) + j * PK_LD + (K0) + h;                                                    \
        const float *a1p = (T) + (32 + j) * PK_LD + (K0) + h;                                             \
        _Pragma("unroll") for (int g = 0; g < (NG); ++g) {                                                \
            SA_MFMA(a0p[4 * g], wf[(S0) + 2 * g], acc0) SA_MFMA(a1p[4 * g], wf[(S0) + 2 * g], acc1)       \
            SA_MFMA(a0p[4 * g + 2], wf[(S0) + 2 * g + 1], acc0) SA_MFMA(a1p[4 * g + 2], wf[(S0) + 2 * g + 1], acc1) \
        }                                                                                                 \
    }

// a lane's 64 registers of a 128 x 32 weight panel: wf[s] = B[k][COL] of a k-major matrix with row stride LD, k = s + 64 h
#define SA_LOAD_PANEL(wf, w, LD, COL)                                                                     \
    _Pragma("unroll") for (int s = 0; s < 64; ++s) wf[s] = w[(long)(s + 64 * h) * LD + COL];

// relu(acc + bias) -> column COL of tile T (the next layer's A operand): the accumulator of row half RB, or both of a wave's 64 x 32
// block
#define SA_STORE_RELU(T, RB, COL, acc, bias)                                                              \
    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                        \
        (T)[(32 * (RB) + (r & 3) + 8 * (r >> 2) + 4 * h) * PK_LD + COL] = fmaxf(acc[r] + (bias), 0.f);
#define SA_STORE_RELU2(T, COL, acc0, acc1, bias)                                                          \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                      \
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;                                                   \
        (T)[row * PK_LD + COL] = fmaxf(acc0[r] + (bias), 0.f);                                            \
        (T)[(32 + row) * PK_LD + COL] = fmaxf(acc1[r] + (bias), 0.f);                                     \
    }

// max over the tile's 64 rows of one column (16 accumulator registers x 2 row halves per lane, then the other lane half)
__device__ __forceinline__ float sa_max64(const f32x16 &acc0, const f32x16 &acc1)
{
    float mx = fmaxf(acc0[0], acc1[0]);
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(acc0[r], acc1[r]));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
}

// ---- tile tickets (common.hpp ticket_release): thread 0 draws, the workgroup reads the draw after its next barrier.  The slots
// alternate: slot[(served + 1) & 1] is written before tile `served`'s first barrier, read after it and rewritten two tiles later.
__device__ __forceinline__ long sa_first_ticket(unsigned int *slot, unsigned int *ticket, int tid)
{
    if (tid == 0) slot[0] = atomicAdd(ticket, 1u);
    __syncthreads();
    return slot[0];
}
// Not on the last tile this workgroup serves: a ticket drawn and not served would be a tile nobody computes.
__device__ __forceinline__ void sa_next_ticket(unsigned int *slot, unsigned int *ticket, int tid, int served, int tiles_per_wg)
{
    const bool more = served + 1 < tiles_per_wg;
    if (tid == 0) slot[(served + 1) & 1] = more ? atomicAdd(ticket, 1u) : 0xffffffffu;
}

// ---- row descriptors of a packed list (csrc/ball_pack.hip; tests/row_lists.py)
//   with tilecloud:    (centre << 16) | point, the cloud of tile t in tilecloud[t], hdr[0] tiles
//   without (round 5): (cloud << 16) | (centre << 9) | point, written by prcnn_rcnn_roi_geometry_packs for the RoI clouds (512 points,
//     128 centres at most); the list's hdr[1] rows are cut into tiles wherever they fall: a tile holds the rows of several clouds, only
//     the list's last tile is partly filled (its missing rows read as copies of the list's last row: copies do not change a max).
//     With a tile per cloud the 1600 RoI clouds of a launch padded 39 rows to 64 on the second level of the uniform scene, 102 to 128
//     on LiDAR-shaped ones.
struct SaRowCodec {
    bool rowcloud;
    unsigned int kmask, cmask;
    int cshift;
    long last_row, tiles;
    __device__ __forceinline__ SaRowCodec(const unsigned int *__restrict__ hdr, bool rows_carry_cloud) : rowcloud(rows_carry_cloud)
    {
        const long nrows = hdr[1];
        tiles = rowcloud ? (nrows + PK_ROWS - 1) / PK_ROWS : (long)hdr[0];
        last_row = rowcloud ? nrows - 1 : 0x7fffffffffffL;
        kmask = rowcloud ? 0x1ffu : 0xffffu; cmask = rowcloud ? 0x7fu : 0xffffu;
        cshift = rowcloud ? 9 : 16;
    }
    __device__ __forceinline__ long row(long r) const { return min(r, last_row); }           // the list entry that tile row r reads
    __device__ __forceinline__ int point(unsigned int info) const { return (int)(info & kmask); }
    __device__ __forceinline__ int centre(unsigned int info) const { return (int)((info >> cshift) & cmask); }
    __device__ __forceinline__ long cloud(unsigned int info, int tile_cloud) const { return rowcloud ? (long)(int)(info >> 16) : (long)tile_cloud; }
};

// ---- a tile's list entries, fetched one tile ahead: R descriptors per thread (rows r0 + (64 / R) i), the tile's cloud, and by the
// first 64 threads the centre-relative coordinates of row tid
template <int R>
__device__ __forceinline__ void sa_fetch_rows(const SaRowCodec &cd, const unsigned int *__restrict__ rowinfo, const int *__restrict__ tilecloud,
                                              const float4 *__restrict__ rowdxyz, long t, int r0, int tid, unsigned int (&info)[R], int &cloud,
                                              float4 &d)
{
#pragma unroll
    for (int i = 0; i < R; ++i) info[i] = rowinfo[cd.row(t * PK_ROWS + r0 + (PK_ROWS / R) * i)];
    if (!cd.rowcloud) cloud = tilecloud[t];
    if (tid < PK_ROWS) d = rowdxyz[cd.row(t * PK_ROWS + tid)];
}
// float4 `chunk` of the row of P (b, n, 128) that descriptor `info` names
__device__ __forceinline__ float4 sa_gather_p(const SaRowCodec &cd, const float4 *__restrict__ P, unsigned int info, int cloud, int n, int chunk)
{
    return P[(cd.cloud(info, cloud) * n + (long)cd.point(info)) * (PK_C / 4) + chunk];
}
// bit i set when tile row i begins a new centre (cc[64]: output row of every tile row, LDS): the same word in every wave
__device__ __forceinline__ unsigned long long sa_segment_starts(const int *cc, int lane)
{
    const int myc = cc[lane], prevc = cc[lane ? lane - 1 : 0];
    return __ballot(lane == 0 || myc != prevc);
}

}  // namespace prcnn
