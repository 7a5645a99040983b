// rows_layer.hip -- one 128-wide f32 MFMA layer over 64-row tiles, as a general entry for the 128-wide shared-MLP / Conv1d layers of the
// network (FP level 0, the first layers of the RPN heads, the per-point parts of SA levels) and as the three-launch form of the RCNN
// entrance chain (csrc/rcnn_entrance.hip):
//
//   rows_layer_kernel       out = act(A0 @ W0 [+ A1 @ W1] + bias) over whole tiles, or over the tiles a tile map names
//   rows_layer_list_kernel  the same layer (one panel) over a LIST of rows
//
// The tile, the MFMA mapping, the panel, the weight load and the ticket draws are sa_tile.hpp's: tile = 64 rows, 4 waves, wave w owns
// output columns [32w, 32w+32), its 128 x 32 weight panels live in VGPRs (64 per panel), activations in LDS rows of 132 floats, K split
// across the two lane halves so one ds_read_b128 feeds four v_mfma_f32_32x32x2_f32.  The staged epilogue and the row store are
// mfma_stream.hpp's.
#include "sa_tile.hpp"
#include "mfma_stream.hpp"

namespace prcnn {

constexpr int ROWS_TILES_PER_WG = 8;

// rows row[i] (i < 8) of src (row stride ld) -> p[i]: this thread's 16 bytes at float column `off` of each
template <typename V, typename I>
__device__ __forceinline__ void rows_fetch8(V (&p)[8], const float *__restrict__ src, const I (&row)[8], int ld, int off)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = *reinterpret_cast<const V *>(src + (long)row[i] * ld + off);
}

// ---- one 128-wide layer over 64-row tiles:  out = act(A0 @ W0 [+ A1 @ W1] + bias)
//   PRO = 0: A0 = src0 rows (128 floats at column col0, row stride ld0);   PRO = 1: A0 = relu(in5 @ Wu1 + bu1) computed by
//   the builder from columns 0..4 of src0 (the first xyz_up layer: K = 5 is VALU work);  NPANEL = 2 adds A1 = src1 rows.
// The inputs of the NEXT tile are fetched into registers right after this tile's builder, so the HBM latency runs
// behind the MFMAs; barriers order LDS only (lds_barrier), they do not drain those loads.  The accumulators are staged
// through LDS (tile 0 is dead by then) so that every output row leaves as 32 x 16-byte lanes.
template <int NPANEL, int PRO, bool RELU>
__global__ __launch_bounds__(256, 2) void rows_layer_kernel(
    long tiles, int per_wg, const float *__restrict__ src0, int ld0, int col0, const float *__restrict__ src1, int ld1, int col1,
    const float4 *__restrict__ wu1, const float4 *__restrict__ bu1, const float *__restrict__ w0, const float *__restrict__ w1,
    const float *__restrict__ bias, float *__restrict__ out, unsigned int *__restrict__ ticket,
    const int *__restrict__ tilemap, const unsigned int *__restrict__ ntiles_dev)
{
    // tilemap (optional): ticket j serves tile tilemap[j], j < *ntiles_dev -- only the tiles that hold DISTINCT pooled rows
    // (prcnn_pooled_tiles); the grid is still sized for all tiles and surplus workgroups draw a ticket and leave.
    if (ntiles_dev) tiles = (long)*ntiles_dev;
#define TILE_OF(tk) (tilemap ? (long)tilemap[tk] : (long)(tk))
    __shared__ float lds[NPANEL * PK_ROWS * PK_LD + 4];
    float *T0 = lds, *T1 = lds + (NPANEL - 1) * PK_ROWS * PK_LD;
    unsigned int *slot = reinterpret_cast<unsigned int *>(lds + NPANEL * PK_ROWS * PK_LD);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, h = lane >> 5;
    const int chunk = tid & 31, r0 = tid >> 5;
    float wa[64], wb[NPANEL == 2 ? 64 : 1];
    SA_LOAD_PANEL(wa, w0, PK_C, 32 * w + j)
    if constexpr (NPANEL == 2) SA_LOAD_PANEL(wb, w1, PK_C, 32 * w + j)
    const float bias_w = bias[32 * w + j];
    float4 k1[PRO ? 5 : 1], b1 = {0, 0, 0, 0};
    if constexpr (PRO == 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) k1[k] = wu1[k * 32 + chunk];
        b1 = bu1[chunk];
    }

    constexpr bool PF = (NPANEL == 1);   // two panels: 128 weight registers leave no room for a 64-register prefetch
    float4 p0[8], p1[NPANEL == 2 ? 8 : 1];
    float pd[PRO ? 8 : 1];
    long rn[8];                          // the rows a fetch is for
#define ROWS_FETCH(tile)                                                                                              \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) rn[i] = (tile) * PK_ROWS + r0 + 8 * i;                              \
    rows_fetch8(p0, src0, rn, ld0, PRO == 1 ? 0 : col0 + 4 * chunk);                                                  \
    if constexpr (PRO == 1) { _Pragma("unroll") for (int i = 0; i < 8; ++i) pd[i] = src0[rn[i] * ld0 + 4]; }          \
    if constexpr (NPANEL == 2) rows_fetch8(p1, src1, rn, ld1, col1 + 4 * chunk);

    long t = sa_first_ticket(slot, ticket, tid);
    if (t >= tiles) { if (tid == 0) ticket_release(ticket); return; }
    long tt = TILE_OF(t);
    if (PF) { ROWS_FETCH(tt) }
    for (int served = 0; served < per_wg && t < tiles; ++served) {
        sa_next_ticket(slot, ticket, tid, served, per_wg);
        if (!PF) { ROWS_FETCH(tt) }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = r0 + 8 * i;
            float4 v = p0[i];
            if constexpr (PRO == 1) {
                const float4 q = p0[i];
                const float d = pd[i];
                v = relu4(pk_fma4(k1[4], d, pk_fma4(k1[3], q.w, pk_fma4(k1[2], q.z, pk_fma4(k1[1], q.y, pk_fma4(k1[0], q.x, b1))))));
            }
            *reinterpret_cast<float4 *>(T0 + row * PK_LD + 4 * chunk) = v;
            if constexpr (NPANEL == 2) *reinterpret_cast<float4 *>(T1 + row * PK_LD + 4 * chunk) = p1[i];
        }
        lds_barrier();
        const long t_next = slot[(served + 1) & 1];
        const long tt_next = t_next < tiles ? TILE_OF(t_next) : 0;
        if (PF && t_next < tiles) { ROWS_FETCH(tt_next) }           // in flight during the MFMAs below
        f32x16 acc0 = {0}, acc1 = {0};
        SA_PANEL2(T0, wa, 16, acc0, acc1)
        if constexpr (NPANEL == 2) SA_PANEL2(T1, wb, 16, acc0, acc1)
        lds_barrier();                                              // every wave has finished reading the tiles
        RT_EPILOGUE(T0, bias_w, RELU)
        lds_barrier();
        RT_STORE_ROWS8(float4, T0, out, (tt * PK_ROWS + row))
        lds_barrier();                                              // the next builder overwrites T0
        t = t_next;
        tt = tt_next;
    }
#undef ROWS_FETCH
#undef TILE_OF
    if (tid == 0) ticket_release(ticket);          // the launch's last workgroup zeroes the counter for the word's next user
}

// ---- one 128 -> 128 layer over a LIST of rows (round 5): out[r] = act(src[r] @ W + bias) for r = rowmap[0 .. hdr[1]), 64 list entries
// per tile whichever rows they are; rows that are not listed are neither read nor written.  The per-point part of the RCNN's second SA
// level runs over the level-1 centres that are their own representatives only (47 of 128 per RoI on the uniform scene: the others
// copy an earlier centre and no row list names them).  Tiles strided over the workgroups; the NEXT tile's rows (their numbers were
// fetched one tile earlier still) arrive behind the MFMAs.  Per row the arithmetic of rows_layer_kernel / packed_layer_stream_kernel.
template <bool RELU>
__global__ __launch_bounds__(256, 2) void rows_layer_list_kernel(const float *__restrict__ src, int ld, int col, const float *__restrict__ w0,
                                                                 const float *__restrict__ bias, float *__restrict__ out,
                                                                 const int *__restrict__ rowmap, const unsigned int *__restrict__ hdr)
{
    __shared__ float T0[PK_ROWS * PK_LD];
    const long nrows = (long)hdr[1];
    const long tiles = (nrows + PK_ROWS - 1) / PK_ROWS;
    long t = blockIdx.x;
    if (t >= tiles) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, h = lane >> 5;
    const int chunk = tid & 31, r0 = tid >> 5;
    float wa[64];
    SA_LOAD_PANEL(wa, w0, PK_C, 32 * w + j)
    const float bias_w = bias[32 * w + j];
    const long step = gridDim.x;
    int cur[8], nxt[8];
    f32x4 p0[8];
    // the list entries of this thread's 8 rows of tile `tile` (the last tile's missing entries repeat the list's last row); none: 0
#define LIST_ROWS(dst, tile)                                                                                          \
    if ((tile) < tiles) { _Pragma("unroll") for (int i = 0; i < 8; ++i) dst[i] = rowmap[min((tile) * PK_ROWS + r0 + 8 * i, nrows - 1)]; } \
    else { _Pragma("unroll") for (int i = 0; i < 8; ++i) dst[i] = 0; }
    LIST_ROWS(cur, t)
    LIST_ROWS(nxt, t + step)
    rows_fetch8(p0, src, cur, ld, col + 4 * chunk);
    for (; t < tiles; t += step) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4 *>(T0 + (r0 + 8 * i) * PK_LD + 4 * chunk) = p0[i];
        lds_barrier();
        int nn[8];
        if (t + step < tiles) {                                     // the next tile's rows, the numbers of the one after it: behind the MFMAs
            rows_fetch8(p0, src, nxt, ld, col + 4 * chunk);
            LIST_ROWS(nn, t + 2 * step)
        }
        f32x16 acc0 = {0}, acc1 = {0};
        SA_PANEL2(T0, wa, 16, acc0, acc1)
        lds_barrier();                                              // every wave has finished reading the tile
        RT_EPILOGUE(T0, bias_w, RELU)
        lds_barrier();
        RT_STORE_ROWS8(float4, T0, out, (long)cur[i])
        lds_barrier();                                              // the next builder overwrites T0
        if (t + step < tiles) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { cur[i] = nxt[i]; nxt[i] = nn[i]; }
        }
    }
#undef LIST_ROWS
}

// One generation of workgroups when the launch is short (tiles / 512 slots per workgroup, tickets balance the rest); at least
// ROWS_TILES_PER_WG so that long launches still turn workgroups over.
int rows_layer_launch(int npanel, int pro, bool relu, long tiles, const float *src0, int ld0, int col0, const float *src1, int ld1, int col1,
                      const float *wu1, const float *bu1, const float *w0, const float *w1, const float *bias, float *out, const int *tilemap,
                      const unsigned int *ntiles, hipStream_t st, const char *what)
{
    PRCNN_REQUIRE((npanel == 1 || npanel == 2) && (!pro || (npanel == 1 && relu)), "%s: no such form of the layer kernel", what);
    int per_wg = (int)((tiles + 511) / 512);
    if (per_wg < ROWS_TILES_PER_WG) per_wg = ROWS_TILES_PER_WG;
    const int grid = (int)((tiles + per_wg - 1) / per_wg);
    unsigned int *tk = next_ticket(st);
    if (!tk) { set_error("%s: cannot set up the tile ticket", what); return PRCNN_ELAUNCH; }
#define LAUNCH(NP, PRO, RL) hipLaunchKernelGGL((rows_layer_kernel<NP, PRO, RL>), dim3(grid), dim3(256), 0, st, tiles, per_wg, src0, ld0, col0, \
                                               src1, ld1, col1, (const float4 *)wu1, (const float4 *)bu1, w0, w1, bias, out, tk, tilemap, ntiles)
    if (pro) LAUNCH(1, 1, true);
    else if (npanel == 1) { if (relu) LAUNCH(1, 0, true); else LAUNCH(1, 0, false); }
    else                  { if (relu) LAUNCH(2, 0, true); else LAUNCH(2, 0, false); }
#undef LAUNCH
    return check_launch(what);
}

}  // namespace prcnn

using namespace prcnn;

// out (r,128) = act(A0 @ w[0:128] [+ A1 @ w[128:256]] + bias) for r % 64 == 0 rows.  A0 = src0 rows (128 floats at column col0, row
// stride ld0); npanel = 2 adds A1 = src1 rows (col1, ld1), i.e. a K = 256 layer whose input is two 128-wide halves (of one tensor or
// of two).
extern "C" int prcnn_rows_gemm128(long r, int npanel, const float *src0, int ld0, int col0, const float *src1, int ld1,
                                  int col1, const float *w, const float *bias, int relu, float *out, void *stream)
{
    PRCNN_REQUIRE(r >= 0 && r % PK_ROWS == 0, "rows_gemm128: %ld rows is not a multiple of %d", r, PK_ROWS);
    PRCNN_REQUIRE(npanel == 1 || npanel == 2, "rows_gemm128: npanel must be 1 or 2");
    PRCNN_REQUIRE(ld0 % 4 == 0 && col0 % 4 == 0 && col0 >= 0 && col0 + PK_C <= ld0, "rows_gemm128: bad layout of source 0");
    PRCNN_REQUIRE(npanel == 1 || (ld1 % 4 == 0 && col1 % 4 == 0 && col1 >= 0 && col1 + PK_C <= ld1), "rows_gemm128: bad layout of source 1");
    if (r == 0) return PRCNN_OK;
    PRCNN_REQUIRE(src0 && w && bias && out && (npanel == 1 || src1), "rows_gemm128: null pointer");
    PRCNN_REQUIRE((((uintptr_t)src0 | (uintptr_t)out | (npanel == 2 ? (uintptr_t)src1 : 0)) & 15) == 0, "rows_gemm128: 16-byte alignment required");
    return rows_layer_launch(npanel, 0, relu != 0, r / PK_ROWS, src0, ld0, col0, src1, ld1, col1, nullptr, nullptr, w, w + (size_t)PK_C * PK_C,
                             bias, out, nullptr, nullptr, (hipStream_t)stream, "rows_gemm128");
}

// out (r, 128) rows rowmap[0 .. hdr[1]) = act(src rows (128 floats at column col, row stride ld) @ w (128, 128) k-major + bias): the
// 128-wide layer of prcnn_rows_gemm128 (npanel = 1) over a LIST of rows; rows that are not listed are left as they are.
extern "C" int prcnn_rows_gemm128_rows(long r, const float *src, int ld, int col, const float *w, const float *bias, int relu, float *out,
                                       const int *rowmap, const unsigned int *hdr, void *stream)
{
    PRCNN_REQUIRE(r >= 0 && r <= 0x7fffffffL && ld % 4 == 0 && col % 4 == 0 && col >= 0 && col + PK_C <= ld, "rows_gemm128_rows: bad layout");
    if (r == 0) return PRCNN_OK;
    PRCNN_REQUIRE(src && w && bias && out && rowmap && hdr, "rows_gemm128_rows: null pointer");
    PRCNN_REQUIRE((((uintptr_t)src | (uintptr_t)out) & 15) == 0, "rows_gemm128_rows: 16-byte alignment required");
    const long tiles = (r + PK_ROWS - 1) / PK_ROWS;              // at most: the list is on the device
    const long grid = tiles < mfma_grid_cap() ? tiles : mfma_grid_cap();
    if (relu) hipLaunchKernelGGL(rows_layer_list_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, ld, col, w, bias, out, rowmap, hdr);
    else hipLaunchKernelGGL(rows_layer_list_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, src, ld, col, w, bias, out, rowmap, hdr);
    return check_launch("rows_gemm128_rows");
}
