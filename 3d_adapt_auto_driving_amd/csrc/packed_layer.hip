// packed_layer.hip -- one shared-MLP layer of ANY width, out = act(A @ W + bias), on the f32 matrix cores: every per-point product,
// RPN SA3 / SA4 and the RCNN GroupAll level layer by layer (the fused kernels of sa_mlp_fused.hip / sa_packed.hip keep a level's
// weights in registers, which caps the widths at 128-128-256), FP layer 1 with its interpolated addend, the heads.
//
// Rows: a packed list whose tile count lives on the device (hdr[0], csrc/ball_pack.hip; the grid is sized for the worst case and the
// surplus workgroups exit at once) or a row count from the host.  K and N are multiples of 128 (the caller zero-pads: exact, relu(0) = 0
// meets zero weight rows).  The unit of work is a 64-row tile x a 128-column block; K runs in 128-deep panels: the panel of W in
// registers, the panel of A in LDS, 128 v_mfma_f32_32x32x2_f32 per panel (csrc/layer_tile.hpp: lane roles, stages, epilogues).  Every
// form sums in the same order and gives the same bits -- oracle/mlp_oracle.c orc_rows_layer_mfma restates it.
//
// Five forms; pl_plan() below is the one place that picks (items = row tiles x column blocks with something to store):
//   packed_layer_kernel<SEGMAX>          K = 128: one panel, nothing to prefetch; three workgroups per CU cover each other's loads
//   packed_layer_stream_kernel           K = 128, host count, >= PRCNN_PL_STREAM_MIN items: resident weights, the row tiles streamed
//   packed_layer_pipe_kernel<SEGMAX>     K >= 256: every panel fetched behind the MFMAs of the one before it
//   packed_layer_pipe32_kernel           K >= 256, host count, < 256 items: 32-row tiles, twice the workgroups (no addend)
//   packed_layer_persist_kernel<ADD>     K >= 256, host count, one problem, whole blocks, > PRCNN_PL_STREAM_CAP items: ticketed items,
//                                        the panel pipeline runs on from one item into the next
// SEGMAX (the last layer of a level + max pool): out[centre] = max over the centre's rows, atomicMax into a zeroed slice; lists only.
// The one-panel, pipe and pipe32 kernels take up to PL_MAX_BATCH problems per launch (blockIdx.z).
#include "layer_tile.hpp"
#include <cstdlib>

namespace prcnn {

#define PL_LOAD_A(dst, kk)                                                                              \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                     \
        long g = t * PL_ROWS + r0 + 8 * i;                                                              \
        if (g >= rows) g = rows - 1; /* ragged last tile (host-count mode): recompute the last row */   \
        dst[i] = *reinterpret_cast<const f32x4 *>(pb.A + g * pb.lda + (kk) + 4 * chunk);               \
    }
#define PL_STORE_A(src)                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 8; ++i)                                                       \
        *reinterpret_cast<f32x4 *>(tile + (r0 + 8 * i) * PL_LD + 4 * chunk) = src[i];

// K = 128: one panel, nothing to prefetch
template <bool SEGMAX>
__global__ __launch_bounds__(256, 2) void packed_layer_kernel(const PLBatch bt)
{
    const PLProblem pb = bt.p[blockIdx.z];                     // a copy: every field is read here, in one run of scalar loads
    __shared__ float tile[PL_ROWS * PL_LD];
    __shared__ int ctr[PL_ROWS];
    const long t = blockIdx.x;
    const long rows = pb.hdr ? (long)pb.hdr[0] * PL_ROWS : pb.rows_host;
    const int n0 = blockIdx.y * 128;
    if (t * PL_ROWS >= rows || n0 >= pb.n_store) return;       // (a batched launch is sized for its largest problem)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, h = lane >> 5;
    const int chunk = tid & 31, r0 = tid >> 5;
    const int K = pb.K, N = pb.N;
    f32x16 acc0 = {0}, acc1 = {0};
    // weights through a buffer resource: one 32-bit lane offset in a VGPR, the row offset of each load in a scalar register
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)pb.W, 0, K * N * 4, 0x00020000);
    const unsigned int row_bytes = (unsigned int)N * 4u;
    const unsigned int lane_off = ((unsigned int)(64 * h) * (unsigned int)N + (unsigned int)(n0 + 32 * w + j)) * 4u;
    for (int k0 = 0; k0 < K; k0 += 128) {
        float wf[64];
        f32x4 ar[8];
        PL_LOAD_W(wf, k0)
        PL_LOAD_A(ar, k0)
        if (k0) __syncthreads();                           // every wave has finished reading the previous panel
        PL_STORE_A(ar)
        __syncthreads();
        PL_STAGE(tile, wf)
    }
    pl_epilogue<SEGMAX>(acc0, acc1, tile, ctr, t, rows, n0, pb);
}

// K >= 256: two LDS tiles, two weight register sets, every panel fetched behind the MFMAs of the one before it
// (PL_STAGE_PREFETCH); the k order of every dot product is the same as in the one-panel kernel (panels in sequence).
template <bool SEGMAX>
__global__ __launch_bounds__(256, 2) void packed_layer_pipe_kernel(const PLBatch bt)
{
    const PLProblem pb = bt.p[blockIdx.z];
    __shared__ float tiles[2 * PL_ROWS * PL_LD];
    __shared__ int ctr[PL_ROWS];
    const long t = blockIdx.x;
    const long rows = pb.hdr ? (long)pb.hdr[0] * PL_ROWS : pb.rows_host;
    const int n0 = blockIdx.y * 128;
    if (t * PL_ROWS >= rows || n0 >= pb.n_store) return;       // (a batched launch is sized for its largest problem)
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = tid & 31, r0 = tid >> 5;
    const int K = pb.K, N = pb.N;
    f32x16 acc0 = {0}, acc1 = {0};
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)pb.W, 0, K * N * 4, 0x00020000);
    const unsigned int row_bytes = (unsigned int)N * 4u;
    const unsigned int lane_off = ((unsigned int)(64 * h) * (unsigned int)N + (unsigned int)(n0 + 32 * w + j)) * 4u;
    // this tile's rows of A as their own buffer: rows past the end (a ragged last tile) are out of its range and read as 0
    const long left = rows - t * PL_ROWS;
    const unsigned int a_row_bytes = (unsigned int)pb.lda * 4u;
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(pb.A + t * PL_ROWS * pb.lda), 0, (int)((left < PL_ROWS ? left : PL_ROWS) * (long)a_row_bytes), 0x00020000);
    const unsigned int a_lane = (unsigned int)r0 * a_row_bytes + 16u * chunk;
    float wa[64], wb[64];
    PL_LOAD_W(wa, 0)
    PL_FETCH_TILE(tiles, 8, 0)
    const int np = K >> 7;
    for (int p = 0; p < np; ++p) {
        PL_VM_DRAIN                                        // the panel about to be used is complete (weights; rows are in LDS)
        lds_barrier();                                     // ... and published; the other tile is free
        const float *T = tiles + (p & 1) * (PL_ROWS * PL_LD);
        float *TN = tiles + ((p + 1) & 1) * (PL_ROWS * PL_LD);
        if (p + 1 < np) {
            PL_STAGE_PREFETCH(T, TN, wa, wb, (p + 1) * 128)
#pragma unroll
            for (int s = 0; s < 64; ++s) wa[s] = wb[s];
        } else {
            PL_STAGE(T, wa)
        }
    }
    if constexpr (!SEGMAX) {
        if (n0 + 128 <= pb.n_store && !pb.addG) {
            // whole 128-column blocks, no addend: the direct epilogue (the staged one was 4.5-14 k of a workgroup's 95-120 k cycles in the
            // launches of at most 512 items this kernel keeps)
            pl_store_direct(acc0, acc1, pb.bias[n0 + 32 * w + j], pb.do_relu, pb.out, pb.ldo, t, rows, (unsigned int)(n0 + 32 * w + j));
            return;
        }
    }
    pl_epilogue<SEGMAX>(acc0, acc1, tiles, ctr, t, rows, n0, pb);
}

// ---- K >= 256 layers, PERSISTENT.  packed_layer_pipe_kernel pays per 64 x 128 tile what profiles/layer_k_sweep.py measures as
// the intercept of time over K: 9.4 us per round of workgroups -- dispatch, an exposed round trip for the first panel (64 weights per
// lane + 8 rows), the LDS-staged epilogue with two barriers, the drain of its stores -- against 7.8 us of MFMAs per panel: 0.55 of
// the MFMA peak at K = 256, 0.67 at K = 512 (0.88 is the slope).  Here a workgroup draws (row tile, column block) items from a ticket
// and never leaves the panel pipeline: the FIRST panel of the next item is fetched behind the MFMAs of the last panel of the running
// one (same PL_STAGE_PREFETCH, other buffer resources), and the epilogue is the direct one.  Per output element the MFMA sequence, the
// bias add and the ReLU are those of the one-tile kernels: same bits.  Host-count mode, N == n_store, no pooling; ADD: the
// interpolation addend (prcnn_packed_layer_interp).
template <bool ADD>
__global__ __launch_bounds__(256, 2) void packed_layer_persist_kernel(const PLProblem pb, unsigned int *__restrict__ ticket)
{
    __shared__ float tiles[2 * PL_ROWS * PL_LD];
    __shared__ unsigned int s_item[2];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = tid & 31, r0 = tid >> 5;
    const long rows = pb.rows_host;
    const int K = pb.K, N = pb.N;
    const unsigned int col_blocks = (unsigned int)(N >> 7);
    const unsigned int n_tiles = (unsigned int)((rows + PL_ROWS - 1) / PL_ROWS);
    const unsigned int n_items = n_tiles * col_blocks;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)pb.W, 0, K * N * 4, 0x00020000);
    const unsigned int row_bytes = (unsigned int)N * 4u;
    const unsigned int a_row_bytes = (unsigned int)pb.lda * 4u;
    const unsigned int a_lane = (unsigned int)r0 * a_row_bytes + 16u * chunk;
    const int np = K >> 7;
    // the rows of a tile as their own buffer: rows past the end (a ragged last tile) read as 0
    auto tile_rsrc = [&](unsigned int t) __attribute__((always_inline)) {
        const long left = rows - (long)t * PL_ROWS;
        return __builtin_amdgcn_make_buffer_rsrc((void *)(pb.A + (long)t * PL_ROWS * pb.lda), 0,
                                                 (int)((left < PL_ROWS ? left : PL_ROWS) * (long)a_row_bytes), 0x00020000);
    };
    auto loff = [&](unsigned int cb) __attribute__((always_inline)) {
        return ((unsigned int)(64 * h) * (unsigned int)N + (cb * 128u + (unsigned int)(32 * w + j))) * 4u;
    };
    // the first item is the workgroup's index (no round trip in front of the first loads; the host launches no more workgroups than
    // items), the later ones are drawn: gridDim.x + ticket
    unsigned int item = blockIdx.x;
    // items in column-block-minor order: neighbours in the draw order share their rows of A
    unsigned int t = item / col_blocks, cb = item - t * col_blocks;
    __amdgpu_buffer_rsrc_t ars = tile_rsrc(t);
    unsigned int lane_off = loff(cb);
    float wa[64], wb[64];
    PL_LOAD_W(wa, 0)
    PL_FETCH_TILE(tiles, 8, 0)
    int pp = 0;                                              // panels staged so far: the LDS tile alternates across items too
    int slot = 1;
    PL_VM_DRAIN                                              // the first item's first panel has arrived
    while (true) {
        f32x16 acc0 = {0}, acc1 = {0};
        unsigned int next = 0xffffffffu, tn = 0, cbn = 0, drawn = 0;
        const float bcol = pb.bias[(int)cb * 128 + 32 * w + j];    // (arrives behind the first panel: waited for by the drain of the second)
        for (int p = 0; p < np; ++p, ++pp) {
            // the panel about to be used is complete (weights in registers, rows in LDS): panel 0 of an item was waited for at the end
            // of the item before it (or above) -- no wait here, so that the stores of that item's results stay in flight behind this
            // panel's MFMAs (vmcnt counts loads and stores alike)
            if (p > 0) {
                PL_VM_DRAIN
                if (p == 1 && tid == 0) s_item[slot] = drawn;
            }
            lds_barrier();                                   // ... and published; the other tile is free
            // the NEXT item is drawn here: the atomic's round trip hides behind this panel's MFMAs, its value is read at the last panel
            if (p == 0 && tid == 0) drawn = gridDim.x + atomicAdd(ticket, 1u);
            const float *T = tiles + (pp & 1) * (PL_ROWS * PL_LD);
            float *TN = tiles + ((pp + 1) & 1) * (PL_ROWS * PL_LD);
            if (p + 1 < np) {
                PL_STAGE_PREFETCH(T, TN, wa, wb, (p + 1) * 128)
#pragma unroll
                for (int s2 = 0; s2 < 64; ++s2) wa[s2] = wb[s2];
            } else {
                next = s_item[slot];                         // (np >= 2: published before this panel's barrier)
                if (next < n_items) {
                    tn = next / col_blocks; cbn = next - tn * col_blocks;
                    const __amdgpu_buffer_rsrc_t ars_n = tile_rsrc(tn);
                    const unsigned int loff_n = loff(cbn);
                    PL_STAGE_PREFETCH_X(T, TN, wa, wb, 0, ars_n, loff_n)
#pragma unroll
                    for (int s2 = 0; s2 < 64; ++s2) wa[s2] = wb[s2];
                    PL_VM_DRAIN                              // (fetched behind 128 MFMAs: normally there already)
                } else {
                    PL_STAGE(T, wa)
                }
            }
        }
        if constexpr (ADD) {
            // the staged epilogue of the one-tile kernels, through the LDS tile of the panel just consumed (the next item's first panel
            // sits in the OTHER tile)
            float *Tlast = tiles + ((pp - 1) & 1) * (PL_ROWS * PL_LD);
            pl_epilogue<false>(acc0, acc1, Tlast, nullptr, (long)t, rows, (int)cb * 128, pb);
            __syncthreads();
        } else {
            pl_store_direct(acc0, acc1, bcol, pb.do_relu, pb.out, pb.ldo, (long)t, rows, cb * 128u + (unsigned int)(32 * w + j));
        }
        if (next >= n_items) break;
        t = tn; cb = cbn;
        ars = tile_rsrc(t);
        lane_off = loff(cb);
        slot ^= 1;
    }
    if (tid == 0) ticket_release(ticket);
}

// ---- K = 128 layers over many row tiles (the per-point parts of the SA levels: 10^5 rows, one panel): PERSISTENT workgroups.
// With one tile per workgroup every tile paid its own 64 weight loads (64 KB per workgroup from L2), an exposed round trip for
// its rows and an epilogue nobody overlapped: 55-59 TFLOP/s (profiles/r02_microbench.md).  Here a workgroup keeps its 128 x 32
// weight slices in registers and strides over the row tiles; the next tile's rows arrive behind the MFMAs of the running one
// (PL_STAGE_ROWS, two LDS tiles).  Per row the arithmetic is that of packed_layer_kernel: same bits.  Host-count mode, no pooling;
// pb.addG != NULL: the interpolation addend.
__global__ __launch_bounds__(256, 2) void packed_layer_stream_kernel(const PLProblem pb)
{
    __shared__ float tiles[2 * PL_ROWS * PL_LD];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = tid & 31, r0 = tid >> 5;
    const int n0 = blockIdx.y * 128;
    const long rows = pb.rows_host;
    const int N = pb.N;
    const long ntiles = (rows + PL_ROWS - 1) / PL_ROWS;
    long t = blockIdx.x;
    if (t >= ntiles || n0 >= pb.n_store) return;
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)pb.W, 0, 128 * N * 4, 0x00020000);
    const unsigned int row_bytes = (unsigned int)N * 4u;
    const unsigned int lane_off = ((unsigned int)(64 * h) * (unsigned int)N + (unsigned int)(n0 + 32 * w + j)) * 4u;
    float wf[64];
    PL_LOAD_W(wf, 0)
    // the whole matrix as one buffer: rows past the end (the ragged last tile) are out of its range and read as zero
    const unsigned int a_row_bytes = (unsigned int)pb.lda * 4u;
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc((void *)pb.A, 0, (int)(rows * (long)a_row_bytes), 0x00020000);
    const unsigned int a_lane = (unsigned int)r0 * a_row_bytes + 16u * chunk;
    PL_FETCH_TILE(tiles, 8, (unsigned int)(t * PL_ROWS) * a_row_bytes)
    // the bias column of this workgroup is loaded once; no wait at the top of an iteration (the rows of the tile were waited for when
    // they went to LDS) -- so the results of the tile before stay in flight behind this tile's MFMAs -- and whole 128-column blocks
    // without an addend leave by the direct epilogue
    const float bcol = pb.bias[n0 + 32 * w + j];
    const bool direct = n0 + 128 <= pb.n_store && !pb.addG;
    PL_VM_DRAIN
    for (int it = 0;; ++it) {
        lds_barrier();                                     // this tile's rows are published; the other tile is free
        float *T = tiles + (it & 1) * (PL_ROWS * PL_LD);
        float *TN = tiles + ((it + 1) & 1) * (PL_ROWS * PL_LD);
        const long tn = t + gridDim.x;
        f32x16 acc0 = {0}, acc1 = {0};
        if (tn < ntiles) {
            const unsigned int soff = (unsigned int)(tn * PL_ROWS) * a_row_bytes;
            PL_STAGE_ROWS(T, TN, wf, soff)
        } else {
            PL_STAGE(T, wf)
        }
        if (direct) {
            pl_store_direct(acc0, acc1, bcol, pb.do_relu, pb.out, pb.ldo, t, rows, (unsigned int)(n0 + 32 * w + j));
        } else {
            pl_epilogue<false>(acc0, acc1, T, nullptr, t, rows, n0, pb);
            __syncthreads();                               // (its staging through T is over before the next stage prefetches into it)
        }
        if (tn >= ntiles) break;
        t = tn;
    }
}

// ---- 32-row tiles: the layers that would give fewer than 256 workgroups of 64 rows (FP3, SA4's per-point parts, the RCNN
// heads: a few thousand rows, many panels).  Their launch time is one workgroup's serial panel chain; halving the rows of a
// tile halves the MFMAs of a stage (one accumulator per wave: 64 MFMAs, each waiting for the one before it -- the pipe's
// latency equals its occupancy for this instruction) and doubles the workgroups.  Per row the k order is that of the 64-row
// kernels: same bits.  Host-count mode only, no addend.
__global__ __launch_bounds__(256, 2) void packed_layer_pipe32_kernel(const PLBatch bt)
{
    const PLProblem pb = bt.p[blockIdx.z];
    const long rows = pb.rows_host;
    const int K = pb.K, N = pb.N;
    constexpr int R = 32;
    __shared__ float tiles[2 * R * PL_LD];
    const long t = blockIdx.x;
    const int n0 = blockIdx.y * 128;
    if (t * R >= rows || n0 >= pb.n_store) return;             // (a batched launch is sized for its largest problem)
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = tid & 31, r0 = tid >> 5;
    f32x16 acc0 = {0};
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void *)pb.W, 0, K * N * 4, 0x00020000);
    const unsigned int row_bytes = (unsigned int)N * 4u;
    const unsigned int lane_off = ((unsigned int)(64 * h) * (unsigned int)N + (unsigned int)(n0 + 32 * w + j)) * 4u;
    const long left = rows - t * R;
    const unsigned int a_row_bytes = (unsigned int)pb.lda * 4u;
    const __amdgpu_buffer_rsrc_t ars =
        __builtin_amdgcn_make_buffer_rsrc((void *)(pb.A + t * R * pb.lda), 0, (int)((left < R ? left : R) * (long)a_row_bytes), 0x00020000);
    const unsigned int a_lane = (unsigned int)r0 * a_row_bytes + 16u * chunk;
    float wa[64], wb[64];
    PL_LOAD_W(wa, 0)
    PL_FETCH_TILE(tiles, R / 8, 0)
    const int np = K >> 7;
    for (int p = 0; p < np; ++p) {
        PL_VM_DRAIN
        lds_barrier();
        const float *T = tiles + (p & 1) * (R * PL_LD);
        float *TN = tiles + ((p + 1) & 1) * (R * PL_LD);
        PL_STAGE_HEAD(T, PL_ONE_HALF)
        if (p + 1 < np) {
            PL_STAGE_GROUPS(wa, PL_ONE_HALF, f32x4 ar[4];, PL32_NEXT_PANEL(TN, wb, (p + 1) * 128) PL_FENCE)
#pragma unroll
            for (int s = 0; s < 64; ++s) wa[s] = wb[s];
        } else {
            PL_STAGE_GROUPS(wa, PL_ONE_HALF, PL_NO_SIDE, PL_FENCE)
        }
    }
    const float bcol = pb.bias[n0 + 32 * w + j];
    const int do_relu = pb.do_relu;
    __syncthreads();                                       // the panel tiles are dead: stage the results through one
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc0[r] + bcol;
        tiles[((r & 3) + 8 * (r >> 2) + 4 * h) * PL_LD + 32 * w + j] = do_relu ? fmaxf(v, 0.f) : v;
    }
    __syncthreads();
    pl_store_rows<R>(tiles, t, rows, n0, pb, false);
}

}  // namespace prcnn

using namespace prcnn;

// ---- the launch plan: which form serves a problem, and its grid.  The one statement of the rule; the thresholds are read here only.
namespace {
enum PLForm { PL_ONE, PL_PIPE, PL_PIPE32, PL_STREAM, PL_PERSIST };
struct PLPlan { PLForm form; long gx; int gy; };
long env_long(const char *v, long dflt) { return v ? atol(v) : dflt; }

// tiles: 64-row tiles (a list: max_tiles).  list: the row count lives on the device (hdr).  single: the call's only problem.
PLPlan pl_plan(const PLProblem &p, long tiles, bool segmax, bool single)
{
    static const long stream_min = env_long(getenv("PRCNN_PL_STREAM_MIN"), 512), stream_cap = env_long(getenv("PRCNN_PL_STREAM_CAP"), 512),
                      persist_min = env_long(getenv("PRCNN_PL_PERSIST_MIN"), 256);
    const int col_blocks = (p.n_store + 127) / 128;            // column blocks that hold nothing to store are not launched
    const long items = tiles * col_blocks;
    const bool host_plain = !p.hdr && !segmax;                 // only the one-tile 64-row kernels read a list's header or pool
    if (p.K == 128) {
        // one panel, many row tiles: resident weights, two workgroups per CU over all column blocks (32-bit offsets into A)
        if (host_plain && items >= stream_min && p.rows_host * p.lda * 4 < (1L << 31)) {
            const long cap = stream_cap / col_blocks > 0 ? stream_cap / col_blocks : 1;
            return {PL_STREAM, tiles < cap ? tiles : cap, col_blocks};
        }
        return {PL_ONE, tiles, col_blocks};
    }
    // fewer than 256 items: 32-row tiles -- that kernel has no addend, so FP layer 1 stays on 64 rows
    if (host_plain && !p.addG && items < 256) return {PL_PIPE32, (p.rows_host + 31) / 32, col_blocks};
    // more than one round of workgroups: the persistent pipeline -- it stores whole 128-column blocks (n_store == N) of ONE problem
    // (items <= workgroups: nothing to pipeline)
    if (host_plain && single && p.n_store == p.N && items > stream_cap && items >= persist_min)
        return {PL_PERSIST, items < stream_cap ? items : stream_cap, 1};
    return {PL_PIPE, tiles, col_blocks};
}

// one launch of form `form` over the k problems of bt (k > 1: the batchable forms only), grid (gx, gy, k)
int pl_launch(PLForm form, const PLBatch &bt, int k, long gx, int gy, bool segmax, hipStream_t st, const char *what)
{
    const dim3 grid((unsigned)gx, gy, k), wg(256);
    switch (form) {
    case PL_ONE:
        if (segmax) hipLaunchKernelGGL(packed_layer_kernel<true>, grid, wg, 0, st, bt);
        else hipLaunchKernelGGL(packed_layer_kernel<false>, grid, wg, 0, st, bt);
        break;
    case PL_PIPE:
        if (segmax) hipLaunchKernelGGL(packed_layer_pipe_kernel<true>, grid, wg, 0, st, bt);
        else hipLaunchKernelGGL(packed_layer_pipe_kernel<false>, grid, wg, 0, st, bt);
        break;
    case PL_PIPE32: hipLaunchKernelGGL(packed_layer_pipe32_kernel, grid, wg, 0, st, bt); break;
    case PL_STREAM: hipLaunchKernelGGL(packed_layer_stream_kernel, grid, wg, 0, st, bt.p[0]); break;
    case PL_PERSIST: {
        unsigned int *ticket = next_ticket(st);
        if (!ticket) { set_error("%s: cannot set up the item ticket", what); return PRCNN_ELAUNCH; }
        if (bt.p[0].addG) hipLaunchKernelGGL(packed_layer_persist_kernel<true>, grid, wg, 0, st, bt.p[0], ticket);
        else hipLaunchKernelGGL(packed_layer_persist_kernel<false>, grid, wg, 0, st, bt.p[0], ticket);
        break;
    }
    }
    return check_launch(what);
}

PLProblem pl_problem(const prcnn_layer_problem &q, bool segmax)
{
    PLProblem p = {};
    p.hdr = q.hdr; p.rows_host = q.rows; p.K = q.K; p.N = q.N; p.A = q.A; p.lda = q.lda; p.W = q.W; p.bias = q.bias;
    p.do_relu = segmax ? 1 : q.relu; p.out = q.out; p.ldo = q.ldo; p.n_store = segmax ? q.N : q.n_store;
    if (segmax) {
        p.rowinfo = q.rowinfo; p.tilecloud = q.tilecloud; p.m = q.m; p.out_col = q.out_col;
        p.lds_pool = (((uintptr_t)q.out | (uintptr_t)q.bias) & 15) == 0 && (q.ldo & 3) == 0 && (q.out_col & 3) == 0;
    }
    return p;
}
}  // namespace

// Layer problems (plain: out[r][0..n_store) = act(A[r][0..K) @ W + bias)[0..n_store); segmax: last layer of a level + max pool,
// out[(b*m)][out_col .. out_col + N) = max over each centre's packed rows of relu(A[r] @ W + bias) through atomicMax into a zeroed
// slice).  K and N multiples of 128, W (K,N) k-major, n_store <= N (the caller pads a narrow last layer's weights to N = 128 and
// asks for its real width).  Row count: hdr != NULL -> hdr[0] * 64 rows (a packed list; max_tiles sizes the grid), else `rows`
// (host count).  Up to 4 problems that land on the same batchable form share ONE launch (grid.z); others are launched one by one.
extern "C" int prcnn_packed_layer_batch(int nprob, const prcnn_layer_problem *pr, int segmax, void *stream)
{
    PRCNN_REQUIRE(nprob >= 0 && nprob <= PL_MAX_BATCH && (nprob == 0 || pr), "packed_layer: 0..%d problems", PL_MAX_BATCH);
    hipStream_t st = (hipStream_t)stream;
    const char *what = segmax ? "packed_layer_segmax" : "packed_layer";
    PLBatch bt;
    long tiles_of[PL_MAX_BATCH];
    int k = 0;
    for (int i = 0; i < nprob; ++i) {
        const prcnn_layer_problem &q = pr[i];
        PRCNN_REQUIRE(q.K > 0 && q.N > 0 && q.K % 128 == 0 && q.N % 128 == 0, "packed_layer: K=%d, N=%d must be multiples of 128", q.K, q.N);
        PRCNN_REQUIRE(q.lda >= q.K && q.lda % 4 == 0, "packed_layer: bad leading dimension of A");
        long tiles;
        if (segmax) {
            PRCNN_REQUIRE(q.b >= 0 && q.m >= 0 && q.max_tiles >= 0 && q.out_col >= 0 && q.ldo >= q.out_col + q.N, "packed_layer_segmax: bad layout");
            if ((long)q.b * q.m == 0) continue;
            PRCNN_REQUIRE(q.A && q.W && q.bias && q.rowinfo && q.tilecloud && q.hdr && q.out, "packed_layer_segmax: null pointer");
            PRCNN_REQUIRE(((uintptr_t)q.A & 15) == 0 && q.max_tiles <= 0x7fffffffL, "packed_layer_segmax: alignment / size");
            if (!q.out_is_zero && hipMemset2DAsync(q.out + q.out_col, (size_t)q.ldo * sizeof(float), 0, (size_t)q.N * sizeof(float),
                                                    (size_t)q.b * q.m, st) != hipSuccess) {
                set_error("packed_layer_segmax: cannot zero the output slice");
                return PRCNN_ELAUNCH;
            }
            tiles = q.max_tiles;
        } else {
            PRCNN_REQUIRE(q.n_store >= 1 && q.n_store <= q.N && q.ldo >= q.n_store, "packed_layer: n_store=%d outside 1..N (or ldo too small)", q.n_store);
            tiles = q.hdr ? q.max_tiles : (q.rows + PL_ROWS - 1) / PL_ROWS;
            PRCNN_REQUIRE(tiles >= 0 && tiles <= 0x7fffffffL && q.rows >= 0, "packed_layer: bad row count");
            if (tiles > 0) {
                PRCNN_REQUIRE(q.A && q.W && q.bias && q.out, "packed_layer: null pointer");
                PRCNN_REQUIRE(((uintptr_t)q.A & 15) == 0 && (((uintptr_t)q.out & 15) == 0 || (q.ldo & 3) != 0), "packed_layer: 16-byte alignment required");
            }
        }
        if (tiles == 0) continue;
        tiles_of[k] = tiles;
        bt.p[k++] = pl_problem(q, segmax);
    }
    if (k == 0) return PRCNN_OK;
    PLPlan plan[PL_MAX_BATCH];
    bool together = true;                                      // every problem on the same form, and that form takes a batch
    long gx = 0;
    int gy = 0;
    for (int i = 0; i < k; ++i) {
        plan[i] = pl_plan(bt.p[i], tiles_of[i], segmax, k == 1);
        together = together && plan[i].form == plan[0].form && (plan[i].form == PL_ONE || plan[i].form == PL_PIPE || plan[i].form == PL_PIPE32);
        if (plan[i].gx > gx) gx = plan[i].gx;                  // (a batched launch is sized for its largest problem)
        if (plan[i].gy > gy) gy = plan[i].gy;
    }
    if (together || k == 1) return pl_launch(plan[0].form, bt, k, gx, gy, segmax, st, what);
    for (int i = 0; i < k; ++i) {
        PLBatch one;
        one.p[0] = bt.p[i];
        const int rc = pl_launch(plan[i].form, one, 1, plan[i].gx, plan[i].gy, segmax, st, what);
        if (rc != PRCNN_OK) return rc;
    }
    return PRCNN_OK;
}

extern "C" int prcnn_packed_layer(const unsigned int *hdr, long rows, long max_tiles, int K, int N, int n_store, const float *A,
                                  long lda, const float *W, const float *bias, int relu, float *out, long ldo, void *stream)
{
    prcnn_layer_problem q = {};
    q.hdr = hdr; q.rows = rows; q.max_tiles = max_tiles; q.K = K; q.N = N; q.n_store = n_store; q.A = A; q.lda = lda; q.W = W;
    q.bias = bias; q.relu = relu; q.out = out; q.ldo = ldo;
    return prcnn_packed_layer_batch(1, &q, 0, stream);
}

extern "C" int prcnn_packed_layer_segmax(int b, int m, long max_tiles, int K, int N, const float *A, long lda, const float *W,
                                         const float *bias, const unsigned int *rowinfo, const int *tilecloud,
                                         const unsigned int *hdr, float *out, int out_stride, int out_col, int out_is_zero, void *stream)
{
    prcnn_layer_problem q = {};
    q.hdr = hdr; q.max_tiles = max_tiles; q.K = K; q.N = N; q.n_store = N; q.A = A; q.lda = lda; q.W = W; q.bias = bias; q.relu = 1;
    q.out = out; q.ldo = out_stride; q.b = b; q.m = m; q.rowinfo = rowinfo; q.tilecloud = tilecloud; q.out_col = out_col;
    q.out_is_zero = out_is_zero;
    return prcnn_packed_layer_batch(1, &q, 1, stream);
}


// The first layer of a feature-propagation module WITHOUT the interpolated tensor.  The reference interpolates the coarse
// level's features to the fine level, concatenates the skip features and applies the layer (pointnet2_modules.py:139-156):
// relu(W [interp(f) | skip] + b).  The layer is linear in front of its ReLU and the interpolation is a weighted sum, so
//     W_a interp(f) = interp(W_a f):   G = f @ W_a at the COARSE level (a quarter of the rows), then
//     out[r] = relu((skip[r] @ W_b + b) + ((w0 G[i0] + w1 G[i1]) + w2 G[i2]))     -- this entry, the addend inside the layer's epilogue.
// A (rows, K) = the skip features, W (K, N) = W_b, G (clouds * m_known rows, N wide, leading dimension ldg), idx / weight (rows, 3) from
// three_nn, row r in cloud r / n_per_cloud.  Not the reference's order of operations (the products are summed in another
// association): results agree to ~1e-7 relative, inside BASELINE's 1e-4 box tolerance; oracle/ext_cpu.py restates THIS order.
extern "C" int prcnn_packed_layer_interp(long rows, int K, int N, const float *A, long lda, const float *W, const float *bias, int relu,
                                         float *out, long ldo, int n_per_cloud, int m_known, const float *G, long ldg, const int *idx,
                                         const float *weight, void *stream)
{
    PRCNN_REQUIRE(rows >= 0 && K > 0 && N > 0 && K % 128 == 0 && N % 128 == 0, "packed_layer_interp: K=%d, N=%d must be multiples of 128", K, N);
    PRCNN_REQUIRE(lda >= K && lda % 4 == 0 && ldo >= N && ldo % 4 == 0 && ldg >= N && ldg % 4 == 0, "packed_layer_interp: bad leading dimensions");
    PRCNN_REQUIRE(n_per_cloud >= 1 && m_known >= 1 && rows % n_per_cloud == 0, "packed_layer_interp: rows must be whole clouds");
    if (rows == 0) return PRCNN_OK;
    PRCNN_REQUIRE(A && W && bias && out && G && idx && weight, "packed_layer_interp: null pointer");
    PRCNN_REQUIRE((((uintptr_t)A | (uintptr_t)out | (uintptr_t)G) & 15) == 0, "packed_layer_interp: 16-byte alignment required");
    const long tiles = (rows + PL_ROWS - 1) / PL_ROWS;
    PRCNN_REQUIRE(tiles <= 0x7fffffffL, "packed_layer_interp: too many rows");
    prcnn_layer_problem q = {};
    q.rows = rows; q.K = K; q.N = N; q.n_store = N; q.A = A; q.lda = lda; q.W = W; q.bias = bias; q.relu = relu; q.out = out; q.ldo = ldo;
    PLBatch bt;
    PLProblem &p = bt.p[0] = pl_problem(q, false);
    p.addG = G; p.addIdx = idx; p.addW = weight; p.add_n = n_per_cloud; p.add_m = m_known; p.add_ldg = ldg;
    const PLPlan plan = pl_plan(p, tiles, false, true);
    return pl_launch(plan.form, bt, 1, plan.gx, plan.gy, false, (hipStream_t)stream, "packed_layer_interp");
}
