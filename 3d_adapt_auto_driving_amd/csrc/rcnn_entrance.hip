// rcnn_entrance.hip -- the per-point MLP chain at the entrance of the RCNN (lib/net/rcnn_net.py:139-163: xyz_up_layer on
// [x', y', z', mask, depth], concatenation with the RPN features, merge_down_layer) fused with the per-point part of the first SA
// level's layer 1:
//
//   X = relu(relu(in5 @ Wu1 + bu1) @ Wu2 + bu2)                                                (rows x 128)
//   P = relu([X | F] @ Wm + bm) @ Wp + bp = relu(X @ Wm_a + F @ Wm_b + bm) @ Wp + bp
//
// where F are the 128 RPN features of the pooled row and P is what csrc/sa_mlp_fused.hip gathers for SA1
// ("linear before ReLU": W1 [f ; x - c] + b1 = (W1f f + b1) + W1x (x - c)).  The library path did this with four
// GEMMs and a 420 MB concatenation, all of them persistent-grid kernels that stretch by 40-70 % when the geometry
// stream co-runs; here `merged` never exists and the workgroups are short-lived (ticketed tiles) like those of sa_mlp_fused.
// Two forms: three launches of rows_layer_kernel (csrc/rows_layer.hip; X and merged go through HBM), or -- when only P is wanted --
// rcnn_entrance_kernel, where the tile never leaves LDS.  With them the makers of the lists the fused form runs over.
#include "sa_tile.hpp"
#include "mfma_stream.hpp"

namespace prcnn {

// ---- the whole entrance chain over a tile that stays in LDS (round 2, after the stage stamps of csrc/rpn_tail.hip) -----------
// Per 64-row tile: builder (first xyz_up layer, K = 5, VALU; the tile's 128 RPN features go to the second LDS tile) ->
// xyz_up layer 2 -> merge_down over [xfeat | feats] (two panels into one accumulator) -> SA1's per-point part; only P leaves
// the CU.  Four panel stages per tile, each one's 128 x 32 weight slice per wave streaming in behind the MFMAs of the stage
// before it (mfma_stream.hpp); persistent workgroups draw the live tiles from a ticket counter.  Arithmetic per row = the three
// rows_layer_kernel launches, bit for bit (same builder chain, same panel order, same epilogues).
// SRC (over a row list only): the rows carry no features (ld = 8, csrc/roipool.hip's SRC form); list entry e takes them from row
// featmap[e] of `feats`, the RPN's own (points, 128) feature matrix, a negative entry = a zero row (the one listed row of an empty box).
// The same 16 bytes reach the same place of T1: from the first barrier on the two forms are one text.
template <bool SRC>
__global__ __launch_bounds__(256, 2) void rcnn_entrance_kernel(
    long tiles, const float *__restrict__ rows, int ld, int fcol, const float4 *__restrict__ wu1, const float4 *__restrict__ bu1,
    const float *__restrict__ wu2, const float *__restrict__ bu2, const float *__restrict__ wm, const float *__restrict__ bm,
    const float *__restrict__ wp, const float *__restrict__ bp, float *__restrict__ p_out, unsigned int *__restrict__ ticket,
    const int *__restrict__ tilemap, const unsigned int *__restrict__ ntiles_dev, const int *__restrict__ rowmap,
    const float *__restrict__ feats, const int *__restrict__ featmap)
{
    // rowmap != NULL (round 5, prcnn_rcnn_point_mlp_rows): tile t = the rows rowmap[64 t .. 64 t + 63] of `rows` / `p_out` -- the
    // DISTINCT pooled rows of all RoIs back to back (prcnn_pooled_rows), ntiles_dev[1] of them; the last tile's missing entries repeat
    // the list's last row (computed and stored again: the same values to the same place).  With whole 64-row tiles per RoI
    // (tilemap) a RoI's 47 distinct rows of 512 filled a tile of 64; per row the arithmetic does not depend on the tile: same bits.
    long nrows = 0;
    if (rowmap) { nrows = (long)ntiles_dev[1]; tiles = (nrows + RT_ROWS - 1) / RT_ROWS; }
    else if (ntiles_dev) tiles = (long)*ntiles_dev;
    __shared__ float T0[RT_ROWS * RT_LD];
    __shared__ float T1[RT_ROWS * RT_LD];
    __shared__ unsigned int slot[2];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunk = tid & 31, r0 = tid >> 5;
    const unsigned int lane_off = RT_LANE_OFF(32 * w + j);
    const __amdgpu_buffer_rsrc_t rs_u2 = __builtin_amdgcn_make_buffer_rsrc((void *)wu2, 0, 128 * 128 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc((void *)wm, 0, 256 * 128 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_p = __builtin_amdgcn_make_buffer_rsrc((void *)wp, 0, 128 * 128 * 4, 0x00020000);
    const float bias_u2 = bu2[32 * w + j], bias_m = bm[32 * w + j], bias_p = bp[32 * w + j];
    float4 k1[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) k1[k] = wu1[k * 32 + chunk];
    const float4 b1 = bu1[chunk];

    long t = __builtin_amdgcn_readfirstlane((int)sa_first_ticket(slot, ticket, tid));
    float wa[64], wb[64];
    f32x16 acc0, acc1;
    RT_LOAD_W(wa, rs_u2, 0)
    int ridx[8], nidx[8];                                      // this thread's 8 rows of the running tile / of the next one
    int fidx[SRC ? 8 : 1], nfidx[SRC ? 8 : 1];                 // SRC: ... and their feature rows
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ridx[i] = (rowmap && t < tiles) ? rowmap[min(t * RT_ROWS + r0 + 8 * i, nrows - 1)] : 0;
        if constexpr (SRC) fidx[i] = t < tiles ? featmap[min(t * RT_ROWS + r0 + 8 * i, nrows - 1)] : -1;
    }
    for (unsigned int served = 0; t < tiles; ++served) {
        if (!rowmap) {
            const long tt = tilemap ? (long)tilemap[t] : t;
#pragma unroll
            for (int i = 0; i < 8; ++i) ridx[i] = (int)(tt * RT_ROWS + r0 + 8 * i);
        }
        // ---- builder: layer 1 of xyz_up from the 5 input columns -> T0, the row's RPN features -> T1
        {
            float4 q[8], f[8];
            float d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float *row = rows + (long)ridx[i] * (long)ld;
                q[i] = *reinterpret_cast<const float4 *>(row);
                d[i] = row[4];
                if constexpr (SRC) f[i] = *reinterpret_cast<const float4 *>(feats + (long)max(fidx[i], 0) * PK_C + 4 * chunk);
                else f[i] = *reinterpret_cast<const float4 *>(row + fcol + 4 * chunk);
            }
            // the next tile's ticket rides behind the loads (a persistent workgroup: it draws until the tickets run out, so this is
            // not sa_next_ticket, which stops at a workgroup's quota)
            if (tid == 0) slot[(served + 1) & 1] = atomicAdd(ticket, 1u);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float4 v;
                v = relu4(pk_fma4(k1[4], d[i], pk_fma4(k1[3], q[i].w, pk_fma4(k1[2], q[i].z, pk_fma4(k1[1], q[i].y, pk_fma4(k1[0], q[i].x, b1))))));
                *reinterpret_cast<float4 *>(T0 + (r0 + 8 * i) * RT_LD + 4 * chunk) = v;
                if constexpr (SRC)                                 // (a select: whatever row 0 holds, a NaN included, is dropped)
                    if (fidx[i] < 0) f[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4 *>(T1 + (r0 + 8 * i) * RT_LD + 4 * chunk) = f[i];
            }
        }
        RT_VM_DRAIN                                            // (also: this tile's first panel, fetched during the last stage)
        lds_barrier();
        if (rowmap) {                                          // the next tile's row numbers: in flight behind the first stage
            const long tq = (long)__builtin_amdgcn_readfirstlane((int)slot[(served + 1) & 1]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                nidx[i] = tq < tiles ? rowmap[min(tq * RT_ROWS + r0 + 8 * i, nrows - 1)] : 0;
                if constexpr (SRC) nfidx[i] = tq < tiles ? featmap[min(tq * RT_ROWS + r0 + 8 * i, nrows - 1)] : -1;
            }
        }
        // ---- xyz_up layer 2 (wa) while merge panel a (wb) comes in
        RT_STAGE(T0, wa, wb, rs_m, 0, true)
        lds_barrier();                                         // every wave has read the layer-1 rows
        RT_EPILOGUE(T0, bias_u2, true)
        lds_barrier();
        // ---- merge_down: [xfeat | feats] as two panels into one accumulator
        RT_VM_DRAIN
        RT_STAGE(T0, wb, wa, rs_m, 128, true)
        RT_VM_DRAIN
        RT_STAGE(T1, wa, wb, rs_p, 0, false)
        lds_barrier();                                         // every wave has read xfeat
        RT_EPILOGUE(T0, bias_m, true)
        lds_barrier();
        // ---- SA1's per-point part (no activation) while the next tile's first panel (wa) comes in
        RT_VM_DRAIN
        RT_STAGE(T0, wb, wa, rs_u2, 0, true)
        RT_EPILOGUE(T1, bias_p, false)
        lds_barrier();
        RT_STORE_ROWS8(f32x4, T1, p_out, (long)ridx[i])
        const long tn = __builtin_amdgcn_readfirstlane((int)slot[(served + 1) & 1]);
        lds_barrier();                                         // T1 is free for the next builder
        t = tn;
        if (rowmap) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ridx[i] = nidx[i];
                if constexpr (SRC) fidx[i] = nfidx[i];
            }
        }
    }
    if (tid == 0) ticket_release(ticket);          // the launch's last workgroup zeroes the counter for the word's next user
}

// cnt[c] distinct rows of cloud c (rows_per_cloud rows each, a multiple of 64) -> the list of 64-row tiles that hold
// them, in cloud order: tilemap[j], j < hdr[0].  One workgroup, clouds in chunks of 1024 with a running offset.
__global__ __launch_bounds__(1024) void pooled_tiles_kernel(int clouds, int rows_per_cloud, const int *__restrict__ cnt,
                                                            int *__restrict__ tilemap, unsigned int *__restrict__ hdr)
{
    __shared__ int part[1024];
    __shared__ int s_run;
    const int tid = threadIdx.x, per = rows_per_cloud / RT_ROWS;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < clouds; c0 += 1024) {
        const int c = c0 + tid;
        const int live = c < clouds ? min(per, (max(cnt[c], 1) + RT_ROWS - 1) / RT_ROWS) : 0;
        part[tid] = live;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int v = tid >= d ? part[tid - d] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        const int base = s_run + part[tid] - live;
        for (int q = 0; q < live; ++q) tilemap[base + q] = c * per + q;
        __syncthreads();
        if (tid == 1023) s_run += part[1023];
        __syncthreads();
    }
    if (tid == 0) hdr[0] = (unsigned int)s_run;
}

// cnt[c] distinct rows of cloud c -> the list of those rows (row c * rows_per_cloud + j, j < max(cnt[c], 1)) of ALL clouds back to back:
// rowmap[0 .. hdr[1]).  A wave per cloud draws its block from the list's row counter hdr[1] (zero on entry): the order of the clouds in
// the list is the counter's, every row of the input is computed on its own.  featmap (optional): src[row] of every listed row beside it,
// the row of the feature matrix that csrc/roipool.hip's SRC form names for it.
__global__ __launch_bounds__(256) void pooled_rows_kernel(int clouds, int rows_per_cloud, const int *__restrict__ cnt, int *__restrict__ rowmap,
                                                          unsigned int *__restrict__ hdr, const int *__restrict__ src, int *__restrict__ featmap)
{
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= clouds) return;
    const int n = min(max(cnt[c], 1), rows_per_cloud);
    int base = 0;
    if (lane == 0) base = (int)atomicAdd(&hdr[1], (unsigned int)n);
    base = __builtin_amdgcn_readfirstlane(base);
    for (int j = lane; j < n; j += 64) {
        rowmap[base + j] = c * rows_per_cloud + j;
        if (featmap) featmap[base + j] = src[c * rows_per_cloud + j];
    }
}

// ... of the distinct rows only those that the set `used` names (words u32 per cloud, bit j = row j of the cloud; csrc/roi_geometry.hip's
// used0: the pooled points that a kept row of SA level 1's list reads) -- in row order, compacted by ballot and prefix popcount
__global__ __launch_bounds__(256) void pooled_rows_live_kernel(int clouds, int rows_per_cloud, int words, const int *__restrict__ cnt,
                                                               const unsigned int *__restrict__ used, int *__restrict__ rowmap,
                                                               unsigned int *__restrict__ hdr, const int *__restrict__ src, int *__restrict__ featmap)
{
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= clouds) return;
    const int n = min(max(cnt[c], 1), rows_per_cloud);
    const unsigned int *__restrict__ u = used + (long)c * words;
    int total = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        total += (int)__builtin_popcountll(__ballot(j < n && ((u[j >> 5] >> (j & 31)) & 1u)));
    }
    int base = 0;
    if (lane == 0) base = (int)atomicAdd(&hdr[1], (unsigned int)total);
    base = __builtin_amdgcn_readfirstlane(base);
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const bool on = j < n && ((u[j >> 5] >> (j & 31)) & 1u);
        const unsigned long long m = __ballot(on);
        if (on) {
            const int e = base + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            rowmap[e] = c * rows_per_cloud + j;
            if (featmap) featmap[e] = src[c * rows_per_cloud + j];
        }
        base += (int)__builtin_popcountll(m);
    }
}

}  // namespace prcnn

using namespace prcnn;

// what prcnn_rcnn_point_mlp and prcnn_rcnn_point_mlp_rows ask of their common arguments; *run = false: nothing to do (r == 0).
// fused: the chain runs in rcnn_entrance_kernel, whose weight slices come in as 16-byte aligned buffers.  fcol < 0: rows without features.
static int entrance_check(const char *who, long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1, const float *wu2,
                          const float *bu2, const float *wm, const float *bm, const float *wp, const float *bp, const float *p, bool fused,
                          bool *run)
{
    *run = false;
    PRCNN_REQUIRE(r >= 0 && r % RT_ROWS == 0, "%s: %ld rows is not a multiple of %d", who, r, RT_ROWS);
    PRCNN_REQUIRE(ld >= 8 && ld % 4 == 0 && (fcol < 0 || (fcol >= 8 && fcol % 4 == 0 && fcol + PK_C <= ld)), "%s: bad row layout ld=%d fcol=%d", who, ld, fcol);
    if (r == 0) return PRCNN_OK;
    PRCNN_REQUIRE(rows && wu1 && bu1 && wu2 && bu2 && wm && bm && wp && bp && p, "%s: null pointer", who);
    PRCNN_REQUIRE((((uintptr_t)rows | (uintptr_t)wu1 | (uintptr_t)bu1 | (uintptr_t)p) & 15) == 0 &&
                  (!fused || (((uintptr_t)wu2 | (uintptr_t)wm | (uintptr_t)wp) & 15) == 0), "%s: 16-byte alignment required", who);
    *run = true;
    return PRCNN_OK;
}

// the fused chain over r / 64 tiles at most: whole tiles, the tiles of a tile map (tilemap, hdr[0]) or the rows of a list (rowmap, hdr[1]);
// featmap (with a list only): the listed rows' features come from rows featmap[e] of `feats`
static int entrance_launch(const char *who, long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1, const float *wu2,
                           const float *bu2, const float *wm, const float *bm, const float *wp, const float *bp, float *p, const int *tilemap,
                           const unsigned int *hdr, const int *rowmap, const float *feats, const int *featmap, hipStream_t st)
{
    const long tiles = r / RT_ROWS;                            // at most, where a list on the device says how many
    unsigned int *tk = next_ticket(st);
    if (!tk) { set_error("%s: cannot set up the tile ticket", who); return PRCNN_ELAUNCH; }
    const long grid = tiles < mfma_grid_cap() ? tiles : mfma_grid_cap();
    auto kernel = featmap ? rcnn_entrance_kernel<true> : rcnn_entrance_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, tiles, rows, ld, fcol, (const float4 *)wu1, (const float4 *)bu1, wu2,
                       bu2, wm, bm, wp, bp, p, tk, tilemap, hdr, rowmap, feats, featmap);
    return check_launch(who);
}

// rows (r, ld) f32 = the pooled RCNN input rows [x',y',z',mask,depth,0,0,0 | 128 features at column fcol] (r % 64 == 0);
// wu1 (8,128), wu2 (128,128), wm (256,128) = [Wm_a ; Wm_b], wp (128,128): k-major, BN folded.  Three launches of
// rows_layer_kernel:   xfeat  = relu(relu(in5 wu1 + bu1) wu2 + bu2)            (xyz_up_layer)
//                      merged = relu(xfeat wm_a + feats wm_b + bm)               (concat + merge_down_layer)
//                      p      = merged wp + bp                                   (per-point part of SA1's layer 1)
// xfeat, merged, p: (r,128) each, caller-allocated.  xfeat = merged = NULL: only P is wanted, the fused kernel.
extern "C" int prcnn_rcnn_point_mlp(long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1,
                                    const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                                    const float *bp, float *xfeat, float *merged, float *p, const int *tilemap,
                                    const unsigned int *ntiles, void *stream)
{
    PRCNN_REQUIRE((tilemap == nullptr) == (ntiles == nullptr), "rcnn_point_mlp: tilemap and ntiles go together");
    bool run;
    int rc = entrance_check("rcnn_point_mlp", r, ld, fcol, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, !xfeat && !merged, &run);
    if (rc != PRCNN_OK || !run) return rc;
    PRCNN_REQUIRE((xfeat == nullptr) == (merged == nullptr), "rcnn_point_mlp: xfeat and merged are both given or both NULL");
    PRCNN_REQUIRE((((uintptr_t)xfeat | (uintptr_t)merged) & 15) == 0, "rcnn_point_mlp: 16-byte alignment required");
    hipStream_t st = (hipStream_t)stream;
    if (!xfeat) return entrance_launch("rcnn_point_mlp(fused)", r, ld, fcol, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, tilemap, ntiles, nullptr, nullptr, nullptr, st);
    const long tiles = r / RT_ROWS;
    rc = rows_layer_launch(1, 1, true, tiles, rows, ld, 0, nullptr, 0, 0, wu1, bu1, wu2, nullptr, bu2, xfeat, tilemap, ntiles, st,
                           "rcnn_point_mlp(xyz_up)");
    if (rc != PRCNN_OK) return rc;
    rc = rows_layer_launch(2, 0, true, tiles, xfeat, PK_C, 0, rows, ld, fcol, nullptr, nullptr, wm, wm + (size_t)PK_C * PK_C, bm, merged, tilemap,
                           ntiles, st, "rcnn_point_mlp(merge)");
    if (rc != PRCNN_OK) return rc;
    return rows_layer_launch(1, 0, false, tiles, merged, PK_C, 0, nullptr, 0, 0, nullptr, nullptr, wp, nullptr, bp, p, tilemap, ntiles, st,
                             "rcnn_point_mlp(sa1 per-point)");
}

// The fused entrance chain (only p) over a LIST of rows: rowmap[0 .. hdr[1]) from prcnn_pooled_rows -- tiles of 64 list entries, whichever
// RoIs they belong to.  p rows that are not listed are left as they are.
extern "C" int prcnn_rcnn_point_mlp_rows(long r, int ld, int fcol, const float *rows, const float *wu1, const float *bu1,
                                         const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                                         const float *bp, float *p, const int *rowmap, const unsigned int *hdr, void *stream)
{
    PRCNN_REQUIRE(r <= 0x7fffffffL, "rcnn_point_mlp_rows: %ld rows: the list holds 32-bit row numbers", r);
    bool run;
    const int rc = entrance_check("rcnn_point_mlp_rows", r, ld, fcol, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, true, &run);
    if (rc != PRCNN_OK || !run) return rc;
    PRCNN_REQUIRE(rowmap && hdr, "rcnn_point_mlp_rows: null pointer");
    return entrance_launch("rcnn_point_mlp_rows", r, ld, fcol, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, nullptr, hdr, rowmap, nullptr, nullptr,
                           (hipStream_t)stream);
}

// ... over rows that carry no features (r, ld >= 8: [x',y',z',mask,depth, ...], prcnn_roipool3d_canonical_src): list entry e takes its 128
// features from row featmap[e] of feats (any number of rows, 128 wide), zeros where featmap[e] < 0 (prcnn_pooled_rows_src).  Same chain, same bits.
extern "C" int prcnn_rcnn_point_mlp_rows_src(long r, int ld, const float *rows, const float *feats, const float *wu1, const float *bu1,
                                             const float *wu2, const float *bu2, const float *wm, const float *bm, const float *wp,
                                             const float *bp, float *p, const int *rowmap, const int *featmap, const unsigned int *hdr,
                                             void *stream)
{
    PRCNN_REQUIRE(r <= 0x7fffffffL, "rcnn_point_mlp_rows_src: %ld rows: the list holds 32-bit row numbers", r);
    bool run;
    const int rc = entrance_check("rcnn_point_mlp_rows_src", r, ld, -1, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, true, &run);
    if (rc != PRCNN_OK || !run) return rc;
    PRCNN_REQUIRE(rowmap && featmap && hdr && feats, "rcnn_point_mlp_rows_src: null pointer");
    PRCNN_REQUIRE(((uintptr_t)feats & 15) == 0, "rcnn_point_mlp_rows_src: 16-byte alignment required");
    return entrance_launch("rcnn_point_mlp_rows_src", r, ld, 0, rows, wu1, bu1, wu2, bu2, wm, bm, wp, bp, p, nullptr, hdr, rowmap, feats, featmap,
                           (hipStream_t)stream);
}

// cnt (clouds) i32 -> rowmap (clouds * rows_per_cloud entries at most), hdr[1] = number of listed rows (hdr (4 u32) zeroed here unless
// hdr_is_zero): the distinct pooled rows of all clouds back to back, for prcnn_rcnn_point_mlp_rows.
// src / featmap (optional, both or neither; prcnn_pooled_rows_src): src (clouds * rows_per_cloud) i32 -> featmap[e] = src[rowmap[e]] in the same pass.
extern "C" int prcnn_pooled_rows_src(int clouds, int rows_per_cloud, const int *cnt, const int *src, int *rowmap, int *featmap, unsigned int *hdr,
                                     int hdr_is_zero, void *stream)
{
    PRCNN_REQUIRE(clouds >= 0 && rows_per_cloud > 0 && (long)clouds * rows_per_cloud <= 0x7fffffffL, "pooled_rows: bad sizes");
    PRCNN_REQUIRE(hdr && (clouds == 0 || (cnt && rowmap)), "pooled_rows: null pointer");
    PRCNN_REQUIRE((src == nullptr) == (featmap == nullptr), "pooled_rows: src and featmap go together");
    hipStream_t st = (hipStream_t)stream;
    if (!hdr_is_zero && hipMemsetAsync(hdr, 0, 4 * sizeof(unsigned int), st) != hipSuccess) { set_error("pooled_rows: memset failed"); return PRCNN_ELAUNCH; }
    if (clouds == 0) return PRCNN_OK;
    hipLaunchKernelGGL(pooled_rows_kernel, dim3((clouds + 3) / 4), dim3(256), 0, st, clouds, rows_per_cloud, cnt, rowmap, hdr, src, featmap);
    return check_launch("pooled_rows");
}

// prcnn_pooled_rows_src over the LIVE rows only: used (clouds * ceil(rows_per_cloud / 32)) u32, bit j of a cloud's words = row j of it is
// read (prcnn_rcnn_roi_geometry_live's used0 for clouds of 512 rows) -> the listed rows are those j < max(cnt[c], 1) whose bit is set, in
// row order per cloud.  Same header protocol, same counter; a cloud whose set is empty lists nothing.
extern "C" int prcnn_pooled_rows_src_live(int clouds, int rows_per_cloud, const int *cnt, const unsigned int *used, const int *src, int *rowmap,
                                          int *featmap, unsigned int *hdr, int hdr_is_zero, void *stream)
{
    PRCNN_REQUIRE(clouds >= 0 && rows_per_cloud > 0 && (long)clouds * rows_per_cloud <= 0x7fffffffL, "pooled_rows_live: bad sizes");
    PRCNN_REQUIRE(hdr && (clouds == 0 || (cnt && used && rowmap)), "pooled_rows_live: null pointer");
    PRCNN_REQUIRE((src == nullptr) == (featmap == nullptr), "pooled_rows_live: src and featmap go together");
    hipStream_t st = (hipStream_t)stream;
    if (!hdr_is_zero && hipMemsetAsync(hdr, 0, 4 * sizeof(unsigned int), st) != hipSuccess) { set_error("pooled_rows_live: memset failed"); return PRCNN_ELAUNCH; }
    if (clouds == 0) return PRCNN_OK;
    hipLaunchKernelGGL(pooled_rows_live_kernel, dim3((clouds + 3) / 4), dim3(256), 0, st, clouds, rows_per_cloud, (rows_per_cloud + 31) / 32, cnt,
                       used, rowmap, hdr, src, featmap);
    return check_launch("pooled_rows_live");
}

extern "C" int prcnn_pooled_rows(int clouds, int rows_per_cloud, const int *cnt, int *rowmap, unsigned int *hdr, int hdr_is_zero, void *stream)
{
    return prcnn_pooled_rows_src(clouds, rows_per_cloud, cnt, nullptr, rowmap, nullptr, hdr, hdr_is_zero, stream);
}

// cnt (clouds) i32 distinct rows per cloud of rows_per_cloud rows (prcnn_roipool3d_canonical's pooled_cnt) -> tilemap
// (clouds * rows_per_cloud / 64 entries at most) and hdr[0] = number of live 64-row tiles, for prcnn_rcnn_point_mlp.
extern "C" int prcnn_pooled_tiles(int clouds, int rows_per_cloud, const int *cnt, int *tilemap, unsigned int *hdr, void *stream)
{
    PRCNN_REQUIRE(clouds >= 0 && rows_per_cloud > 0 && rows_per_cloud % RT_ROWS == 0, "pooled_tiles: bad sizes");
    PRCNN_REQUIRE(hdr && (clouds == 0 || (cnt && tilemap)), "pooled_tiles: null pointer");
    hipLaunchKernelGGL(pooled_tiles_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, clouds, rows_per_cloud, cnt, tilemap, hdr);
    return check_launch("pooled_tiles");
}
