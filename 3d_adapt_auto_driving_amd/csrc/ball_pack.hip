// ball_pack.hip -- the DISTINCT grouped rows of a ball query's answer as a dense row list: what every packed kernel of the library
// reads (csrc/sa_packed.hip, csrc/packed_layer.hip, csrc/sa_wide.hip, csrc/sa_wide3.hip).
//
// The reference's ball query back-fills every slot beyond the hit count with the FIRST hit
// (ball_query_gpu.cu:35-39), and QueryAndGroup / SharedMLP / max_pool2d (pointnet2_utils.py:241-264,
// pointnet2_modules.py:37-53) then push all nsample rows of a group through the three layers -- although the
// back-filled rows are exact copies of row 0 and the max over a group does not change when copies are dropped.
// On the RCNN levels of a KITTI-shaped scene a ball of nsample = 64 holds ~14 (SA1) / ~7 (SA2) distinct
// points; on real clouds it is rarely full either.  So per cloud: cnt[c] = 1 + (last slot that differs from slot 0), exclusive scan,
// the cloud's rows written as a dense list of (centre, point) pairs cut into 64-row tiles.  `cnt` is defined so that the pooled output
// is the unpacked one for ANY index tensor: rows beyond the last slot that differs from slot 0 are copies of row 0 whatever produced them.
//
// idx (b,m,nsample) i32 -> the distinct grouped rows of every cloud as 64-row tiles:
//   rowinfo  [b * tiles_cap * 64] u32, (centre within cloud) << 16 | (point within cloud); tile t = entries [64t, 64t+64)
//   rowdxyz  [b * tiles_cap * 64] float4, xyz[point] - new_xyz[centre] of the same rows (w = 0)
//   tilecloud[b * tiles_cap] i32, cloud of tile t
//   hdr      [4] u32: [0] = number of tiles, [1] = number of distinct rows (both written by this call)
// with tiles_cap = ceil(m * nsample / 64) tiles per cloud at most.  Needs m <= 15360 centres and n <= 65536 points per cloud (both
// refused otherwise; rowinfo keeps the point in 16 bits).  tests/row_lists.py restates the list in numpy: the definition every
// producer is compared with row for row (tests/test_gpu_row_lists.py).
#include "common.hpp"
#include "sa_tile.hpp"

namespace prcnn {

// `limit` (optional, per cloud): the points k >= limit[cloud] of the cloud are COPIES of point k % limit[cloud] (the
// wrap-around fill of RoI pooling, roipool3d_kernel.cu:152-159).  A copy lies in a ball iff its original does, and the
// original has the lower index, so in a ball query's answer (first nsample hits in index order) every copy is preceded by
// its original: the rows of the slots with index >= limit are duplicates of rows already listed and are dropped too.
__device__ __forceinline__ int pk_limit(const int *__restrict__ limit, int cloud) { return limit ? max(limit[cloud], 1) : 0x7fffffff; }

// `group` consecutive clouds share one row list (one batch of a geometry group: prcnn_ball_pack_groups): list l owns its own slice
// of the outputs and its own header; tiles record the cloud's index INSIDE its list
__device__ __forceinline__ void pk_list_slice(int list, int group, int tiles_cap_cloud, unsigned int *__restrict__ &rowinfo,
                                              float4 *__restrict__ &rowdxyz, int *__restrict__ &tilecloud, unsigned int *__restrict__ &hdr)
{
    rowinfo += (long)list * group * tiles_cap_cloud * PK_ROWS;
    rowdxyz += (long)list * group * tiles_cap_cloud * PK_ROWS;
    tilecloud += (long)list * group * tiles_cap_cloud;
    hdr += 4 * list;
}

// cnts[c] (LDS, preset to 1) <- 1 + the last slot of centre c whose point differs from slot 0's and lies below lim, for the nc centres
// of rows[nc][ns].  Parallel over ELEMENTS (T threads), 16-byte pieces of the index rows where ns allows: the centre's count is an LDS
// atomicMax over its pieces.
__device__ __forceinline__ void pk_count_pass(const int *__restrict__ rows, int nc, int ns, int lim, int *cnts, int tid, int T)
{
    if ((ns & 3) == 0) {
        const int q4 = ns >> 2;
        for (int e = tid; e < nc * q4; e += T) {
            const int c = e / q4, p = (e - c * q4) * 4;
            const int first = rows[(long)c * ns];
            const int4 v = *reinterpret_cast<const int4 *>(rows + (long)c * ns + p);
            int last = -1;
            if (v.x != first && v.x < lim) last = p;
            if (v.y != first && v.y < lim) last = p + 1;
            if (v.z != first && v.z < lim) last = p + 2;
            if (v.w != first && v.w < lim) last = p + 3;
            if (last > 0) atomicMax(&cnts[c], last + 1);
        }
    } else {
        for (int e = tid; e < nc * ns; e += T) {
            const int c = e / ns, p = e - c * ns;
            const int v = rows[e];
            if (p > 0 && v != rows[(long)c * ns] && v < lim) atomicMax(&cnts[c], p + 1);
        }
    }
}

// the last of the n entries of offs (exclusive offsets, LDS) that is <= r: the centre that owns output row r
__device__ __forceinline__ int pk_owner(const int *offs, int n, int r)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// List entry o <- slot p of centre c's index row: the descriptor and the RELATIVE coordinates xyz[point] - new_xyz[centre] (the
// subtraction the tile builders used to do -- three loads of the point + three of the centre per row -- is done once here).
// Slots beyond the limit inside the kept prefix (possible only for index rows that are not a ball query's answer) fall back to the
// row's first entry: still a copy of a listed row.
__device__ __forceinline__ void pk_write_row(const int *__restrict__ row, int p, int lim, int c, const float *__restrict__ ct,
                                             const float *__restrict__ cloud, unsigned int *__restrict__ dst, float4 *__restrict__ dxyz, long o)
{
    const int v = row[p];
    const int k = v < lim ? v : row[0];
    const float *pt = cloud + 3 * (long)k;
    dst[o] = ((unsigned int)c << 16) | (unsigned int)k;
    dxyz[o] = make_float4(pt[0] - ct[0], pt[1] - ct[1], pt[2] - ct[2], 0.f);
}

// ------------------------------------------------------------------------------------------------ one workgroup per cloud
// LDS: cnt / offset per centre (m ints) + per-thread partial sums.  Tiles are allocated from one atomic counter, so the tile count
// stays on the device.
// `rep` (optional, (b, n) i32, round 3): rep[cloud][k] = the lowest-indexed point of the cloud that is an exact copy of point k
// (coordinates AND features; k itself when it is the first of its kind) -- the SA1 centres of a RoI that were sampled from
// wrap-around copies of the same pooled point.  Same argument as for `limit`: a copy lies in a ball iff its representative
// does, and the representative has the lower index, so it is listed earlier in the same row; the slots whose point is not
// its own representative are dropped.  They may sit anywhere in a row, so with `rep` the kept slots are a 64-bit MASK per
// centre (nsample <= 64) instead of a prefix, and output row p of a centre is its p-th kept slot.
__global__ void ball_pack_kernel(int n, int m, int ns, int tiles_cap_cloud, const int *__restrict__ idx, const int *__restrict__ limit,
                                 const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                 unsigned int *__restrict__ rowinfo, float4 *__restrict__ rowdxyz, int *__restrict__ tilecloud,
                                 unsigned int *__restrict__ hdr, int group, const int *__restrict__ rep,
                                 const int *__restrict__ crep)
{
    // Both passes are parallel over ELEMENTS, not over centres (a thread per centre left 32 of 256 threads busy on the RoI
    // clouds' second level and walked each centre's rows as a chain of dependent loads: 47 us for 800 clouds x 32 centres):
    //   1. the count pass;
    //   2. block scan of the counts -> exclusive offsets;
    //   3. every thread takes OUTPUT rows: centre by binary search in the offsets, slot = row - offset.
    extern __shared__ int pk_lds[];
    int *cnts = pk_lds;                   // [m]   distinct count per centre
    int *offs = pk_lds + m;               // [m]   exclusive offsets
    int *part = pk_lds + 2 * m;           // [blockDim.x] partial sums, then their inclusive scan
    unsigned int *keep = reinterpret_cast<unsigned int *>(pk_lds + 2 * m + blockDim.x);   // [2 m] kept-slot masks (only with rep)
    __shared__ int s_base;
    const int gb = blockIdx.x, list = gb / group, b = gb - list * group, tid = threadIdx.x, T = blockDim.x;
    pk_list_slice(list, group, tiles_cap_cloud, rowinfo, rowdxyz, tilecloud, hdr);
    const int *rows = idx + (long)gb * m * ns;
    const int lim = pk_limit(limit, gb);
    const int *__restrict__ rp = rep ? rep + (long)gb * n : nullptr;
    for (int c = tid; c < m; c += T) cnts[c] = 1;
    if (rp)
        for (int c = tid; c < 2 * m; c += T) keep[c] = (c & 1) ? 0u : 1u;       // slot 0 is always kept
    __syncthreads();
    if (rp) {
        for (int e = tid; e < m * ns; e += T) {
            const int c = e / ns, p = e - c * ns;
            const int v = rows[e];
            if (p > 0 && v != rows[(long)c * ns] && v < lim && rp[v] == v) atomicOr(&keep[2 * c + (p >> 5)], 1u << (p & 31));
        }
        __syncthreads();
        for (int c = tid; c < m; c += T) cnts[c] = __popc(keep[2 * c]) + __popc(keep[2 * c + 1]);
    } else {
        pk_count_pass(rows, m, ns, lim, cnts, tid, T);
    }
    __syncthreads();
    if (crep) {
        // `crep` (optional, (b, m) i32): centre c is an exact copy of centre crep[c] <= c (same coordinates, hence the same ball and
        // the same pooled output): it gets NO rows -- its output row stays as the caller left it (zero) and nobody may read it;
        // the level above lists only representatives (its `rep` is this map)
        const int *__restrict__ cr = crep + (long)gb * m;
        for (int c = tid; c < m; c += T)
            if (cr[c] != c) cnts[c] = 0;
        __syncthreads();
    }
    const int chunk = (m + T - 1) / T;
    const int c0 = min(m, tid * chunk), c1 = min(m, c0 + chunk);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnts[c];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {     // inclusive scan of the per-thread sums (Hillis-Steele over T <= 1024 entries)
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const int total = part[T - 1];
    int run = part[tid] - sum;
    for (int c = c0; c < c1; ++c) { offs[c] = run; run += cnts[c]; }
    if (tid == 0) {
        const int ntiles = (total + PK_ROWS - 1) / PK_ROWS;
        s_base = (int)atomicAdd(&hdr[0], (unsigned int)ntiles);
        atomicAdd(&hdr[1], (unsigned int)total);
    }
    __syncthreads();
    const int base = s_base;
    const int ntiles = (total + PK_ROWS - 1) / PK_ROWS;
    for (int t = tid; t < ntiles; t += T) tilecloud[base + t] = b;
    unsigned int *dst = rowinfo + (long)base * PK_ROWS;
    float4 *dxyz = rowdxyz + (long)base * PK_ROWS;
    const float *cloud = xyz + (long)gb * n * 3;
    // rows beyond `total` fill the cloud's last tile with copies of its last row (copies do not change a max)
    for (int r = tid; r < ntiles * PK_ROWS; r += T) {
        int c = m - 1, p = 0;
        if (r < total) { c = pk_owner(offs, m, r); p = r - offs[c]; }
        if (rp) {                           // p-th kept slot of the centre: select in its 64-bit mask
            unsigned long long mm = ((unsigned long long)keep[2 * c + 1] << 32) | keep[2 * c];
            int slot = 0;
#pragma unroll
            for (int sft = 32; sft >= 1; sft >>= 1) {
                const int below = __popcll(mm & ((1ull << sft) - 1ull));
                if (p >= below) { p -= below; mm >>= sft; slot += sft; }
            }
            p = slot;
        }
        pk_write_row(rows + (long)c * ns, p, lim, c, new_xyz + ((long)gb * m + c) * 3, cloud, dst, dxyz, r);
    }
}

// ------------------------------------------------------------------------------------------------ many workgroups per cloud
// Round 6.  ball_pack_kernel is ONE workgroup per cloud: 32 workgroups for a geometry group, 142 us for the 1.2 M rows of SA1's wider
// scale on LiDAR-shaped scenes, 2.5 launches and 178 us per step there on geometry streams that are 90 % busy (profiles/
// r06_bench_step_kernel_stats_lidar.md).  The plain form (no representative map over the points) as TWO launches whose workgroups own
// PK_CH centres each: (1) counts per centre + their sum per chunk; (2) every workgroup finds its place from the chunk sums -- the
// clouds of a list in INDEX order (no atomic: the tile list is deterministic now), its chunk behind the chunks before it -- and writes
// its rows.  Same rows per cloud in the same order as ball_pack_kernel, same padding of a cloud's last tile, same header.
constexpr int PK_CH = 64;           // centres per workgroup

__global__ __launch_bounds__(256) void ball_pack_count_kernel(int m, int ns, int nchunk, const int *__restrict__ idx, const int *__restrict__ limit,
                                                              const int *__restrict__ crep, int *__restrict__ cnts, int *__restrict__ csum)
{
    __shared__ int s_cnt[PK_CH];
    const int chunk = blockIdx.x, gb = blockIdx.y, tid = threadIdx.x;
    const int c0 = chunk * PK_CH, nc = min(PK_CH, m - c0);
    if (tid < PK_CH) s_cnt[tid] = 1;
    __syncthreads();
    pk_count_pass(idx + ((long)gb * m + c0) * ns, nc, ns, pk_limit(limit, gb), s_cnt, tid, 256);
    __syncthreads();
    int v = 0;
    if (tid < nc) {
        v = s_cnt[tid];
        if (crep && crep[(long)gb * m + c0 + tid] != c0 + tid) v = 0;          // a centre that copies an earlier one gets no rows
        cnts[(long)gb * m + c0 + tid] = v;
    }
    if (tid < 64) {                                                            // PK_CH = 64: one wave holds the chunk
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (tid == 0) csum[(long)gb * nchunk + chunk] = v;
    }
}

__global__ __launch_bounds__(256) void ball_pack_write_kernel(int n, int m, int ns, int nchunk, int tiles_cap_cloud, const int *__restrict__ idx,
                                                              const int *__restrict__ limit, const float *__restrict__ xyz,
                                                              const float *__restrict__ new_xyz, const int *__restrict__ cnts,
                                                              const int *__restrict__ csum, unsigned int *__restrict__ rowinfo,
                                                              float4 *__restrict__ rowdxyz, int *__restrict__ tilecloud,
                                                              unsigned int *__restrict__ hdr, int group)
{
    __shared__ int s_off[PK_CH + 1];
    __shared__ int s_red[256];
    __shared__ int s_red2[256];
    const int chunk = blockIdx.x, gb = blockIdx.y, tid = threadIdx.x;
    const int list = gb / group, b = gb - list * group;
    pk_list_slice(list, group, tiles_cap_cloud, rowinfo, rowdxyz, tilecloud, hdr);
    const int c0 = chunk * PK_CH, nc = min(PK_CH, m - c0);
    // tiles of the list's clouds before this one (index order), rows of this cloud's chunks before this one, rows of the cloud
    const int *lsum = csum + (long)list * group * nchunk;
    int tiles_before = 0, tiles_all = 0, rows_all = 0;
    for (int j = tid; j < group; j += 256) {
        int tot = 0;
        for (int k = 0; k < nchunk; ++k) tot += lsum[(long)j * nchunk + k];
        const int tl = (tot + PK_ROWS - 1) / PK_ROWS;
        if (j < b) tiles_before += tl;
        tiles_all += tl; rows_all += tot;
    }
    int before = 0, total = 0;
    for (int k = tid; k < nchunk; k += 256) {
        const int v = lsum[(long)b * nchunk + k];
        if (k < chunk) before += v;
        total += v;
    }
    auto block_sum = [&](int v, int *buf) {
        buf[tid] = v;
        __syncthreads();
        for (int d = 128; d >= 1; d >>= 1) {
            if (tid < d) buf[tid] += buf[tid + d];
            __syncthreads();
        }
        const int r = buf[0];
        __syncthreads();
        return r;
    };
    tiles_before = block_sum(tiles_before, s_red);
    before = block_sum(before, s_red2);
    total = block_sum(total, s_red);
    if (chunk == 0 && b == 0) {                                                 // the list's header (block-uniform condition)
        tiles_all = block_sum(tiles_all, s_red2);
        rows_all = block_sum(rows_all, s_red);
        if (tid == 0) { hdr[0] = (unsigned int)tiles_all; hdr[1] = (unsigned int)rows_all; }
    }
    // exclusive offsets of this chunk's centres (one wave)
    if (tid < 64) {
        const int v = tid < nc ? cnts[(long)gb * m + c0 + tid] : 0;
        const int incl = wave_incl_scan(v, tid);
        s_off[tid] = incl - v;
        if (tid == 63) s_off[PK_CH] = incl;
    }
    __syncthreads();
    const int mine = s_off[PK_CH];                                              // rows of this chunk
    const int ntiles = (total + PK_ROWS - 1) / PK_ROWS;
    const int lim = pk_limit(limit, gb);
    const int *rows = idx + (long)gb * m * ns;
    const float *cloud = xyz + (long)gb * n * 3;
    unsigned int *dst = rowinfo + (long)tiles_before * PK_ROWS;
    float4 *dxyz = rowdxyz + (long)tiles_before * PK_ROWS;
    // the cloud's tiles that START inside this chunk's rows are recorded by this workgroup (tile 0 by the first chunk that has rows)
    for (int t = (before + PK_ROWS - 1) / PK_ROWS + tid; (long)t * PK_ROWS < (long)before + mine; t += 256) tilecloud[tiles_before + t] = b;
    // rows beyond `total` fill the cloud's last tile with copies of its LAST CENTRE's first row (as ball_pack_kernel): by the last chunk
    const int extra = (chunk == nchunk - 1) ? ntiles * PK_ROWS - total : 0;
    for (int r = tid; r < mine + extra; r += 256) {
        int c = m - 1, p = 0;
        if (r < mine) { const int lo = pk_owner(s_off, nc, r); c = c0 + lo; p = r - s_off[lo]; }
        const long o = r < mine ? (long)before + r : (long)total + (r - mine);
        pk_write_row(rows + (long)c * ns, p, lim, c, new_xyz + ((long)gb * m + c) * 3, cloud, dst, dxyz, o);
    }
}

// rep[cloud][j] = the lowest j' with src(sel[cloud][j']) == src(sel[cloud][j]), where src(i) = prev ? prev[cloud][i] : i % limit[cloud]
// (limit: the points k >= limit[cloud] are copies of k % limit[cloud]; prev: the representative map of the level below).
__global__ void dup_rep_kernel(int n, int m, const int *__restrict__ sel, const int *__restrict__ limit, const int *__restrict__ prev,
                               int *__restrict__ rep)
{
    extern __shared__ int first[];             // [n]: lowest j sampled from each source point
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    for (int i = tid; i < n; i += T) first[i] = 0x7fffffff;
    __syncthreads();
    const int lim = pk_limit(limit, b);
    const int *__restrict__ s = sel + (long)b * m;
    const int *__restrict__ pv = prev ? prev + (long)b * n : nullptr;
    for (int j = tid; j < m; j += T) {
        const int i = s[j];
        const int src = pv ? pv[i] : (i >= lim ? i % lim : i);
        atomicMin(&first[src], j);
    }
    __syncthreads();
    for (int j = tid; j < m; j += T) {
        const int i = s[j];
        const int src = pv ? pv[i] : (i >= lim ? i % lim : i);
        rep[(long)b * m + j] = first[src];
    }
}

}  // namespace prcnn

using namespace prcnn;

// limit (b) i32, optional: points k >= limit[cloud] are copies of point k % limit[cloud] (see pk_limit).
static int ball_pack_launch(int b, int group, int n, int m, int nsample, const int *idx, const int *limit, const float *xyz,
                            const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr, void *stream,
                            const int *rep = nullptr, const int *crep = nullptr, int hdr_is_zero = 0)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && m >= 0 && nsample >= 1, "ball_pack: bad sizes");
    PRCNN_REQUIRE(group >= 1 && b % group == 0, "ball_pack: %d clouds do not split into lists of %d", b, group);
    PRCNN_REQUIRE(m <= 15360, "ball_pack: m=%d centres per cloud unsupported (<= 15360)", m);
    PRCNN_REQUIRE(n <= 65536, "ball_pack: n=%d points per cloud unsupported (rowinfo keeps the point in 16 bits)", n);
    PRCNN_REQUIRE(hdr, "ball_pack: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int lists = b > 0 ? b / group : 1;
    // (round 4 tried counting in a self-resetting ticket record instead of this memset: 6323 / 6337 scenes/s against 6362 / 6402 at K = 96,
    //  6103 / 6120 with agent-scope fences around the arrival count -- the five fills per step are on nobody's critical path.  Not kept.)
    //  Round 5: the caller may hand over headers that ARE zero -- slices of an arena it zeroes once per chain of launches
    //  (prcnn_ball_pack_ex: 3.65 header fills per step -> 0.75 arena fills that also cover the levels' pooled outputs).)
    if (!hdr_is_zero && hipMemsetAsync(hdr, 0, (size_t)lists * 4 * sizeof(unsigned int), st) != hipSuccess) { set_error("ball_pack: memset failed"); return PRCNN_ELAUNCH; }
    if (b == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(idx && rowinfo && tilecloud && xyz && new_xyz && rowdxyz, "ball_pack: null pointer");
    PRCNN_REQUIRE(((uintptr_t)rowdxyz & 15) == 0, "ball_pack: rowdxyz must be 16-byte aligned");
    PRCNN_REQUIRE(((uintptr_t)idx & 15) == 0 || (nsample & 3) != 0, "ball_pack: 16-byte alignment required");
    const int cap = (int)(((long)m * nsample + PK_ROWS - 1) / PK_ROWS);
    if (!rep && m >= 512) {
        // many workgroups per cloud (round 6): counts, then rows -- see ball_pack_count_kernel
        const int nchunk = (m + PK_CH - 1) / PK_CH;
        int *scr = (int *)scratch_for(st, ((size_t)b * m + (size_t)b * nchunk) * sizeof(int), 14);
        if (!scr) { set_error("ball_pack: cannot allocate the count scratch"); return PRCNN_ELAUNCH; }
        int *cnts = scr, *csum = scr + (size_t)b * m;
        hipLaunchKernelGGL(ball_pack_count_kernel, dim3(nchunk, b), dim3(256), 0, st, m, nsample, nchunk, idx, limit, crep, cnts, csum);
        hipLaunchKernelGGL(ball_pack_write_kernel, dim3(nchunk, b), dim3(256), 0, st, n, m, nsample, nchunk, cap, idx, limit, xyz, new_xyz, cnts, csum,
                           rowinfo, (float4 *)rowdxyz, tilecloud, hdr, group);
        return check_launch("ball_pack");
    }
    int threads = 64;                              // enough threads for the cloud's index elements, 16 bytes each
    while (threads < (int)(((long)m * nsample + 3) / 4) && threads < 1024) threads *= 2;
    PRCNN_REQUIRE(!rep || nsample <= 64, "ball_pack: a representative map needs nsample <= 64 (got %d)", nsample);
    const size_t lds = ((size_t)2 * m + threads + (rep ? 2 * m : 0)) * sizeof(int);
    if (lds > 48 * 1024) {
        const int rc = ensure_dynamic_lds((const void *)ball_pack_kernel, lds, "ball_pack");
        if (rc != PRCNN_OK) return rc;
    }
    hipLaunchKernelGGL(ball_pack_kernel, dim3(b), dim3(threads), lds, st, n, m, nsample, cap, idx, limit, xyz, new_xyz, rowinfo,
                       (float4 *)rowdxyz, tilecloud, hdr, group, rep, crep);
    return check_launch("ball_pack");
}

extern "C" int prcnn_ball_pack(int b, int n, int m, int nsample, const int *idx, const int *limit, const float *xyz,
                               const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr,
                               void *stream)
{
    return ball_pack_launch(b, b > 0 ? b : 1, n, m, nsample, idx, limit, xyz, new_xyz, rowinfo, rowdxyz, tilecloud, hdr, stream);
}

// prcnn_ball_pack with representative maps (see ball_pack_kernel): rep (b, n) i32 over the POINTS, rep[cloud][k] <= k,
// rep[cloud][rep[cloud][k]] == rep[cloud][k]: the slots whose point is not its own representative are dropped as well;
// crep (b, m) i32 over the CENTRES, same properties: a centre that is not its own representative gets no rows at all.  Either may be null.
extern "C" int prcnn_ball_pack_rep(int b, int n, int m, int nsample, const int *idx, const int *limit, const int *rep, const int *crep,
                                   const float *xyz, const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud,
                                   unsigned int *hdr, void *stream)
{
    return ball_pack_launch(b, b > 0 ? b : 1, n, m, nsample, idx, limit, xyz, new_xyz, rowinfo, rowdxyz, tilecloud, hdr, stream, rep, crep);
}

// The same for b = lists x group clouds in ONE launch: list l = clouds [l group, (l + 1) group) gets its own row list
//   rowinfo / rowdxyz  [lists][group * tiles_cap * 64], tilecloud [lists][group * tiles_cap] (cloud index inside the list),
//   hdr [lists][4]
// -- the packed row lists of every batch of a geometry group (one list per batch: each batch's kernels walk their own tiles).
extern "C" int prcnn_ball_pack_groups(int b, int group, int n, int m, int nsample, const int *idx, const int *limit, const float *xyz,
                                      const float *new_xyz, unsigned int *rowinfo, float *rowdxyz, int *tilecloud, unsigned int *hdr,
                                      void *stream)
{
    return ball_pack_launch(b, group, n, m, nsample, idx, limit, xyz, new_xyz, rowinfo, rowdxyz, tilecloud, hdr, stream);
}

// Every form of the above behind one entry (round 5): group (1 list = all b clouds: pass b), limit / rep / crep optional, and
// hdr_is_zero != 0: hdr [lists][4] holds zeros already (the caller zeroes an arena of headers with ONE fill): no memset here.
extern "C" int prcnn_ball_pack_ex(int b, int group, int n, int m, int nsample, const int *idx, const int *limit, const int *rep,
                                  const int *crep, const float *xyz, const float *new_xyz, unsigned int *rowinfo, float *rowdxyz,
                                  int *tilecloud, unsigned int *hdr, int hdr_is_zero, void *stream)
{
    return ball_pack_launch(b, group > 0 ? group : (b > 0 ? b : 1), n, m, nsample, idx, limit, xyz, new_xyz, rowinfo, rowdxyz, tilecloud, hdr,
                            stream, rep, crep, hdr_is_zero);
}

/* sel (b, m) i32: indices into clouds of n points (an FPS answer).  limit (b) i32 and / or prev (b, n) i32 say which of the n
 * points are exact copies of one another; rep (b, m) i32 <- for every sampled point the first sampled point of the same source. */
extern "C" int prcnn_dup_rep(int b, int n, int m, const int *sel, const int *limit, const int *prev, int *rep, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n >= 1 && m >= 0 && n <= 12288, "dup_rep: bad sizes b=%d n=%d m=%d", b, n, m);
    if (b == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(sel && rep && (limit || prev), "dup_rep: null pointer");
    hipLaunchKernelGGL(dup_rep_kernel, dim3(b), dim3(128), (size_t)n * sizeof(int), (hipStream_t)stream, n, m, sel, limit, prev, rep);
    return check_launch("dup_rep");
}
