// scatter_plan.hip -- the order-fixed, atomic-free backward of grouping (K3), gather (K5) and three_interpolate (K9) for gfx950
// (DESIGN.md section 28).
//
// The three gradients are scatter-adds: grad_points[b][c][idx[b][s]] += term(b, c, s).  The literal ports (ball_group.hip,
// interp.hip) do one float atomicAdd per slot, so the order of a destination's sum is arrival order.  Here the index is TRANSPOSED
// once per call -- per destination k the ascending list of the slots that name it (the "scatter plan": offsets + entries) -- and the
// sums become a GATHER: lane <-> destination walks its list in that fixed order.  One plan serves every channel of a call.
//
// Plan build (not the hot path; a pure function of idx, no host read, no allocation):
//   zero, count (integer atomics: order-free), one exclusive scan per cloud, placement through an atomic cursor (the lists are then
//   complete but in arrival order), and the ordering pass: a wave owns 64 consecutive destinations, whose lists are one contiguous
//   stretch of `entries`; it takes as many whole lists as fit one LDS tile and gives every entry its rank inside its own list (the
//   slots of a list are distinct, so the ranks are a permutation); a single list longer than the tile is regenerated in order by a
//   ballot / prefix compaction of idx[s] == k over the cloud's slots (at most slots / tile such lists per cloud).
//
// Sums (the hot path): one thread per destination and up to 8 channels; a list is cut into chunks of PRCNN_SCATTER_CHUNK entries,
// each summed left to right from +0.0f, the chunk sums added left to right from +0.0f (include/prcnn_hip.h states the contract).
// Every element of grad_points is written.  While a row of grad_out fits LDS (128 KiB: every training shape of this model) a
// workgroup stages the rows of one (cloud, channel tile) there and serves all destinations from them; longer rows are gathered
// through L2, with the grid ordered so that the workgroups of one (cloud, channel tile) run on ONE XCD (workgroup w runs on XCD
// w % 8: observed placement; another one costs locality only).
#include "common.hpp"
#include <limits.h>

namespace prcnn {

constexpr int SP_TILE = 2048;     // entries of the ordering pass's LDS tile (8 KiB per one-wave workgroup)
constexpr int SP_CT = 8;          // channels per thread of the sum kernel

__global__ __launch_bounds__(256) void sp_zero_kernel(long total, int *__restrict__ cnt)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) cnt[i] = 0;
}

// cnt[b][k] = number of slots that name destination k; a value outside [0, n) is counted nowhere
__global__ __launch_bounds__(256) void sp_count_kernel(int n, int slots, const int *__restrict__ idx, int *__restrict__ cnt)
{
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const int k = idx[(long)b * slots + s];
    if ((unsigned)k < (unsigned)n) atomicAdd(cnt + (long)b * n + k, 1);
}

// offsets[b][0 .. n] = exclusive scan of cnt[b][0 .. n); cnt is left at zero: it is the placement's cursor next.  One workgroup per cloud.
__global__ __launch_bounds__(256) void sp_scan_kernel(int n, int *__restrict__ cnt, int *__restrict__ offsets)
{
    __shared__ int wsum[4];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    int *c = cnt + (long)b * n;
    int *o = offsets + (long)b * ((long)n + 1);
    int carry = 0;
    for (long base = 0; base < n; base += 1024) {
        const long k0 = base + 4 * t;
        int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = k0 + e < n ? c[k0 + e] : 0;
        const int sum = v[0] + v[1] + v[2] + v[3];
        int inc = sum;                           // wave_incl_scan (common.hpp) as text: through the call the kernel's setup is scheduled differently
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < w) before += wsum[i];
            total += wsum[i];
        }
        int ex = carry + before + inc - sum;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k0 + e < n) {
                o[k0 + e] = ex;
                c[k0 + e] = 0;
                ex += v[e];
            }
        carry += total;
        __syncthreads();
    }
    if (t == 0) o[n] = carry;
}

// every in-range slot takes the next free place of its destination's list: complete lists, arrival order
__global__ __launch_bounds__(256) void sp_place_kernel(int n, int slots, const int *__restrict__ idx, const int *__restrict__ offsets,
                                                       int *__restrict__ cursor, int *__restrict__ entries)
{
    const int b = blockIdx.y;
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= slots) return;
    const int k = idx[(long)b * slots + s];
    if ((unsigned)k >= (unsigned)n) return;
    const int pos = offsets[(long)b * ((long)n + 1) + k] + atomicAdd(cursor + (long)b * n + k, 1);
    entries[(long)b * slots + pos] = (int)s;
}

// Puts every list in ascending order.  One wave (= one workgroup) per 64 consecutive destinations of a cloud.
__global__ __launch_bounds__(64) void sp_order_kernel(int n, int slots, const int *__restrict__ idx, const int *__restrict__ offsets,
                                                      int *__restrict__ entries)
{
    __shared__ int tile[SP_TILE];
    __shared__ int offs[65];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int k0 = blockIdx.x * 64;
    const int nd = min(64, n - k0);                     // destinations of this wave
    const int *o = offsets + (long)b * ((long)n + 1) + k0;
    const int *ix = idx + (long)b * slots;
    int *ent = entries + (long)b * slots;
    offs[lane] = o[min(lane, nd)];
    if (lane == 0) offs[64] = o[nd];                    // (lanes >= nd hold o[nd] as well: their lists are empty)
    __syncthreads();
    const int mine = offs[lane + 1];                    // end of list `lane`
    int d = 0;
    while (d < nd) {                                    // d is wave-uniform
        const int start = offs[d];
        // lists d .. e-1 fit the tile together (the ends are monotonic: the lanes that pass are d, d+1, ...)
        const int e = d + __popcll(__ballot(lane >= d && lane < nd && mine - start <= SP_TILE));
        if (e == d) {
            // list d alone is longer than the tile: regenerate it in ascending order from the index itself
            const int k = k0 + d;
            int base = 0;
            for (long s0 = 0; s0 < slots; s0 += 64) {
                const long s = s0 + lane;
                const bool hit = s < slots && ix[s] == k;
                const unsigned long long m = __ballot(hit);
                if (hit) ent[start + base + __popcll(m & ((1ull << lane) - 1ull))] = (int)s;
                base += __popcll(m);
            }
            d += 1;
            continue;
        }
        const int len = offs[e] - start;
        for (int i = lane; i < len; i += 64) tile[i] = ent[start + i];
        __syncthreads();
        for (int i = lane; i < len; i += 64) {
            const int v = tile[i];
            const int dl = ix[v] - k0;                  // the list this entry belongs to (placement put it there: d <= dl < e)
            if (dl < d || dl >= e) continue;            // (cannot happen while idx is not written during the call: keeps every store inside the stretch)
            const int lo = offs[dl] - start, hi = offs[dl + 1] - start;
            int rank = 0;
            for (int j = lo; j < hi; ++j) rank += tile[j] < v ? 1 : 0;
            ent[start + lo + rank] = v;
        }
        __syncthreads();
        d = e;
    }
}

// One destination's ordered sums for up to CT channels: rows `src` (row floats each; global memory or an LDS image of it), the list
// entries[e0 .. e1).  INTERP = false: term = src[ch][s].  INTERP = true: slot s is unknown point s / 3, term = src[ch][s / 3] * w[s].
// dst[ch * n] <- the sum, for every ch < nch (an empty list: +0.0f).
template <bool INTERP, int CT>
__device__ __forceinline__ void sp_sum_list(const float *src, int row, int nch, const float *__restrict__ w, const int *__restrict__ ent,
                                            int e0, int e1, float *__restrict__ dst, int n)
{
    float tot[CT], acc[CT];
#pragma unroll
    for (int ch = 0; ch < CT; ++ch) tot[ch] = acc[ch] = 0.0f;
    int filled = 0;                                     // entries in the open chunk
    for (int e = e0; e < e1; ++e) {
        const int s = ent[e];
        const int col = INTERP ? s / 3 : s;
        const float ws = INTERP ? w[s] : 0.0f;
#pragma unroll
        for (int ch = 0; ch < CT; ++ch)
            if (ch < nch) {
                const float t = src[ch * row + col];
                acc[ch] = __fadd_rn(acc[ch], INTERP ? __fmul_rn(t, ws) : t);
            }
        if (++filled == PRCNN_SCATTER_CHUNK) {
#pragma unroll
            for (int ch = 0; ch < CT; ++ch) {
                tot[ch] = __fadd_rn(tot[ch], acc[ch]);
                acc[ch] = 0.0f;
            }
            filled = 0;
        }
    }
#pragma unroll
    for (int ch = 0; ch < CT; ++ch)
        if (ch < nch) dst[(long)ch * n] = filled ? __fadd_rn(tot[ch], acc[ch]) : tot[ch];
}

// The sums with the gathered rows in LDS (the mirror image of the forward's group_cat_lds_kernel): a workgroup stages the R rows of
// grad_out of one (cloud, channel tile) with coalesced loads -- every byte of grad_out leaves HBM once -- and serves ALL n destinations
// from them, so the data-dependent 4-byte gather is an LDS read instead of a cache line per lane.  R * row floats of dynamic LDS.
// (Measured against the kernel below, which gathers through L2: profiles/backward_ops_probe.py)
template <bool INTERP, int R>
__global__ __launch_bounds__(1024) void sp_sum_lds_kernel(int c, int n, int slots, int row, int c_total, int c0, int ctiles,
                                                          const float *__restrict__ grad_out, const float *__restrict__ weight,
                                                          const int *__restrict__ offsets, const int *__restrict__ entries,
                                                          float *__restrict__ grad_points)
{
    extern __shared__ float sp_rows[];                  // [R][row]
    const int b = blockIdx.x / ctiles, ch0 = (blockIdx.x % ctiles) * R;
    const int nch = min(R, c - ch0);
    const int t = threadIdx.x, nt = blockDim.x;
    const float *g = grad_out + ((long)b * c_total + c0 + ch0) * row;     // nch consecutive rows: one contiguous stretch
    const int total = nch * row;
    if ((((uintptr_t)g) & 15) == 0 && (total & 3) == 0) {
        const float4 *src = reinterpret_cast<const float4 *>(g);
        float4 *dst = reinterpret_cast<float4 *>(sp_rows);
        for (int i = t; i < (total >> 2); i += nt) dst[i] = src[i];
    } else {
        for (int i = t; i < total; i += nt) sp_rows[i] = g[i];
    }
    __syncthreads();
    const int *o = offsets + (long)b * ((long)n + 1);
    const int *ent = entries + (long)b * slots;
    const float *w = INTERP ? weight + (long)b * slots : nullptr;
    float *out = grad_points + ((long)b * c + ch0) * n;
    for (int k = t; k < n; k += nt) sp_sum_list<INTERP, R>(sp_rows, row, nch, w, ent, o[k], o[k + 1], out + k, n);
}

// The sums with the rows gathered through L2 (rows too long for LDS).  grid.x = 8 * ceil(rgroups / 8) * dtiles: workgroup w -> XCD
// w % 8, row group (w / 8 / dtiles) * 8 + XCD, destination tile w / 8 % dtiles: the rows a row group gathers from stay in one L2.
template <bool INTERP>
__global__ __launch_bounds__(256) void sp_sum_kernel(int c, int n, int slots, int row, int c_total, int c0, int dtiles, int rgroups,
                                                     int ctiles, const float *__restrict__ grad_out, const float *__restrict__ weight,
                                                     const int *__restrict__ offsets, const int *__restrict__ entries,
                                                     float *__restrict__ grad_points)
{
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int rg = (j / dtiles) * 8 + xcd;
    if (rg >= rgroups) return;
    const int k = (j % dtiles) * 256 + threadIdx.x;
    if (k >= n) return;
    const int b = rg / ctiles, ch0 = (rg % ctiles) * SP_CT;
    const int *o = offsets + (long)b * ((long)n + 1);
    sp_sum_list<INTERP, SP_CT>(grad_out + ((long)b * c_total + c0 + ch0) * row, row, min(SP_CT, c - ch0), INTERP ? weight + (long)b * slots : nullptr,
                               entries + (long)b * slots, o[k], o[k + 1], grad_points + ((long)b * c + ch0) * n + k, n);
}

template <bool INTERP, int R>
static int launch_sum_lds(int b, int c, int n, int slots, int row, int c_total, int c0, const float *grad_out, const float *weight,
                          const int *offsets, const int *entries, float *grad_points, hipStream_t st, const char *what)
{
    const size_t lds = (size_t)R * row * sizeof(float);
    if (lds > 64 * 1024) {
        const int rc = ensure_dynamic_lds((const void *)sp_sum_lds_kernel<INTERP, R>, lds, what);
        if (rc != PRCNN_OK) return rc;
    }
    const int ctiles = ceil_div(c, R);
    const long blocks = (long)b * ctiles;
    PRCNN_REQUIRE(blocks <= INT_MAX, "%s: %ld workgroups", what, blocks);
    // more than 32 KiB of rows (at most four such workgroups on a CU): 16 waves each to hide the gather's latency; below: 4 waves, many workgroups per CU
    const int threads = lds > 32 * 1024 ? 1024 : 256;
    hipLaunchKernelGGL((sp_sum_lds_kernel<INTERP, R>), dim3((unsigned)blocks), dim3(threads), lds, st, c, n, slots, row, c_total, c0, ctiles,
                       grad_out, weight, offsets, entries, grad_points);
    return check_launch(what);
}

template <bool INTERP>
static int launch_sum(int b, int c, int n, int slots, int row, int c_total, int c0, const float *grad_out, const float *weight,
                      const int *offsets, const int *entries, float *grad_points, hipStream_t st, const char *what)
{
    // the rows in LDS while one fits (128 KiB): 8 or 4 of them per workgroup while that keeps two workgroups on a CU (64 KiB), else 2 or 1
    const long rowb = (long)row * sizeof(float);
#define SP_LDS(R) return launch_sum_lds<INTERP, R>(b, c, n, slots, row, c_total, c0, grad_out, weight, offsets, entries, grad_points, st, what)
    if (rowb * 8 <= 64 * 1024) SP_LDS(8);
    if (rowb * 4 <= 64 * 1024) SP_LDS(4);
    if (rowb * 2 <= 128 * 1024) SP_LDS(2);              // (two rows even where they fill the CU: every row of a tile shares the reads of
    if (rowb <= 128 * 1024) SP_LDS(1);                  //  entries and weights, which is what bounds the finest interpolation)
#undef SP_LDS
    const int ctiles = ceil_div(c, SP_CT), dtiles = ceil_div(n, 256);
    const long rgroups = (long)b * ctiles;
    const long blocks = 8 * ((rgroups + 7) / 8) * dtiles;
    PRCNN_REQUIRE(blocks <= INT_MAX, "%s: %ld workgroups", what, blocks);
    PRCNN_REQUIRE((long)row * SP_CT <= INT_MAX, "%s: rows of %d floats", what, row);      // sp_sum_list indexes a channel tile with ints
    hipLaunchKernelGGL(sp_sum_kernel<INTERP>, dim3((unsigned)blocks), dim3(256), 0, st, c, n, slots, row, c_total, c0, dtiles,
                       (int)rgroups, ctiles, grad_out, weight, offsets, entries, grad_points);
    return check_launch(what);
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_scatter_plan_workspace(int b, int n, int slots)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && slots >= 0, "scatter_plan_workspace: bad sizes b=%d n=%d slots=%d", b, n, slots);
    const long words = (long)b * n;
    PRCNN_REQUIRE(words <= INT_MAX, "scatter_plan_workspace: b * n = %ld", words);
    return words > 0 ? (int)words : 1;
}

extern "C" int prcnn_scatter_plan(int b, int n, int slots, const int *idx, int *offsets, int *entries, int *work, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && slots >= 0, "scatter_plan: bad sizes b=%d n=%d slots=%d", b, n, slots);
    PRCNN_REQUIRE(b <= 65535 && (long)b * n <= INT_MAX, "scatter_plan: b=%d n=%d too large", b, n);
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(offsets && (slots == 0 || (idx && entries)) && (n == 0 || work), "scatter_plan: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const bool any = n > 0 && slots > 0;
    const dim3 per_slot(ceil_div(slots, 256), b);
    if (n > 0) {
        const long total = (long)b * n;
        hipLaunchKernelGGL(sp_zero_kernel, dim3((unsigned)(total > 4096L * 256 ? 4096L : (total + 255) / 256)), dim3(256), 0, st, total, work);
    }
    if (any) hipLaunchKernelGGL(sp_count_kernel, per_slot, dim3(256), 0, st, n, slots, idx, work);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(b), dim3(256), 0, st, n, work, offsets);
    if (any) {
        hipLaunchKernelGGL(sp_place_kernel, per_slot, dim3(256), 0, st, n, slots, idx, offsets, work, entries);
        hipLaunchKernelGGL(sp_order_kernel, dim3(ceil_div(n, 64), b), dim3(64), 0, st, n, slots, idx, offsets, entries);
    }
    return check_launch("scatter_plan");
}

extern "C" int prcnn_group_points_grad_ordered(int b, int c, int n, int slots, int c_total, int c0, const float *grad_out,
                                               const int *offsets, const int *entries, float *grad_points, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && c >= 0 && n >= 0 && slots >= 0 && c0 >= 0 && c_total >= 0 && (long)c0 + c <= c_total,
                  "group_points_grad_ordered: bad sizes b=%d c=%d n=%d slots=%d c_total=%d c0=%d", b, c, n, slots, c_total, c0);
    if (b == 0 || c == 0 || n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(offsets && grad_points && (slots == 0 || (grad_out && entries)), "group_points_grad_ordered: null pointer");
    return launch_sum<false>(b, c, n, slots, slots, c_total, c0, grad_out, nullptr, offsets, entries, grad_points, (hipStream_t)stream,
                             "group_points_grad_ordered");
}

extern "C" int prcnn_three_interpolate_grad_ordered(int b, int c, int n, int m, const float *grad_out, const float *weight,
                                                    const int *offsets, const int *entries, float *grad_points, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && c >= 0 && n >= 0 && m >= 0 && (long)n * 3 <= INT_MAX, "three_interpolate_grad_ordered: bad sizes b=%d c=%d n=%d m=%d",
                  b, c, n, m);
    if (b == 0 || c == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(offsets && grad_points && (n == 0 || (grad_out && weight && entries)), "three_interpolate_grad_ordered: null pointer");
    return launch_sum<true>(b, c, m, 3 * n, n, c, 0, grad_out, weight, offsets, entries, grad_points, (hipStream_t)stream,
                            "three_interpolate_grad_ordered");
}
