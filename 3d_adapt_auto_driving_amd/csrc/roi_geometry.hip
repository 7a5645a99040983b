// roi_geometry.hip -- sampling, ball query, representative maps and row lists of the RCNN's RoI clouds, a wave per RoI.
#include "fps_common.hpp"

// ---- the whole geometry chain of the RCNN's RoI clouds in ONE kernel (round 3) -----------------------------------------------
// rcnn_net.py:165-175 runs, per RoI, SA level 1 (sample 128 of the 512 pooled points, ball query r1 / 64) and SA level 2 (sample 32 of
// those 128, ball query r2 / 64).  As separate launches over the 800 RoI clouds of a batch that was FPS, limited ball query,
// representative map, FPS, ball query, representative map: six latency-bound kernels (one wave per cloud each, ~0.8 us per dependent
// FPS iteration) that were 0.41 ms of the proposal stream in the pipelined step and a quarter of a millisecond of host time.
// Here ONE WAVE serves a RoI from the pooled coordinates to both index tensors: the cloud stays in registers (8 points per lane)
// through sampling and the first ball query, the 128 sampled centres stay in registers (2 per lane) through the second pair; the hit
// lists are staged in LDS ([slot][centre]) and leave as coalesced rows.  Per operator the arithmetic is that of fps_reg_kernel /
// ball_query_kernel / dup_rep_kernel: same indices, bit for bit (tests/test_gpu_ops.py compares with the separate entry points,
// tests/test_gpu_shadow.py with the oracle).
namespace prcnn {

constexpr int RG_N = 512, RG_M1 = 128, RG_M2 = 32, RG_NS = 64;
constexpr int RG_LD1 = RG_M1 + 1, RG_LD2 = RG_M2 + 1;   // row strides of the staged hit lists (16-bit entries): odd, see the rows-out loops

// coordinates of point (lane l, slot) -- both wave-uniform, slot < D -- of the D first register slots: a scalar compare ladder in front
// of three v_readlane (fs_pick3 over a prefix of the arrays)
template <int PPT, int D, int I = 0>
__device__ __forceinline__ void roi_pick3(const float (&px)[PPT], const float (&py)[PPT], const float (&pz)[PPT], int slot, int l,
                                          float &x, float &y, float &z)
{
    if (I + 1 == D || slot == I) {
        x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px[I]), l));
        y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py[I]), l));
        z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[I]), l));
    } else if constexpr (I + 1 < D) {
        roi_pick3<PPT, D, I + 1>(px, py, pz, slot, l, x, y, z);
    }
}

// FPS of a cloud of n <= 64 PPT points held in registers (point k = lane + 64 i) -> sel[0..m) in LDS; all lanes in step.  Returns the
// number of picks made before only copies of picked points were left (m if that never happened): sel[that ..] = 0.
//
// Only the first `lim` points are distinct: D = ceil(lim / 64) register slots take part instead of PPT (round 5; a pooled RoI cloud has
// 20-80 distinct points of its 512 on the synthetic scenes, and a pick was ~130 VALU instructions of a single-wave dependent chain).
//   MOD = true:  point k >= lim is a copy of point k % lim (the pooled rows).  A copy has its source's coordinates, hence its source's
//     running minimum at every step, and the scan's pick is the arg-max with the smallest tie key: it is decided among the SOURCES when
//     each carries the smallest key of its copies; the index handed back is that copy's, as in the scan over all n.
//   MOD = false: the points k >= lim are all copies of point 0 (the sampled centres behind an exhausted level-1 scan).  Point 0 is the
//     first pivot: its minimum is 0 from the first step on and its key never decides a pick before the exit below.
// The exit: a best value of exactly 0 means only copies of picked points are left -- every later pick is point 0 (fps_reg_kernel).
template <int PPT, int D, bool MOD>
__device__ __forceinline__ int roi_fps(int n, int lim, int m, KeyCodec kc, const float (&px)[PPT], const float (&py)[PPT],
                                       const float (&pz)[PPT], int *__restrict__ s_sel, const int lane)
{
    float pt[D];
    uint32_t pk[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const int k = lane + 64 * i;
        pt[i] = k < lim ? 1e10f : -INFINITY;
        uint32_t key = 0xffffffffu;
        if (k < lim) {
            key = kc.encode(k);
            if (MOD)
                for (int c = k + lim; c < n; c += lim) {
                    const uint32_t kc2 = kc.encode(c);
                    key = kc2 < key ? kc2 : key;
                }
        }
        pk[i] = key;
    }
    if (lane == 0) s_sel[0] = 0;
    float ox = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px[0]), 0));
    float oy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py[0]), 0));
    float oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[0]), 0));
    for (int j = 1; j < m; ++j) {
        float lv = -INFINITY;
        if constexpr (D >= 2) {
            // slot PAIRS on packed f32 arithmetic (each half the scalar form's operations, one rounding each: same bits; see fps_spec_kernel)
            const pk_f32x2 o_x = {ox, ox}, o_y = {oy, oy}, o_z = {oz, oz};
#pragma unroll
            for (int i = 0; i < D; i += 2) {
                const pk_f32x2 dx = (pk_f32x2){px[i], px[i + 1]} - o_x, dy = (pk_f32x2){py[i], py[i + 1]} - o_y, dz = (pk_f32x2){pz[i], pz[i + 1]} - o_z;
                const pk_f32x2 d = kc.hipcc ? (pk_f32x2)(__builtin_elementwise_fma(dy, dy, dx * dx) + dz * dz) : (pk_f32x2)((dx * dx + dy * dy) + dz * dz);
                pt[i] = fmin_raw(d.x, pt[i]); pt[i + 1] = fmin_raw(d.y, pt[i + 1]);
                lv = fmax_raw(lv, fmax_raw(pt[i], pt[i + 1]));
            }
        } else {
            const float d = kc.hipcc ? fps_dist<true>(px[0], py[0], pz[0], ox, oy, oz) : sqdist3(px[0], py[0], pz[0], ox, oy, oz);
            pt[0] = fmin_raw(d, pt[0]);
            lv = pt[0];
        }
        const float bv = wave_max_f32(lv);
        uint32_t lk = 0xffffffffu;                               // this lane's smallest key among its slots at the best value, and its slot
        int ls = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const bool take = pt[i] == bv && pk[i] < lk;
            lk = take ? pk[i] : lk;
            ls = take ? i : ls;
        }
        // one lane at the best value (the rule once the points are distinct): its key is the answer, no second reduction
        const unsigned long long at = __ballot(lv == bv);
        uint32_t bkey;
        int wl;
        if (__builtin_popcountll(at) == 1) {
            wl = (int)__builtin_ctzll(at);
            bkey = (uint32_t)__builtin_amdgcn_readlane((int)lk, wl);
        } else {
            bkey = wave_min_u32(lk);
            const unsigned long long wm = __ballot(lk == bkey);
            wl = wm ? (int)__builtin_ctzll(wm) : 0;
        }
        const bool valid = !(bkey == 0xffffffffu || !(bv > -1.0f));
        int old = valid ? kc.decode(bkey) : 0;
        old = __builtin_amdgcn_readfirstlane(old);
        if (lane == 0) s_sel[j] = old;
        if (bv == 0.f) {
            for (int jj = j + 1 + lane; jj < m; jj += 64) s_sel[jj] = 0;
            return j;
        }
        // the next pivot: the winner's source sits in slot `ls` of lane `wl` (point 0 behind an invalid best)
        wl = valid ? wl : 0;
        const int slot = valid ? __builtin_amdgcn_readlane(ls, wl) : 0;
        roi_pick3<PPT, D>(px, py, pz, slot, wl, ox, oy, oz);
    }
    return m;
}

template <int PPT, bool MOD>
__device__ __forceinline__ int roi_fps_any(int n, int lim, int m, KeyCodec kc, const float (&px)[PPT], const float (&py)[PPT],
                                           const float (&pz)[PPT], int *__restrict__ s_sel, const int lane)
{
    static_assert(PPT == 8 || PPT == 2, "the two shapes of the RoI chain");
    if constexpr (PPT == 8) {
        if (lim > 256) return roi_fps<PPT, 8, MOD>(n, lim, m, kc, px, py, pz, s_sel, lane);
        if (lim > 128) return roi_fps<PPT, 4, MOD>(n, lim, m, kc, px, py, pz, s_sel, lane);
    }
    if (lim > 64) return roi_fps<PPT, 2, MOD>(n, lim, m, kc, px, py, pz, s_sel, lane);
    return roi_fps<PPT, 1, MOD>(n, lim, m, kc, px, py, pz, s_sel, lane);
}

// first `ns` in-range points (k < n_scan, index order) of CPL centres per lane among the PPT * 64 points in registers -> hit lists in
// LDS, s_hits[slot * stride + centre], counts in cnt[] (returned in registers); lanes whose centres are all full stop the scan early together.
// MASK: um[i] bit l <- point 64 i + l was staged by some live centre (the point of a scan step is wave-uniform: a ballot per step)
template <int PPT, int CPL, bool MASK>
__device__ __forceinline__ void roi_ball_query_any(int n_scan, int ns, float r2, const float (&px)[PPT], const float (&py)[PPT],
                                                   const float (&pz)[PPT], const float (&cx)[CPL], const float (&cy)[CPL], const float (&cz)[CPL],
                                                   const bool (&live)[CPL], unsigned short *__restrict__ s_hits, int stride, int (&cnt)[CPL],
                                                   unsigned long long (&um)[PPT], const int lane)
{
#pragma unroll
    for (int q = 0; q < CPL; ++q) cnt[q] = live[q] ? 0 : ns;
    if constexpr (MASK) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) um[i] = 0ull;
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int base = 64 * i;
        if (base >= n_scan) break;
        bool full = true;
#pragma unroll
        for (int q = 0; q < CPL; ++q) full = full && cnt[q] >= ns;
        if (__all(full)) break;
        const int nb = min(64, n_scan - base);
        for (int l = 0; l < nb; ++l) {
            const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px[i]), l));
            const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py[i]), l));
            const float z = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[i]), l));
            bool staged = false;
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const float d2 = sqdist3(cx[q], cy[q], cz[q], x, y, z);
                if (d2 < r2 && cnt[q] < ns) {
                    s_hits[cnt[q] * stride + lane + 64 * q] = (unsigned short)(base + l);
                    ++cnt[q];
                    staged = true;
                }
            }
            if constexpr (MASK)
                if (__any(staged)) um[i] |= 1ull << l;
        }
    }
}

template <int PPT, int CPL>
__device__ __forceinline__ void roi_ball_query(int n_scan, int ns, float r2, const float (&px)[PPT], const float (&py)[PPT],
                                               const float (&pz)[PPT], const float (&cx)[CPL], const float (&cy)[CPL], const float (&cz)[CPL],
                                               const bool (&live)[CPL], unsigned short *__restrict__ s_hits, int stride, int (&cnt)[CPL],
                                               const int lane)
{
    unsigned long long none[PPT];
    roi_ball_query_any<PPT, CPL, false>(n_scan, ns, r2, px, py, pz, cx, cy, cz, live, s_hits, stride, cnt, none, lane);
}

// rows of an index tensor out of the staged hit lists: slot s of centre c; slots past the hit count repeat the first hit, an empty ball is
// a row of zeros.  The lists sit in LDS as [slot][centre] with an ODD row stride: the ball query writes a slot of 64 centres side by
// side, this loop reads the 64 slots of one centre -- 64 consecutive rows -- and with an even stride (128 entries = 256 bytes) those
// were 64 addresses in ONE bank: 300 cycles per row, a fifth of the kernel.  cnt_lo / cnt_hi: the hit counts of centres lane / lane + 64.
template <int M>
__device__ __forceinline__ void roi_rows_out(int ns, const unsigned short *__restrict__ s_hits, int stride, int cnt_lo, int cnt_hi,
                                             int *__restrict__ out, const int lane)
{
    if (ns == 64) {                                               // a row per wave store: centre c = the iteration, slot = the lane
#pragma unroll 8
        for (int c = 0; c < M; ++c) {
            const int tot = __builtin_amdgcn_readlane(c < 64 ? cnt_lo : cnt_hi, c & 63);
            const int v = s_hits[(lane < tot ? lane : 0) * stride + c];
            out[c * 64 + lane] = tot == 0 ? 0 : v;
        }
    } else {
        for (int e = lane; e < M * ns; e += 64) {
            const int c = e / ns, s = e - c * ns;
            const int t_lo = __shfl(cnt_lo, c & 63, 64), t_hi = __shfl(cnt_hi, c & 63, 64);
            const int tot = c < 64 ? t_lo : t_hi;
            out[e] = tot == 0 ? 0 : (int)s_hits[(s < tot ? s : 0) * stride + c];
        }
    }
}

// The row lists of the two sampled levels (prcnn_rcnn_roi_geometry_packs): what prcnn_ball_pack_ex makes of idx1 (limit, crep = rep1)
// and of idx2 (rep = rep1, crep = rep2), written by the wave that has the hit lists in LDS anyway -- as separate launches the two
// packs re-derived them from 10240 index entries per cloud (1024-thread workgroups, a block scan, a binary search per row) and cost
// the step 26 us (uniform scene) / 57 us (LiDAR-shaped) of 1060 / 1540 (profiles/sensitivity_probe.py).  hdr: zero on entry.
struct RgPacks {
    unsigned int *rowinfo1; float4 *rowdxyz1; int *tilecloud1; unsigned int *hdr1;
    unsigned int *rowinfo2; float4 *rowdxyz2; int *tilecloud2; unsigned int *hdr2;
    unsigned int *rowinfo3; float4 *rowdxyz3; unsigned int *hdr3;    // optional third list (rows carry their cloud): see the kernel's end
    int *crows1; unsigned int *hdr_c1;                               // optional: the level-1 centres that are their own representatives, as rows
    // tilecloud* == NULL: the lists' rows carry their cloud -- descriptor (cloud << 16) | (centre << 9) | point -- and are drawn from the
    // list's ROW counter hdr[1], so that tiles are cut wherever the rows fall (csrc/sa_packed.hip reads such a list when it is given no
    // tilecloud): no padded last tile per cloud
};

// One cloud's list: centre c (c = lane: keep_lo / tot_lo, c = lane + 64: keep_hi / tot_hi; M centres) lists keep[c] rows -- 0 for a
// centre that copies an earlier one, else max(hits, 1) -- row p of it = hit p of its staged list (point 0 of an empty ball), in centre
// order, cut into 64-row tiles drawn from the list's counter; the last tile is filled with copies of centre M - 1's first row (as
// ball_pack_kernel fills it).  pmap: staged hit -> point of the cloud (null: itself); cmap_*: centre -> point of the cloud.
// PAD_LAST (the live-rows form, where centre M - 1 may list nothing): the last tile is filled with copies of the list's last ROW instead.
template <int M, bool PAD_LAST = false>
__device__ __forceinline__ void roi_pack_out(int b, int keep_lo, int keep_hi, int tot_lo, int tot_hi, const unsigned short *__restrict__ s_hits,
                                             int stride, int *__restrict__ s_off, const float *__restrict__ cloud,
                                             const int *__restrict__ pmap, const int *__restrict__ cmap, const int *__restrict__ cmap2,
                                             unsigned int *__restrict__ rowinfo, float4 *__restrict__ rowdxyz, int *__restrict__ tilecloud,
                                             unsigned int *__restrict__ hdr, const int lane)
{
    const int in_lo = wave_incl_scan(keep_lo, lane);
    const int sum_lo = __builtin_amdgcn_readlane(in_lo, 63);
    const int in_hi = wave_incl_scan(M > 64 ? keep_hi : 0, lane) + sum_lo;
    const int total = __builtin_amdgcn_readlane(in_hi, 63);
    if (lane < M) s_off[lane] = in_lo - keep_lo;
    if (M > 64) s_off[lane + 64] = in_hi - keep_hi;
    const bool rowcloud = tilecloud == nullptr;
    const int nt = (total + 63) >> 6;
    int base = 0;
    if (lane == 0) {
        if (rowcloud) {
            base = (int)atomicAdd(&hdr[1], (unsigned int)total);  // the cloud's first ROW of the list
        } else {
            base = (int)atomicAdd(&hdr[0], (unsigned int)nt);     // the cloud's first TILE
            atomicAdd(&hdr[1], (unsigned int)total);
        }
    }
    base = __builtin_amdgcn_readfirstlane(base);
    __syncthreads();                                              // (one wave: orders the LDS writes above before the searches below)
    if (!rowcloud)
        for (int t = lane; t < nt; t += 64) tilecloud[base + t] = b;
    unsigned int *__restrict__ dst = rowinfo + (rowcloud ? (long)base : (long)base * 64);
    float4 *__restrict__ dx = rowdxyz + (rowcloud ? (long)base : (long)base * 64);
    const int rows_out = rowcloud ? total : nt * 64;
    for (int r0 = 0; r0 < rows_out; r0 += 64) {
        const int r = r0 + lane;                                  // (every lane stays in the loop: the shuffles below read all of them)
        int c = M - 1, p = 0;
        const int rl = PAD_LAST ? min(r, total - 1) : r;          // the listed row this one is (a copy of)
        if (rl >= 0 && rl < total) {
            int lo = 0, hi = M - 1;                               // the last centre whose offset is <= rl
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_off[mid] <= rl) lo = mid; else hi = mid - 1;
            }
            c = lo; p = rl - s_off[lo];
        }
        const int t_lo = __shfl(tot_lo, c & 63, 64), t_hi = __shfl(tot_hi, c & 63, 64);
        const int tot = (M > 64 && c >= 64) ? t_hi : t_lo;
        const int k = tot == 0 ? 0 : (int)s_hits[p * stride + c];
        const int pi = pmap ? pmap[k] : k;
        const int ci = cmap2 ? cmap[cmap2[c]] : cmap[c];
        const float *__restrict__ pt = cloud + 3 * pi, *__restrict__ ct = cloud + 3 * ci;
        if (r < rows_out) {
            dst[r] = rowcloud ? (((unsigned int)b << 16) | ((unsigned int)c << 9) | (unsigned int)k) : (((unsigned int)c << 16) | (unsigned int)k);
            dx[r] = make_float4(pt[0] - ct[0], pt[1] - ct[1], pt[2] - ct[2], 0.f);
        }
    }
}

// LIVE (prcnn_rcnn_roi_geometry_live): level 2 runs FIRST -- its sampling and ball query need the 128 centres only -- and says which
// level-1 centres a row of its list names; level 1's ball query, list and centre rows then cover those centres alone, and used0 gets the
// pooled points that the kept level-1 rows name.  Both levels' hit lists take turns in s_hits: the same LDS as the other order.
template <bool LIVE>
__global__ __launch_bounds__(64) void rcnn_roi_geometry_kernel(
    KeyCodec kc1, KeyCodec kc2, float r1sq, float r2sq, int ns1, int ns2, const float *__restrict__ xyz /* (b, 512, 3) */,
    const int *__restrict__ limit /* (b) */, float *__restrict__ new_xyz1 /* (b,128,3) */, int *__restrict__ idx1 /* (b,128,ns1) */,
    int *__restrict__ rep1 /* (b,128) */, float *__restrict__ new_xyz2 /* (b,32,3) */, int *__restrict__ idx2 /* (b,32,ns2) */,
    int *__restrict__ rep2 /* (b,32) */, const RgPacks pk /* .rowinfo1 == NULL: no row lists */, unsigned int *__restrict__ used0 /* LIVE: (b,16) */)
{
    // hit lists of the running ball query, [slot][centre], as 16-bit point numbers (< 512): 16.5 KB.  With 32-bit entries the workgroup
    // held 36 KB of LDS -- FOUR single-wave workgroups per CU, one per SIMD, and 1600 RoI clouds took two rounds of a chain that is
    // latency-bound from end to end (250 us per 1600 clouds); at 21 KB seven fit and every cloud of a launch is resident at once
    __shared__ unsigned short s_hits[RG_NS * RG_LD1];
    __shared__ int s_sel1[RG_M1], s_sel2[RG_M2];
    __shared__ int s_first[RG_N];
    __shared__ int s_rep1[RG_M1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *__restrict__ cloud = xyz + (long)b * RG_N * 3;
    const int lim = limit ? min(max(limit[b], 1), RG_N) : RG_N;
    __builtin_amdgcn_s_setprio(3);

    // ---- level 1: sample 128 of the 512 pooled points
    float px[8], py[8], pz[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = lane + 64 * i;
        px[i] = cloud[3 * k]; py[i] = cloud[3 * k + 1]; pz[i] = cloud[3 * k + 2];
    }
    const int nd1 = roi_fps_any<8, true>(RG_N, lim, RG_M1, kc1, px, py, pz, s_sel1, lane);
    __syncthreads();
    // the centres that are their own representatives are the first nd1 (distinct picks; what follows are copies of centre 0): listed as
    // rows b * 128 + c for the per-point layer of the level above (prcnn_rows_gemm128_rows), which nobody asks for the other rows
    if (!LIVE && pk.crows1) {
        int base = 0;
        if (lane == 0) base = (int)atomicAdd(&pk.hdr_c1[1], (unsigned int)nd1);
        base = __builtin_amdgcn_readfirstlane(base);
        for (int c = lane; c < nd1; c += 64) pk.crows1[base + c] = b * RG_M1 + c;
    }
    // the sampled centres: coordinates into registers (centre c = lane + 64 q) and out to new_xyz1
    float qx[2], qy[2], qz[2];
    int src1[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = lane + 64 * q, k = s_sel1[c];
        qx[q] = cloud[3 * k]; qy[q] = cloud[3 * k + 1]; qz[q] = cloud[3 * k + 2];
        float *o = new_xyz1 + ((long)b * RG_M1 + c) * 3;
        o[0] = qx[q]; o[1] = qy[q]; o[2] = qz[q];
        src1[q] = k >= lim ? k % lim : k;                        // the distinct pooled point behind this centre
    }
    // ---- ball query of level 1 over the DISTINCT pooled points only (prcnn_ball_query_limit)
    int cnt1[2];
    if constexpr (!LIVE) {
        const bool live[2] = {true, true};
        roi_ball_query<8, 2>(lim, ns1, r1sq, px, py, pz, qx, qy, qz, live, s_hits, RG_LD1, cnt1, lane);
    }
    // representative map of the centres: the first centre sampled from the same source (prcnn_dup_rep)
#pragma unroll
    for (int i = 0; i < 8; ++i) s_first[lane + 64 * i] = 0x7fffffff;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) atomicMin(&s_first[src1[q]], lane + 64 * q);
    __syncthreads();
    int own1[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = s_first[src1[q]];
        s_rep1[lane + 64 * q] = r;
        rep1[(long)b * RG_M1 + lane + 64 * q] = r;
        own1[q] = r == lane + 64 * q;
    }
    if constexpr (!LIVE) {
        if (idx1) roi_rows_out<RG_M1>(ns1, s_hits, RG_LD1, cnt1[0], cnt1[1], idx1 + (long)b * RG_M1 * ns1, lane);
        if (pk.rowinfo1) {
            __syncthreads();                                      // s_first is free: the list's offsets
            roi_pack_out<RG_M1>(b, own1[0] ? max(cnt1[0], 1) : 0, own1[1] ? max(cnt1[1], 1) : 0, cnt1[0], cnt1[1], s_hits, RG_LD1, s_first, cloud,
                                nullptr, s_sel1, nullptr, pk.rowinfo1, pk.rowdxyz1, pk.tilecloud1, pk.hdr1, lane);
        }
    }
    __syncthreads();                                              // s_hits is reused below

    // ---- level 2: sample 32 of the 128 centres (held in registers as points k = lane + 64 q), ball query over all 128.
    // Behind an exhausted level-1 scan (nd1 < 128 picks, then copies of point 0) only the first nd1 centres are distinct.
    roi_fps_any<2, false>(RG_M1, nd1, RG_M2, kc2, qx, qy, qz, s_sel2, lane);
    __syncthreads();
    float cx[1] = {0.f}, cy[1] = {0.f}, cz[1] = {0.f};
    const bool has = lane < RG_M2;
    const int src2 = has ? s_rep1[s_sel2[lane]] : 0;            // the first level-1 centre with the same source as this one's pick
    // centre coordinates of level 2 by a cross-lane read of the registers that hold the 128 points
    {
        const int k = has ? s_sel2[lane] : 0;
        const int ql = k & 63, qi = k >> 6;
        const float x0 = __shfl(qx[0], ql), x1 = __shfl(qx[1], ql);
        const float y0 = __shfl(qy[0], ql), y1 = __shfl(qy[1], ql);
        const float z0 = __shfl(qz[0], ql), z1 = __shfl(qz[1], ql);
        cx[0] = qi ? x1 : x0; cy[0] = qi ? y1 : y0; cz[0] = qi ? z1 : z0;
        if (has) {
            float *o = new_xyz2 + ((long)b * RG_M2 + lane) * 3;
            o[0] = cx[0]; o[1] = cy[0]; o[2] = cz[0];
        }
    }
    // representative map of level 2's centres through the map of level 1
    for (int i = lane; i < RG_M1; i += 64) s_first[i] = 0x7fffffff;
    __syncthreads();
    if (has) atomicMin(&s_first[src2], lane);
    __syncthreads();
    const int r2own = has ? s_first[src2] : -1;
    if (has) rep2[(long)b * RG_M2 + lane] = r2own;
    int cnt2[1], cntd2 = 0;
    unsigned long long um1[2];                                    // LIVE: the level-1 centres (k = 64 i + bit) that a row of level 2's list names
    {
        // the scan runs over the nd1 distinct centres; the centres behind them are copies of centre 0: in range together with it, and
        // then the next hits in index order.  LIVE: no index tensor is written, only the centres that list rows are scanned for, and
        // every hit staged for one of them is a row of the list (they are among the distinct centres)
        const bool live[1] = {LIVE ? r2own == lane : has};
        roi_ball_query_any<2, 1, LIVE>(nd1, ns2, r2sq, qx, qy, qz, cx, cy, cz, live, s_hits, RG_LD2, cnt2, um1, lane);
        cntd2 = live[0] ? cnt2[0] : 0;                            // hits among the distinct centres: the rows the level's list keeps
        if constexpr (LIVE) {
            if (__any(live[0] && cntd2 == 0)) um1[0] |= 1ull;     // point 0 of an empty ball
        } else {
            const float x0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qx[0]), 0));
            const float y0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qy[0]), 0));
            const float z0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qz[0]), 0));
            if (has && sqdist3(cx[0], cy[0], cz[0], x0, y0, z0) < r2sq)
                for (int k = nd1; k < RG_M1 && cnt2[0] < ns2; ++k) {
                    s_hits[cnt2[0] * RG_LD2 + lane] = (unsigned short)k;
                    ++cnt2[0];
                }
        }
    }
    if constexpr (!LIVE) {
        if (idx2) roi_rows_out<RG_M2>(ns2, s_hits, RG_LD2, has ? cnt2[0] : 0, 0, idx2 + (long)b * RG_M2 * ns2, lane);
    }
    if (pk.rowinfo1) {
        __syncthreads();
        roi_pack_out<RG_M2>(b, r2own == lane ? max(cntd2, 1) : 0, 0, cntd2, 0, s_hits, RG_LD2, s_first, cloud, s_sel1, s_sel1, s_sel2,
                            pk.rowinfo2, pk.rowdxyz2, pk.tilecloud2, pk.hdr2, lane);
    }
    // the list of the level ABOVE (rcnn_net.py's GroupAll module: one group of all 32 centres, no centre subtraction): a row per centre of
    // level 2 that is its own representative -- what prcnn_ball_pack_ex makes of the index rows 0 .. 31 around the origin with rep = rep2,
    // every cloud a list of its own centre 0
    if (pk.rowinfo3) {
        const unsigned long long own = __ballot(has && r2own == lane);
        const int n3 = __builtin_popcountll(own);
        int base = 0;
        if (lane == 0) base = (int)atomicAdd(&pk.hdr3[1], (unsigned int)n3);
        base = __builtin_amdgcn_readfirstlane(base);
        if (has && r2own == lane) {
            const int r = base + (int)__builtin_popcountll(own & ((1ull << lane) - 1ull));
            pk.rowinfo3[r] = ((unsigned int)b << 16) | (unsigned int)lane;
            pk.rowdxyz3[r] = make_float4(cx[0] - 0.f, cy[0] - 0.f, cz[0] - 0.f, 0.f);
        }
    }
    if constexpr (LIVE) {
        // ---- level 1 over the centres that level 2 reads (all of them among the nd1 that are their own representatives; centre 0 is
        // always one: level 2 samples it first and its ball holds it)
        __syncthreads();                                          // s_hits and s_first are free again
        bool use1[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) use1[q] = own1[q] && ((um1[q] >> lane) & 1ull);
        if (pk.crows1) {                                          // ... as rows for level 2's per-point layer, in centre order
            const unsigned long long u_lo = __ballot(use1[0]), u_hi = __ballot(use1[1]);
            const int n_lo = __builtin_popcountll(u_lo);
            int base = 0;
            if (lane == 0) base = (int)atomicAdd(&pk.hdr_c1[1], (unsigned int)(n_lo + __builtin_popcountll(u_hi)));
            base = __builtin_amdgcn_readfirstlane(base);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (use1[0]) pk.crows1[base + (int)__builtin_popcountll(u_lo & below)] = b * RG_M1 + lane;
            if (use1[1]) pk.crows1[base + n_lo + (int)__builtin_popcountll(u_hi & below)] = b * RG_M1 + 64 + lane;
        }
        unsigned long long um0[8];                                // the pooled points that a kept row of level 1's list names
        roi_ball_query_any<8, 2, true>(lim, ns1, r1sq, px, py, pz, qx, qy, qz, use1, s_hits, RG_LD1, cnt1, um0, lane);
#pragma unroll
        for (int q = 0; q < 2; ++q) cnt1[q] = use1[q] ? cnt1[q] : 0;
        if (__any((use1[0] && cnt1[0] == 0) || (use1[1] && cnt1[1] == 0))) um0[0] |= 1ull;   // point 0 of an empty ball
        if (used0) {
            unsigned int w = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                w = lane == 2 * i ? (unsigned int)um0[i] : w;
                w = lane == 2 * i + 1 ? (unsigned int)(um0[i] >> 32) : w;
            }
            if (lane < RG_N / 32) used0[(long)b * (RG_N / 32) + lane] = w;
        }
        if (pk.rowinfo1) {
            __syncthreads();
            roi_pack_out<RG_M1, true>(b, use1[0] ? max(cnt1[0], 1) : 0, use1[1] ? max(cnt1[1], 1) : 0, cnt1[0], cnt1[1], s_hits, RG_LD1, s_first,
                                      cloud, nullptr, s_sel1, nullptr, pk.rowinfo1, pk.rowdxyz1, pk.tilecloud1, pk.hdr1, lane);
        }
    }
}

}  // namespace prcnn

using namespace prcnn;

/* RoI clouds xyz (b,512,3) whose points k >= limit[cloud] are copies of point k % limit[cloud] (pooled RoI rows) ->
 *   new_xyz1 (b,128,3), idx1 (b,128,ns1), rep1 (b,128): furthest_point_sample(128) + ball_query(r1, ns1) over the distinct points
 *                                                        (= prcnn_fps_new_xyz, prcnn_ball_query_limit, prcnn_dup_rep with `limit`);
 *   new_xyz2 (b,32,3), idx2 (b,32,ns2), rep2 (b,32): the same one level up over the 128 centres (prcnn_fps_new_xyz, prcnn_ball_query
 *                                                      with empty balls written as zeros, prcnn_dup_rep with prev = rep1).
 * ns1, ns2 <= 64.  The shape of rcnn_net.py:165-175 under default.yaml (RCNN.NUM_POINTS 512, SA_CONFIG NPOINTS [128, 32, -1]). */
static int roi_geometry_any(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                            const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                            const prcnn::RgPacks *packs, void *stream, unsigned int *used0 = nullptr, bool live = false)
{
    PRCNN_REQUIRE(b >= 0 && n == RG_N && m1 == RG_M1 && m2 == RG_M2, "rcnn_roi_geometry: written for 512 -> 128 -> 32 points (got %d -> %d -> %d)", n, m1, m2);
    PRCNN_REQUIRE(ns1 >= 1 && ns1 <= RG_NS && ns2 >= 1 && ns2 <= RG_NS && r1 > 0.f && r2 > 0.f, "rcnn_roi_geometry: nsample must be 1..64, radii positive");
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && new_xyz1 && rep1 && new_xyz2 && rep2, "rcnn_roi_geometry: null pointer");
    PRCNN_REQUIRE((idx1 && idx2) || (!idx1 && !idx2 && packs->rowinfo1), "rcnn_roi_geometry: the index tensors may only be left out (both) when the row lists are asked for");
    KeyCodec kc1, kc2;
    if (const int rc = fps_codec(RG_N, &kc1)) return rc;
    if (const int rc = fps_codec(RG_M1, &kc2)) return rc;
    hipLaunchKernelGGL(live ? rcnn_roi_geometry_kernel<true> : rcnn_roi_geometry_kernel<false>, dim3(b), dim3(64), 0, (hipStream_t)stream,
                       kc1, kc2, r1 * r1, r2 * r2, ns1, ns2, xyz, limit, new_xyz1, idx1, rep1, new_xyz2, idx2, rep2, *packs, used0);
    return check_launch("rcnn_roi_geometry");
}

extern "C" int prcnn_rcnn_roi_geometry(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                                       const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                                       void *stream)
{
    const prcnn::RgPacks none = {};
    return roi_geometry_any(b, n, m1, r1, ns1, m2, r2, ns2, xyz, limit, new_xyz1, idx1, rep1, new_xyz2, idx2, rep2, &none, stream);
}

/* prcnn_rcnn_roi_geometry + the distinct-row lists of both levels in the same launch (round 5):
 *   list 1 = prcnn_ball_pack_ex(b, b, 512, 128, ns1, idx1, limit, NULL, rep1, xyz, new_xyz1, ...),
 *   list 2 = prcnn_ball_pack_ex(b, b, 128, 32, ns2, idx2, NULL, rep1, rep2, new_xyz1, new_xyz2, ...)
 * -- the same rows per cloud in the same order, cut into the same tiles (the order of the CLOUDS' tiles in a list is whatever the
 * counter hands out, as it is for prcnn_ball_pack).  rowinfo* / rowdxyz* / tilecloud*: sized as for prcnn_ball_pack
 * (b * ceil(m * ns / 64) tiles); hdr1 / hdr2 (4 u32 each): zeroed here unless hdr_is_zero.  tilecloud1 == tilecloud2 == NULL: lists
 * whose rows carry their cloud (see RgPacks; the form the engine uses: prcnn_sa_packed_mlp reads it).  idx1 == idx2 == NULL: the index tensors
 * are not written (a caller that feeds the row lists to the packed MLP kernels has no use for them: 10240 words per cloud).
 * rowinfo3 / rowdxyz3 / hdr3 (optional, b * m2 rows at most): the list of the GroupAll level above -- every cloud one group (centre 0) of
 * its m2 level-2 centres, the centres that copy an earlier one dropped: prcnn_ball_pack_ex(b, b, m2, 1, m2, {0..m2-1}, NULL, rep2, NULL,
 * new_xyz2, origin, ...) in the row-carried form.
 * crows1 / hdr_c1 (optional, b * m1 entries at most): the level-1 centres that are their own representatives as rows cloud * m1 + centre,
 * hdr_c1[1] of them -- for prcnn_rows_gemm128_rows (the per-point layer of level 2 over exactly the rows its lists name). */
static int roi_geometry_lists(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                              const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                              unsigned int *rowinfo1, float *rowdxyz1, int *tilecloud1, unsigned int *hdr1,
                              unsigned int *rowinfo2, float *rowdxyz2, int *tilecloud2, unsigned int *hdr2,
                              unsigned int *rowinfo3, float *rowdxyz3, unsigned int *hdr3, int *crows1, unsigned int *hdr_c1,
                              int hdr_is_zero, void *stream, unsigned int *used0, bool live)
{
    PRCNN_REQUIRE(hdr1 && hdr2, "rcnn_roi_geometry_packs: null header");
    PRCNN_REQUIRE((crows1 != nullptr) == (hdr_c1 != nullptr), "rcnn_roi_geometry_packs: the centre rows come with their header");
    if (hdr_c1 && !hdr_is_zero && hipMemsetAsync(hdr_c1, 0, 4 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) {
        set_error("rcnn_roi_geometry_packs: memset failed");
        return PRCNN_ELAUNCH;
    }
    PRCNN_REQUIRE((rowinfo3 != nullptr) == (rowdxyz3 != nullptr) && (rowinfo3 != nullptr) == (hdr3 != nullptr) && (!rowinfo3 || !tilecloud1),
                  "rcnn_roi_geometry_packs: the third list comes whole, and only with lists whose rows carry their cloud");
    if (!hdr_is_zero && (hipMemsetAsync(hdr1, 0, 4 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess ||
                         hipMemsetAsync(hdr2, 0, 4 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess ||
                         (hdr3 && hipMemsetAsync(hdr3, 0, 4 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess))) {
        set_error("rcnn_roi_geometry_packs: memset failed");
        return PRCNN_ELAUNCH;
    }
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(rowinfo1 && rowdxyz1 && rowinfo2 && rowdxyz2, "rcnn_roi_geometry_packs: null pointer");
    PRCNN_REQUIRE((tilecloud1 && tilecloud2) || (!tilecloud1 && !tilecloud2 && b <= 65536), "rcnn_roi_geometry_packs: both lists with a tilecloud or none");
    PRCNN_REQUIRE((((uintptr_t)rowdxyz1 | (uintptr_t)rowdxyz2 | (uintptr_t)rowdxyz3) & 15) == 0, "rcnn_roi_geometry_packs: rowdxyz must be 16-byte aligned");
    const prcnn::RgPacks pk = {rowinfo1, (float4 *)rowdxyz1, tilecloud1, hdr1, rowinfo2, (float4 *)rowdxyz2, tilecloud2, hdr2,
                               rowinfo3, (float4 *)rowdxyz3, hdr3, crows1, hdr_c1};
    return roi_geometry_any(b, n, m1, r1, ns1, m2, r2, ns2, xyz, limit, new_xyz1, idx1, rep1, new_xyz2, idx2, rep2, &pk, stream, used0, live);
}

extern "C" int prcnn_rcnn_roi_geometry_packs(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                                             const int *limit, float *new_xyz1, int *idx1, int *rep1, float *new_xyz2, int *idx2, int *rep2,
                                             unsigned int *rowinfo1, float *rowdxyz1, int *tilecloud1, unsigned int *hdr1,
                                             unsigned int *rowinfo2, float *rowdxyz2, int *tilecloud2, unsigned int *hdr2,
                                             unsigned int *rowinfo3, float *rowdxyz3, unsigned int *hdr3, int *crows1, unsigned int *hdr_c1,
                                             int hdr_is_zero, void *stream)
{
    return roi_geometry_lists(b, n, m1, r1, ns1, m2, r2, ns2, xyz, limit, new_xyz1, idx1, rep1, new_xyz2, idx2, rep2, rowinfo1, rowdxyz1, tilecloud1,
                              hdr1, rowinfo2, rowdxyz2, tilecloud2, hdr2, rowinfo3, rowdxyz3, hdr3, crows1, hdr_c1, hdr_is_zero, stream, nullptr, false);
}

/* The "live rows" form of prcnn_rcnn_roi_geometry_packs: the same sampling, maps and centre coordinates, the same level-2 and GroupAll
 * lists -- and of level 1 only what level 2 reads.  A level-1 centre is LIVE iff a row of the level-2 list names it; list 1 holds the rows
 * of the live centres only (each as in the full list, in centre order), crows1 the live centres only, and a list with tilecloud fills a
 * cloud's last tile with copies of the cloud's last listed row.  used0 (b, 16) u32, every word written: bit k of a cloud's 512 <- a row of
 * its (kept) list 1 names pooled point k; never empty (centre 0 is always live and its ball holds point 0) -- the mask
 * prcnn_pooled_rows_src_live takes.  The index tensors are never written.  Nothing above level 2 reads a centre that is not live, nothing
 * reads a pooled point outside used0: the network's results are those of the full lists, bit for bit. */
extern "C" int prcnn_rcnn_roi_geometry_live(int b, int n, int m1, float r1, int ns1, int m2, float r2, int ns2, const float *xyz,
                                            const int *limit, float *new_xyz1, int *rep1, float *new_xyz2, int *rep2,
                                            unsigned int *rowinfo1, float *rowdxyz1, int *tilecloud1, unsigned int *hdr1,
                                            unsigned int *rowinfo2, float *rowdxyz2, int *tilecloud2, unsigned int *hdr2,
                                            unsigned int *rowinfo3, float *rowdxyz3, unsigned int *hdr3, int *crows1, unsigned int *hdr_c1,
                                            unsigned int *used0, int hdr_is_zero, void *stream)
{
    PRCNN_REQUIRE(used0 || b == 0, "rcnn_roi_geometry_live: null pointer");
    return roi_geometry_lists(b, n, m1, r1, ns1, m2, r2, ns2, xyz, limit, new_xyz1, nullptr, rep1, new_xyz2, nullptr, rep2, rowinfo1, rowdxyz1,
                              tilecloud1, hdr1, rowinfo2, rowdxyz2, tilecloud2, hdr2, rowinfo3, rowdxyz3, hdr3, crows1, hdr_c1, hdr_is_zero, stream,
                              used0, true);
}
