// fps_spec.hip -- the speculative furthest-point-sampling kernels: several picks per workgroup exchange on a Morton-ordered cloud held in
// registers, one workgroup per cloud (2048 < n <= 16384) or two (n <= 32768), and their host launchers.  fps.hip dispatches here.
#include "fps_common.hpp"
#include <stdlib.h>
#include <map>
#include <mutex>

namespace prcnn {

// ---------------------------------------------------------------------------------------------
// Spatially pruned FPS (exact).  A new pivot can lower the running minimum of point k only if
// d(k, pivot)^2 < temp[k] <= V, where V = max_k temp[k] is the value of the pivot just selected.
// So only points inside the ball of radius sqrt(V) around the pivot need a distance evaluation, and
// V shrinks as sampling proceeds (about (area / j) after j picks).  The cloud is first ordered along a
// Morton curve over (x, z) (fps_order_kernel: one workgroup per cloud, LDS counting sort), so that each
// group of 64 consecutive points -- one register slot across the lanes of a wave, a "tile" -- is
// spatially compact.  Per iteration lane i < PPT of every wave tests the pivot against the bounding box
// of tile i (a lower bound of every distance in the tile, with a 1e-5 relative safety margin that
// covers f32 rounding of both sides); tiles that cannot change are skipped, and a wave none of whose
// tiles changed re-submits its cached best.  Selected indices, tie rule and running minima are
// bit-identical to the full scan: skipped points satisfy min(d, temp) == temp.
// ---------------------------------------------------------------------------------------------

// (fps_pruned_kernel, the one-pick-per-exchange kernel of round 3 -- 4.07 ms for 32 x (16384 -> 4096) against the speculative kernel's
// 1.69 -- was removed in round 6 together with its switch PRCNN_FPS_SEQUENTIAL; the pruning above lives on in fps_spec_kernel.)

// ---------------------------------------------------------------------------------------------
// SPECULATIVE multi-pick FPS (round 4) -- the same picks as the sequential scan, several per exchange.
//
// Round 3's fps_pruned_kernel paid one workgroup-wide exchange (LDS atomic, barrier, LDS read, scalar load of the pivot) per PICK:
// 0.99 us x 4095 picks = 4.07 ms for 16384 -> 4096, the longest launch of the step and the limiter on LiDAR-shaped scenes.
// An exchange can decide MORE than one pick.  Let the points be ordered by (running minimum desc, tie key asc) and let
// g0, g1, ... be the head of that order.  g0 is the next pick.  If adding g0 leaves g1's minimum unchanged
// (d(g1, g0) >= min(g1)) then g1 is the pick after it -- every other minimum can only have decreased -- and so on: g_q
// follows as long as it is unchanged by ALL of g0 .. g_{q-1}.  Once the sampled points are dense these heads are the centres
// of separate holes and rarely interact, so a round decides several picks and the distance updates of all of them run
// behind ONE barrier.
//
// What a wave publishes when its entries changed (16 waves, one LDS table; two barriers per round: table complete / verdict in):
//   E1 = its best point (value, key, coordinates); E2 = the best point of its OTHER lanes; and a bound B = the largest value
//   any of its unpublished points can have (third among the lanes' bests, and the second bests of the two publishing lanes).
// ONE wave then merges the 32 published entries: take the best remaining entry g;
// accept it if it is the first one, or if (a) its value is STRICTLY above max_w B_w -- then every unpublished point of the
// cloud comes after it in the order -- and (b) none of the pivots accepted in this round is closer to it than its minimum
// (d < min would change it).  The first entry that fails ends the round.  Accepted pivots update the registers (tile boxes
// prune as before, against the wave's own maximum), touched waves rebuild their entries, untouched ones re-publish.
// Same picks, same tie rule, same running minima as the sequential scan, bit for bit (tests/test_gpu_ops.py,
// tests/test_gpu_reference_kernels.py: lattices and duplicate clouds with thousands of exact ties included).
// ---------------------------------------------------------------------------------------------
constexpr int FS_RMAX = 16;     // picks per round at most

// a value that every lane of the wave holds, as a wave-uniform one (v_readfirstlane: the compiler keeps it in an SGPR)
__device__ __forceinline__ float fs_uniform(float v)
{
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ float fs_readlane(float v, int l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// c <- the smallest key among the lanes `in`, m <- the lanes `in && also` that hold it.  Round 7: the lanes `in` are those whose value
// equals a wave maximum -- ONE lane unless values tie exactly -- and then the key is that lane's, read with v_readlane: a ballot and
// a population count in place of a cross-lane minimum (four DPP steps, four v_readlane) on the rebuild's dependent chain.
__device__ __forceinline__ void fs_key_of(bool in, bool also, uint32_t lk, uint32_t &c, unsigned long long &m)
{
    const unsigned long long a = __ballot(in);
    if (__popcll(a) == 1) c = (uint32_t)__builtin_amdgcn_readlane((int)lk, (int)__builtin_ctzll(a));
    else c = wave_min_u32(in ? lk : 0xffffffffu);
    m = a & __ballot(also && lk == c);
}

// coordinates of point (lane l, slot) -- both wave-uniform -- as three v_readlane behind scalar compares: a binary tree over the slot,
// log2(PPT) compare-and-branch (round 7; until then a ladder `slot == 0, == 1, ...`, up to PPT of them).  (Indexing the register arrays
// with the uniform slot made the compiler keep scratch copies of px / py / pz once the kernel was at its 128-VGPR limit; a per-lane
// select chain would cost 3 x PPT VALU instructions per rebuild.)
template <int PPT, int LO = 0, int N = PPT>
__device__ __forceinline__ void fs_pick3(const float (&px)[PPT], const float (&py)[PPT], const float (&pz)[PPT], int slot, int l,
                                         float &x, float &y, float &z)
{
    if constexpr (N == 1) {
        x = fs_readlane(px[LO], l); y = fs_readlane(py[LO], l); z = fs_readlane(pz[LO], l);
    } else if (slot < LO + N / 2) {
        fs_pick3<PPT, LO, N / 2>(px, py, pz, slot, l, x, y, z);
    } else {
        fs_pick3<PPT, LO + N / 2, N / 2>(px, py, pz, slot, l, x, y, z);
    }
}

template <int PPT>
__global__ __launch_bounds__(1024) void fps_spec_kernel(
    int n, int m, KeyCodec kc, const float *__restrict__ xyz, const int *__restrict__ perm,
    float *__restrict__ temp, int *__restrict__ idx, float *__restrict__ new_xyz, const int *__restrict__ rejected = nullptr)
{
    // temp == NULL: the running minima start at the reference caller's fill value (1e10, pointnet2_utils.py:26) and are not handed back;
    // new_xyz != NULL: the coordinates of the picks are written as well (prcnn_fps_new_xyz: the caller's gather launch folded in);
    // rejected: as in fps_reg_kernel
    constexpr int SB = PPT == 16 ? 4 : (PPT == 8 ? 3 : 2);          // slot bits below the tie key
    __shared__ unsigned long long s_vk[32];                          // packed (value, key) of the published entries
    __shared__ float s_xyz[32][3];
    __shared__ float s_bound[16];
    __shared__ int s_rank[32], s_blk[32];                            // per entry: entries that precede it / one of them blocks it
    const int b = blockIdx.x;
    if (rejected && rejected[b] == 0) return;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    const int *__restrict__ order = perm + (long)b * n;
    float *__restrict__ mind = temp ? temp + (long)b * n : nullptr;
    int *__restrict__ sel = idx + (long)b * m;
    float *__restrict__ nxyz = new_xyz ? new_xyz + (long)b * m * 3 : nullptr;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    __builtin_amdgcn_s_setprio(3);

    // COPIED in fps_spec2_kernel (keep the two in step): the tile load and box reduction, box_mask, update, and the rebuild of the wave's
    // entries in step 1.  Held in a struct or passed to shared helpers these blocks compile to other (and more) instructions HERE, so
    // they stay as text; the copies differ where fps_spec2_kernel says so.
    float px[PPT], py[PPT], pz[PPT], pt[PPT];
    uint32_t pc[PPT];                                                 // (tie key << SB) | slot; ~0 for a slot beyond the cloud
    float bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY, bz0 = INFINITY, bz1 = -INFINITY;
    float wx0 = INFINITY, wx1 = -INFINITY, wy0 = INFINITY, wy1 = -INFINITY, wz0 = INFINITY, wz1 = -INFINITY;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        // position in Morton order: a wave = 1024 consecutive positions.  (Round 6, measured and not kept: tiles or tile PAIRS dealt
        // round-robin to the waves so that a pivot's neighbourhood is spread over them -- with the lazy rebuild of round 5 in place:
        // pairs 1.91 / 2.32 ms, single tiles 2.04 / 2.41 ms against 1.69 / 2.46 ms, uniform / LiDAR-shaped, same picks.)
        const int s = w * (64 * PPT) + i * 64 + lane;
        float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
        if (s < n) {
            const int k = order[s];
            px[i] = cloud[3 * k]; py[i] = cloud[3 * k + 1]; pz[i] = cloud[3 * k + 2];
            pt[i] = mind ? mind[k] : 1e10f;
            pc[i] = (kc.encode(k) << SB) | (uint32_t)i;
            x0 = x1 = px[i]; y0 = y1 = py[i]; z0 = z1 = pz[i];
        } else {
            px[i] = py[i] = pz[i] = 0.f;
            pt[i] = -INFINITY;
            pc[i] = 0xffffffffu;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = fmin_raw(x0, __shfl_xor(x0, d, 64)); x1 = fmax_raw(x1, __shfl_xor(x1, d, 64));
            y0 = fmin_raw(y0, __shfl_xor(y0, d, 64)); y1 = fmax_raw(y1, __shfl_xor(y1, d, 64));
            z0 = fmin_raw(z0, __shfl_xor(z0, d, 64)); z1 = fmax_raw(z1, __shfl_xor(z1, d, 64));
        }
        if (lane == i) { bx0 = x0; bx1 = x1; by0 = y0; by1 = y1; bz0 = z0; bz1 = z1; }
        wx0 = fmin_raw(wx0, x0); wx1 = fmax_raw(wx1, x1); wy0 = fmin_raw(wy0, y0); wy1 = fmax_raw(wy1, y1);
        wz0 = fmin_raw(wz0, z0); wz1 = fmax_raw(wz1, z1);
    }
    // the wave's OWN box, the union of its tile boxes (round 7): six wave-uniform values, held in SGPRs -- see wave_hit
    wx0 = fs_uniform(wx0); wx1 = fs_uniform(wx1); wy0 = fs_uniform(wy0); wy1 = fs_uniform(wy1); wz0 = fs_uniform(wz0); wz1 = fs_uniform(wz1);

    // lane i < PPT holds the box of tile i: ONE pivot, its coordinates wave-uniform, is tested against the PPT tile boxes at a time
    // (rounds 4-6: every group of PPT lanes held the boxes and 64 / PPT pivots were tested per pass; fps_spec2_kernel still does)
    // pivots against the registers: tile boxes prune against `bound`, an upper bound of every running minimum of this wave
    // `touched`: one of the tiles that hold this wave's two PUBLISHED points went through an update -- only then are its entries rebuilt
    // (round 5).  A pivot that changes other points of the wave leaves the published points, their values and keys as they are, and
    // the published bound B (and `bound` below) stays an upper bound of everything unpublished, since running minima only fall: the
    // merge stays exact with the stale bound, it may only accept fewer entries.  Measured on the round model (profiles/fps_round_sim.py
    // lazy): 7.7 instead of 10.1 rebuilds per round on the uniform scene, 5.1 instead of 6.9 on the LiDAR-shaped one, the rounds
    // themselves 481 / 742 against 480 / 742.
    unsigned long long touched = 0ull, etiles = ~0ull;
    float bound = INFINITY;
    // which tiles can the pivot change?  bit i: tile i (live: lane < PPT)
    auto box_mask = [&](float ox, float oy, float oz, bool live) __attribute__((always_inline)) {
        const float dx = fmax_raw(fmax_raw(bx0 - ox, ox - bx1), 0.f);
        const float dy = fmax_raw(fmax_raw(by0 - oy, oy - by1), 0.f);
        const float dz = fmax_raw(fmax_raw(bz0 - oz, oz - bz1), 0.f);
        const float lb = dx * dx + dy * dy + dz * dz;
        return __ballot(live && !(lb * 0.99999f >= bound));           // empty boxes give lb = +inf
    };
    // WAVE-LEVEL CULL (round 7): can the point (ox, oy, oz) -- per lane -- change ANY point of this wave?  The same test as box_mask,
    // same margin, same `bound`, against the wave's own box.  Exact: the wave box contains every tile box, so each of dx, dy, dz and
    // with them lb (sums and products of non-negative terms, every rounding monotone) is no larger than the tile's -- a point that fails
    // here fails box_mask for every tile.  It runs in the merge, where lane e already HOLDS entry e's coordinates, in front of
    // barrier A2 (whose wait hides it): the round's pivots are then known per wave as a set of entry lanes, and phase 4 box-tests
    // only those, one by one, reading their coordinates with v_readlane.  Rounds 4-6 sent every pivot through the tile tests of
    // every wave -- ceil(r / 4) passes of 3 ds_bpermute + ~15 VALU + a ballot at the head of the busiest wave's chain
    // (profiles/r06_fps_round_stamps.txt) -- behind three ds_permute that put pivot q into lanes 3 q .. 3 q + 2 of one register;
    // a wave a sixteenth of the cloud sees 1-3 of a round's 8.5 pivots, and neither permute is needed to find them.
    auto wave_hit = [&](float ox, float oy, float oz) __attribute__((always_inline)) {
        const float dx = fmax_raw(fmax_raw(wx0 - ox, ox - wx1), 0.f);
        const float dy = fmax_raw(fmax_raw(wy0 - oy, oy - wy1), 0.f);
        const float dz = fmax_raw(fmax_raw(wz0 - oz, oz - wz1), 0.f);
        const float lb = dx * dx + dy * dy + dz * dz;
        return !(lb * 0.99999f >= bound);
    };
    auto update = [&](float ox, float oy, float oz, unsigned long long mask) __attribute__((always_inline)) {
        if (mask != 0ull) {
            touched |= mask & etiles;
            // Tiles in PAIRS on packed f32 arithmetic (round 5): v_pk_add / v_pk_mul / v_pk_fma apply to each half exactly the operation
            // of the scalar form (one rounding each), so a tile's new minima are the same bits; a pair is updated when EITHER tile passed
            // the box test -- for the other one the update is the identity (no point of a pruned tile can come closer than its minimum:
            // that is what the pruning rests on).  8 packed + 2 min instructions per pair instead of 9 per tile.
            const pk_f32x2 o_x = {ox, ox}, o_y = {oy, oy}, o_z = {oz, oz};
            if (kc.hipcc) {
#pragma unroll
                for (int i = 0; i < PPT; i += 2)
                    if ((mask >> i) & 3ull) {
                        const pk_f32x2 dx = (pk_f32x2){px[i], px[i + 1]} - o_x, dy = (pk_f32x2){py[i], py[i + 1]} - o_y,
                                       dz = (pk_f32x2){pz[i], pz[i + 1]} - o_z;
                        const pk_f32x2 d = __builtin_elementwise_fma(dy, dy, dx * dx) + dz * dz;
                        pt[i] = fmin_raw(d.x, pt[i]); pt[i + 1] = fmin_raw(d.y, pt[i + 1]);
                    }
            } else {
#pragma unroll
                for (int i = 0; i < PPT; i += 2)
                    if ((mask >> i) & 3ull) {
                        const pk_f32x2 dx = (pk_f32x2){px[i], px[i + 1]} - o_x, dy = (pk_f32x2){py[i], py[i + 1]} - o_y,
                                       dz = (pk_f32x2){pz[i], pz[i + 1]} - o_z;
                        const pk_f32x2 d = (dx * dx + dy * dy) + dz * dz;
                        pt[i] = fmin_raw(d.x, pt[i]); pt[i + 1] = fmin_raw(d.y, pt[i + 1]);
                    }
            }
        }
    };
    if (t == 0) {
        sel[0] = 0;
        if (nxyz) { nxyz[0] = cloud[0]; nxyz[1] = cloud[1]; nxyz[2] = cloud[2]; }
    }
    if (t < 32) { s_rank[t] = 0; s_blk[t] = 0; }                      // (the first barrier A orders this before any atomic)
    int j = 1;                                                        // picks made so far
    if (m > 1) {                                                      // the given start point, index 0
        const float ox = cloud[0], oy = cloud[1], oz = cloud[2];
        update(ox, oy, oz, box_mask(ox, oy, oz, lane < PPT));
    }
    touched = ~0ull;                                                  // the entries have to be built
    while (j < m) {
        // ---- 1. this wave's entries: rebuilt when one of its tiles changed
        if (touched != 0ull) {
            float bv = -INFINITY, sv = -INFINITY;                     // best and second-best VALUE of this lane
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                sv = __builtin_amdgcn_fmed3f(bv, sv, pt[i]);          // = max(sv, min(bv, pt)) while sv <= bv: one v_med3_f32
                bv = fmax_raw(bv, pt[i]);
            }
            uint32_t lk = 0xffffffffu;                                // (key, slot) of this lane's best
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const uint32_t c = pt[i] == bv ? pc[i] : 0xffffffffu;
                lk = c < lk ? c : lk;
            }
            // best lane, best of the other lanes, third value
            const float v1 = wave_max_f32(bv);
            uint32_t c1; unsigned long long m1;
            fs_key_of(bv == v1, true, lk, c1, m1);
            const int l1 = m1 ? (int)__builtin_ctzll(m1) : 0;
            const float bv2 = lane == l1 ? -INFINITY : bv;
            const float v2 = wave_max_f32(bv2);
            uint32_t c2; unsigned long long m2;
            fs_key_of(bv2 == v2, lane != l1, lk, c2, m2);
            const int l2 = m2 ? (int)__builtin_ctzll(m2) : l1;
            const float v3 = wave_max_f32((lane == l1 || lane == l2) ? -INFINITY : bv);
            const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), l1));
            const float s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), l2));
            const float wB = fmax_raw(v3, fmax_raw(s1, s2));
            bound = v1;
            const int sl1 = (int)(c1 & ((1u << SB) - 1u)), sl2 = (int)(c2 & ((1u << SB) - 1u));
            const bool has2 = m2 != 0ull && c2 != 0xffffffffu;
            etiles = (1ull << sl1) | (has2 ? (1ull << sl2) : 0ull);
            // ---- 2. publish (only a wave whose entries changed writes: the table keeps the others'): lane 0 the best point, lane 1
            // the best point of the other lanes
            float x1 = 0.f, y1 = 0.f, z1 = 0.f, x2 = 0.f, y2 = 0.f, z2 = 0.f;
            fs_pick3<PPT>(px, py, pz, __builtin_amdgcn_readfirstlane(sl1), l1, x1, y1, z1);
            fs_pick3<PPT>(px, py, pz, __builtin_amdgcn_readfirstlane(sl2), l2, x2, y2, z2);
            const float ex = lane == 0 ? x1 : x2, ey = lane == 0 ? y1 : y2, ez = lane == 0 ? z1 : z2;
            if (lane < 2) {
                const float ev = lane == 0 ? v1 : (has2 ? v2 : -INFINITY);
                const uint32_t ek = lane == 0 ? (c1 == 0xffffffffu ? 0xffffffffu : (c1 >> SB)) : (has2 ? (c2 >> SB) : 0xffffffffu);
                s_vk[2 * w + lane] = pack_candidate(ev, ek);
                s_xyz[2 * w + lane][0] = ex; s_xyz[2 * w + lane][1] = ey; s_xyz[2 * w + lane][2] = ez;
                if (lane == 0) s_bound[w] = wB;
            }
        }
        lds_barrier();                                                // A: the table is complete
        // ---- 3. merge (round 6 form: two barriers per round, no LDS atomic, no verdict broadcast).  All 32 x 32 pairs at once over the
        // 16 waves: wave w OWNS entries 2 w and 2 w + 1 -- lane (e = lane & 31, h = lane >> 5) compares entry i = 2 w + h with entry e:
        // does e precede i in the order (value desc, key asc), and does it lie closer to i than i's running minimum?  Entry i's RANK
        // (how many precede it) and its BLOCKED bit are a population count / a test of one half of a ballot: wave-uniform, written by
        // one lane.  Behind the second barrier EVERY wave reads the 32 ranks and derives the verdict itself -- the picks of the round
        // are the ranks 0 .. r-1 up to the first rank that fails -- so nobody waits for wave 0 and a third barrier; the pivots stay
        // in their entry lanes (round 6 permuted pivot q into lane q of every wave: ds_permute, lane e sends to lane rank(e)).
        // (Rounds 4-5: lane = entry i, wave = entry e, ranks summed through LDS atomics, the verdict by wave 0 into s_res, barrier B:
        // pairs 540 + verdict 760 + the barrier ~ 1500 of a round's 8200 cycles, profiles/r05_fps_round_stamps.txt.  History before that:
        // every wave merging the whole table by sequential extraction -- issue-bound, 5.2 ms; one wave walking its half of the table,
        // 16 dependent LDS round trips: 2.6 k of 10.2 k cycles.)
        const int left = m - j;
        const int e = lane & 31, h = lane >> 5;
        const unsigned long long pke = s_vk[e];
        float cv; uint32_t ck;                                        // entry e: what this lane is responsible for in the verdict
        unpack_candidate(pke, cv, ck);
        const float cx = s_xyz[e][0], cy = s_xyz[e][1], cz = s_xyz[e][2];
        const float gB = wave_max_f32(lane < 16 ? s_bound[lane] : -INFINITY);     // (read in front of A2: the next publish rewrites it behind A2)
        {
            const int i = 2 * w + h;
            const unsigned long long pki = s_vk[i];
            float iv; uint32_t ik;
            unpack_candidate(pki, iv, ik);
            const float ix = s_xyz[i][0], iy = s_xyz[i][1], iz = s_xyz[i][2];
            const bool before = pke > pki;
            const float d = kc.hipcc ? fps_dist<true>(ix, iy, iz, cx, cy, cz) : sqdist3(ix, iy, iz, cx, cy, cz);
            const unsigned long long bb = __ballot(before), kb = __ballot(before && (d < iv));
            if (e == 0) {
                s_rank[i] = __popc((unsigned)(h ? (bb >> 32) : bb));
                s_blk[i] = (unsigned)(h ? (kb >> 32) : kb) != 0u;
            }
        }
        const bool valid = !(ck == 0xffffffffu || !(cv > -1.0f));      // (reference: best starts at -1, besti at 0)
        // should entry e become a pivot of this round: does it reach this wave?  (an invalid first entry stands for point 0: always)
        const bool hit = wave_hit(cx, cy, cz) || !valid;
        lds_barrier();                                                // A2: every entry has its rank
        const int rank = s_rank[e];
        const bool blocked = s_blk[e] != 0;
        const bool pass = rank == 0 ? true : ((cv > gB) && (cv > 0.f) && valid && !blocked);
        // a round ends behind an invalid first entry (the reference then picks index 0: every running minimum is below -1 / NaN)
        const bool stop = !pass || (rank == 0 && !valid);
        int r = (int)wave_min_u32((stop && !(rank == 0)) ? (uint32_t)rank : ((rank == 0 && !valid) ? 1u : 32u));
        r = min(min(r, left), FS_RMAX);
        if (r < 1) r = 1;
        const float ox_ = valid ? cx : cloud[0], oy_ = valid ? cy : cloud[1], oz_ = valid ? cz : cloud[2];
        if (w == 0 && h == 0 && rank < r) {                           // the outputs: one wave writes them
            sel[j + rank] = valid ? kc.decode(ck) : 0;
            if (nxyz) { nxyz[3 * (j + rank)] = ox_; nxyz[3 * (j + rank) + 1] = oy_; nxyz[3 * (j + rank) + 2] = oz_; }
        }
        // ---- 4. running minima against this round's pivots (the last pick of the whole run does not update them: sampling_gpu.cu)
        // The pivots stay where they are, in the entry lanes (first half, rank < apply_n); this wave's share of them is one ballot.
        // In which order a wave applies them is free: a running minimum is a min over the pivots, `touched` an OR.
        // (Rounds 4-6 permuted pivot q into lanes 3 q .. 3 q + 2 of one register; three registers, lane q = pivot q, spilled
        // fps_spec_kernel<16> at its 128-register limit THEN -- the three here replace that register and the permutes' operands.)
        j += r;
        const int apply_n = j >= m ? r - 1 : r;
        touched = 0ull;
        unsigned mine = (unsigned)__ballot(h == 0 && rank < apply_n && hit);
        while (mine != 0u) {
            const int l = __builtin_ctz(mine);
            mine &= mine - 1u;
            const float ox = fs_readlane(ox_, l), oy = fs_readlane(oy_, l), oz = fs_readlane(oz_, l);
            update(ox, oy, oz, box_mask(ox, oy, oz, lane < PPT));
        }
    }
    if (mind) {
#pragma unroll
        for (int i = 0; i < PPT; ++i)
            if (pc[i] != 0xffffffffu) mind[kc.decode(pc[i] >> SB)] = pt[i];
    }
}

// ---------------------------------------------------------------------------------------------
// The speculative kernel for 16384 < n <= 32768 (round 5: tools/cfgs/double.yaml, NUM_POINTS 32768): TWO workgroups per cloud.
//
// 32768 points x (x, y, z, running minimum) do not fit one compute unit's registers (a 1024-thread workgroup has 128 VGPRs per thread:
// 16 points each), and streaming half of them from L2 for every pick is what fps_generic_kernel does (~3.5 us per pick).  Here the
// cloud in Morton order is cut in two and each half lives in the registers of a workgroup of its own, exactly as in fps_spec_kernel<16>;
// the two workgroups run the SAME rounds in lockstep:
//   * every wave publishes its two entries + its bound into the round's table in GLOBAL memory (64 entries, two tables alternating:
//     a table is rewritten two rounds later, when both workgroups are provably past reading it);
//   * one cross-workgroup barrier per round (a monotonic counter per cloud: agent-scope release add, acquire spin);
//   * each workgroup copies the 64 entries into its LDS and computes the verdict over all 64 x 64 pairs REDUNDANTLY -- the merge is
//     deterministic, both arrive at the same picks, no second exchange is needed; workgroup 0 writes the outputs;
//   * each updates the running minima of its own half against the round's pivots.
// Same picks, tie rule and running minima as the sequential scan (tests/test_gpu_ops.py: oracle-exact, lattices and duplicates).
// Placement: the halves of a cloud are blocks q and q + 8 -- dispatched to the same XCD, one right after the other, so a half never
// waits for a partner that cannot be scheduled behind workgroups that themselves wait (see fps_any).
// ---------------------------------------------------------------------------------------------
struct Fps2Table {                                                   // per cloud, in the library's scratch (zeroed `sync` per launch)
    unsigned long long vk[2][64];
    float xyz[2][64][4];
    float bound[2][32];
    unsigned int sync;
    unsigned int pad[63];
};

__device__ __forceinline__ unsigned long long ld_agent_u64(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent_f32(const float *p)
{
    return __int_as_float(__hip_atomic_load(reinterpret_cast<const int *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ void st_agent_u64(unsigned long long *p, unsigned long long v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent_f32(float *p, float v)
{
    __hip_atomic_store(reinterpret_cast<int *>(p), __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(1024) void fps_spec2_kernel(
    int nclouds, int n, int m, KeyCodec kc, const float *__restrict__ xyz, const int *__restrict__ perm,
    float *__restrict__ temp, int *__restrict__ idx, float *__restrict__ new_xyz, Fps2Table *__restrict__ tables)
{
    constexpr int PPT = 16, SB = 4, NE = 64;
    __shared__ unsigned long long s_vk[NE];
    __shared__ float s_xyz[NE][3];
    __shared__ float s_bound[32];
    __shared__ float s_res[64];
    __shared__ int s_rank[NE], s_blk[NE];
    __shared__ unsigned long long s_evk[32];                         // this workgroup's published entries between rebuilds (the registers are full)
    __shared__ float s_exyz[32][3], s_eb[16];
    // blocks q and q + 8 (same XCD) are the two halves of cloud (q / 16) * 8 + q % 8
    const int q_ = blockIdx.x;
    const int b = (q_ >> 4) * 8 + (q_ & 7), half = (q_ >> 3) & 1;
    if (b >= nclouds) return;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    const int *__restrict__ order = perm + (long)b * n;
    float *__restrict__ mind = temp ? temp + (long)b * n : nullptr;
    int *__restrict__ sel = idx + (long)b * m;
    float *__restrict__ nxyz = new_xyz ? new_xyz + (long)b * m * 3 : nullptr;
    Fps2Table *__restrict__ tb = tables + b;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, gw = 16 * half + w;       // gw: this wave among the cloud's 32
    __builtin_amdgcn_s_setprio(3);

    // COPIES of fps_spec_kernel<16>'s blocks (keep them in step; the comments are there): tile load and box reduction (the wave's own box
    // with it), box_mask, wave_hit, update, the rebuild of the wave's entries.  The differences: the wave's first Morton position is
    // gw's, not w's; `touched |= mask` without `& etiles` -- on purpose: this kernel keeps its entries in LDS and rebuilds on any touch;
    // and the wave-level cull runs behind barrier B on the round's pivots as wave 0 left them in s_res (lane q = pivot q, rank order),
    // not on the entries in front of A2: here ONE wave holds the verdict, the others never see the ranks.  A surviving pivot's
    // coordinates are read from s_res again (a broadcast read), not kept in three registers over the loop: this kernel spills
    // (12 registers; 14 with the three, and 8 x (32768 -> 4096) then takes 3.06 / 7.30 ms against 2.92 / 6.97 ms uniform /
    // LiDAR-shaped -- before round 7: 2.97 / 6.95 ms).  Any change here is measured at that shape: the rebuild's key shortcut alone,
    // with the pivot passes of round 6, ALSO spilled 14 and ran 3.15 / 7.8 ms.
    float px[PPT], py[PPT], pz[PPT], pt[PPT];
    uint32_t pc[PPT];
    float bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY, bz0 = INFINITY, bz1 = -INFINITY;
    float wx0 = INFINITY, wx1 = -INFINITY, wy0 = INFINITY, wy1 = -INFINITY, wz0 = INFINITY, wz1 = -INFINITY;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int s = gw * (64 * PPT) + i * 64 + lane;
        float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
        if (s < n) {
            const int k = order[s];
            px[i] = cloud[3 * k]; py[i] = cloud[3 * k + 1]; pz[i] = cloud[3 * k + 2];
            pt[i] = mind ? mind[k] : 1e10f;
            pc[i] = (kc.encode(k) << SB) | (uint32_t)i;
            x0 = x1 = px[i]; y0 = y1 = py[i]; z0 = z1 = pz[i];
        } else {
            px[i] = py[i] = pz[i] = 0.f;
            pt[i] = -INFINITY;
            pc[i] = 0xffffffffu;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = fmin_raw(x0, __shfl_xor(x0, d, 64)); x1 = fmax_raw(x1, __shfl_xor(x1, d, 64));
            y0 = fmin_raw(y0, __shfl_xor(y0, d, 64)); y1 = fmax_raw(y1, __shfl_xor(y1, d, 64));
            z0 = fmin_raw(z0, __shfl_xor(z0, d, 64)); z1 = fmax_raw(z1, __shfl_xor(z1, d, 64));
        }
        if (lane == i) { bx0 = x0; bx1 = x1; by0 = y0; by1 = y1; bz0 = z0; bz1 = z1; }
        wx0 = fmin_raw(wx0, x0); wx1 = fmax_raw(wx1, x1); wy0 = fmin_raw(wy0, y0); wy1 = fmax_raw(wy1, y1);
        wz0 = fmin_raw(wz0, z0); wz1 = fmax_raw(wz1, z1);
    }
    wx0 = fs_uniform(wx0); wx1 = fs_uniform(wx1); wy0 = fs_uniform(wy0); wy1 = fs_uniform(wy1); wz0 = fs_uniform(wz0); wz1 = fs_uniform(wz1);
    unsigned long long touched = 0ull;
    float bound = INFINITY;
    auto box_mask = [&](float ox, float oy, float oz, bool live) __attribute__((always_inline)) {
        const float dx = fmax_raw(fmax_raw(bx0 - ox, ox - bx1), 0.f);
        const float dy = fmax_raw(fmax_raw(by0 - oy, oy - by1), 0.f);
        const float dz = fmax_raw(fmax_raw(bz0 - oz, oz - bz1), 0.f);
        const float lb = dx * dx + dy * dy + dz * dz;
        return __ballot(live && !(lb * 0.99999f >= bound));
    };
    auto wave_hit = [&](float ox, float oy, float oz) __attribute__((always_inline)) {
        const float dx = fmax_raw(fmax_raw(wx0 - ox, ox - wx1), 0.f);
        const float dy = fmax_raw(fmax_raw(wy0 - oy, oy - wy1), 0.f);
        const float dz = fmax_raw(fmax_raw(wz0 - oz, oz - wz1), 0.f);
        const float lb = dx * dx + dy * dy + dz * dz;
        return !(lb * 0.99999f >= bound);
    };
    auto update = [&](float ox, float oy, float oz, unsigned long long mask) __attribute__((always_inline)) {
        if (mask != 0ull) {
            touched |= mask;                                          // (no `& etiles`: entries in LDS, rebuilt on ANY touch)
            // tile pairs on packed f32 arithmetic, as in fps_spec_kernel
            const pk_f32x2 o_x = {ox, ox}, o_y = {oy, oy}, o_z = {oz, oz};
            if (kc.hipcc) {
#pragma unroll
                for (int i = 0; i < PPT; i += 2)
                    if ((mask >> i) & 3ull) {
                        const pk_f32x2 dx = (pk_f32x2){px[i], px[i + 1]} - o_x, dy = (pk_f32x2){py[i], py[i + 1]} - o_y,
                                       dz = (pk_f32x2){pz[i], pz[i + 1]} - o_z;
                        const pk_f32x2 d = __builtin_elementwise_fma(dy, dy, dx * dx) + dz * dz;
                        pt[i] = fmin_raw(d.x, pt[i]); pt[i + 1] = fmin_raw(d.y, pt[i + 1]);
                    }
            } else {
#pragma unroll
                for (int i = 0; i < PPT; i += 2)
                    if ((mask >> i) & 3ull) {
                        const pk_f32x2 dx = (pk_f32x2){px[i], px[i + 1]} - o_x, dy = (pk_f32x2){py[i], py[i + 1]} - o_y,
                                       dz = (pk_f32x2){pz[i], pz[i + 1]} - o_z;
                        const pk_f32x2 d = (dx * dx + dy * dy) + dz * dz;
                        pt[i] = fmin_raw(d.x, pt[i]); pt[i + 1] = fmin_raw(d.y, pt[i + 1]);
                    }
            }
        }
    };
    if (t == 0 && half == 0) {
        sel[0] = 0;
        if (nxyz) { nxyz[0] = cloud[0]; nxyz[1] = cloud[1]; nxyz[2] = cloud[2]; }
    }
    if (t < NE) { s_rank[t] = 0; s_blk[t] = 0; }
    int j = 1;
    if (m > 1) {
        const float ox = cloud[0], oy = cloud[1], oz = cloud[2];
        update(ox, oy, oz, box_mask(ox, oy, oz, lane < PPT));
    }
    touched = ~0ull;
    // this wave's published entries are kept in LDS between rebuilds; every round copies them into the round's table
    unsigned int round = 0;
    while (j < m) {
        if (touched != 0ull) {
            float bv = -INFINITY, sv = -INFINITY;
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                sv = __builtin_amdgcn_fmed3f(bv, sv, pt[i]);
                bv = fmax_raw(bv, pt[i]);
            }
            uint32_t lk = 0xffffffffu;
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const uint32_t c = pt[i] == bv ? pc[i] : 0xffffffffu;
                lk = c < lk ? c : lk;
            }
            const float v1 = wave_max_f32(bv);
            uint32_t c1; unsigned long long m1;
            fs_key_of(bv == v1, true, lk, c1, m1);
            const int l1 = m1 ? (int)__builtin_ctzll(m1) : 0;
            const float bv2 = lane == l1 ? -INFINITY : bv;
            const float v2 = wave_max_f32(bv2);
            uint32_t c2; unsigned long long m2;
            fs_key_of(bv2 == v2, lane != l1, lk, c2, m2);
            const int l2 = m2 ? (int)__builtin_ctzll(m2) : l1;
            const float v3 = wave_max_f32((lane == l1 || lane == l2) ? -INFINITY : bv);
            const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), l1));
            const float s2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), l2));
            const float e_b = fmax_raw(v3, fmax_raw(s1, s2));
            bound = v1;
            const int sl1 = (int)(c1 & ((1u << SB) - 1u)), sl2 = (int)(c2 & ((1u << SB) - 1u));
            const bool has2 = m2 != 0ull && c2 != 0xffffffffu;
            float x1 = 0.f, y1 = 0.f, z1 = 0.f, x2 = 0.f, y2 = 0.f, z2 = 0.f;
            fs_pick3<PPT>(px, py, pz, __builtin_amdgcn_readfirstlane(sl1), l1, x1, y1, z1);
            fs_pick3<PPT>(px, py, pz, __builtin_amdgcn_readfirstlane(sl2), l2, x2, y2, z2);
            const float ev = lane == 0 ? v1 : (has2 ? v2 : -INFINITY);
            const uint32_t ek = lane == 0 ? (c1 == 0xffffffffu ? 0xffffffffu : (c1 >> SB)) : (has2 ? (c2 >> SB) : 0xffffffffu);
            if (lane < 2) {
                s_evk[2 * w + lane] = pack_candidate(ev, ek);
                s_exyz[2 * w + lane][0] = lane == 0 ? x1 : x2; s_exyz[2 * w + lane][1] = lane == 0 ? y1 : y2; s_exyz[2 * w + lane][2] = lane == 0 ? z1 : z2;
                if (lane == 0) s_eb[w] = e_b;
            }
        }
        const int par = (int)(round & 1u);
        if (lane < 2) {                                               // (the same lanes wrote the LDS copy: program order)
            const int e = 2 * gw + lane, le = 2 * w + lane;
            st_agent_u64(&tb->vk[par][e], s_evk[le]);
            st_agent_f32(&tb->xyz[par][e][0], s_exyz[le][0]); st_agent_f32(&tb->xyz[par][e][1], s_exyz[le][1]);
            st_agent_f32(&tb->xyz[par][e][2], s_exyz[le][2]);
            if (lane == 0) st_agent_f32(&tb->bound[par][gw], s_eb[w]);
        }
        // ---- the round's cross-workgroup barrier: both halves have published.  ADVICE r5: a workgroup barrier orders nothing beyond the
        // workgroup, and thread 0's agent-scope release waits for ITS wave's stores only.  So the table stores are agent-scope
        // write-throughs (st_agent_*: they are complete when they are acknowledged, nothing stays dirty in a cache that a release
        // would have to write back) and EVERY wave waits for its own acknowledgements before the workgroup barrier: when thread 0
        // signals, the whole table is at the agent's coherence point.  (A full agent-scope release fence per wave and round --
        // buffer_wbl2, an L2 write-back walk -- does the same and HALVED the kernel: double.yaml 5011 -> 2420 scenes/s.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            __hip_atomic_fetch_add(&tb->sync, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned int want = 2u * (round + 1u);
            // bounded: the host side only launches grids that fit the chip twice over (fps2_capacity), so the partner IS resident or
            // becomes resident as other work retires; should it never arrive (a CU mask narrower than the one the capacity was
            // computed under, a partition change) the launch dies loudly after ~4 s of the 100-MHz clock instead of hanging the GPU
            const long long t0 = wall_clock64();
            while (__hip_atomic_load(&tb->sync, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) {
                __builtin_amdgcn_s_sleep(1);
                if (wall_clock64() - t0 > 400000000ll) __builtin_trap();
            }
        }
        __syncthreads();
        if (t < NE) {
            s_vk[t] = ld_agent_u64(&tb->vk[par][t]);
            s_xyz[t][0] = ld_agent_f32(&tb->xyz[par][t][0]);
            s_xyz[t][1] = ld_agent_f32(&tb->xyz[par][t][1]);
            s_xyz[t][2] = ld_agent_f32(&tb->xyz[par][t][2]);
            if (t < 32) s_bound[t] = ld_agent_f32(&tb->bound[par][t]);
        }
        __syncthreads();                                              // A: the table is complete (in this workgroup's LDS)
        // ---- merge: lane = entry i, wave w compares it with entries 4 w .. 4 w + 3 (all 64 x 64 pairs over the 16 waves)
        const int left = m - j;
        const int i = lane;
        const unsigned long long pki = s_vk[i];
        float cv; uint32_t ck;
        unpack_candidate(pki, cv, ck);
        const float cx = s_xyz[i][0], cy = s_xyz[i][1], cz = s_xyz[i][2];
        {
            int rk = 0;
            bool bl = false;
#pragma unroll 1
            for (int u = 0; u < 4; ++u) {
                const int e = 4 * w + u;
                const unsigned long long pke = s_vk[e];
                const float ex = s_xyz[e][0], ey = s_xyz[e][1], ez = s_xyz[e][2];
                const bool before = pke > pki;
                const float d = kc.hipcc ? fps_dist<true>(cx, cy, cz, ex, ey, ez) : sqdist3(cx, cy, cz, ex, ey, ez);
                rk += before ? 1 : 0;
                bl = bl || (before && (d < cv));
            }
            if (rk) atomicAdd(&s_rank[i], rk);
            if (bl) atomicOr(&s_blk[i], 1);
        }
        lds_barrier();                                                // A2
        if (w == 0) {
            const int rank = s_rank[i];
            const bool blocked = s_blk[i] != 0;
            const float gB = wave_max_f32(lane < 32 ? s_bound[lane] : -INFINITY);
            const bool valid = !(ck == 0xffffffffu || !(cv > -1.0f));
            const bool pass = rank == 0 ? true : ((cv > gB) && (cv > 0.f) && valid && !blocked);
            const bool stop = !pass || (rank == 0 && !valid);
            int r = (int)wave_min_u32((stop && !(rank == 0)) ? (uint32_t)rank : ((rank == 0 && !valid) ? 1u : 64u));
            r = min(min(r, left), FS_RMAX);
            if (r < 1) r = 1;
            if (rank < r) {
                const bool v0 = valid;
                const float ox = v0 ? cx : cloud[0], oy = v0 ? cy : cloud[1], oz = v0 ? cz : cloud[2];
                s_res[1 + 3 * rank] = ox; s_res[2 + 3 * rank] = oy; s_res[3 + 3 * rank] = oz;
                if (half == 0) {
                    sel[j + rank] = valid ? kc.decode(ck) : 0;
                    if (nxyz) { nxyz[3 * (j + rank)] = ox; nxyz[3 * (j + rank) + 1] = oy; nxyz[3 * (j + rank) + 2] = oz; }
                }
            }
            s_rank[i] = 0; s_blk[i] = 0;
            if (lane == 0) s_res[0] = __int_as_float(r);
        }
        lds_barrier();                                                // B
        // the round's result: r, and pivot q's coordinates into lane q (s_res is rewritten behind the NEXT round's barrier A2)
        const int r = __float_as_int(s_res[0]);
        const int q3 = 1 + 3 * min(lane, FS_RMAX - 1);
        const float ox_ = s_res[q3], oy_ = s_res[q3 + 1], oz_ = s_res[q3 + 2];
        j += r;
        const int apply_n = j >= m ? r - 1 : r;
        touched = 0ull;
        // the wave-level cull of fps_spec_kernel: lane q tests pivot q against the wave's own box, the survivors go through the tile tests
        unsigned mine = (unsigned)__ballot(lane < apply_n && wave_hit(ox_, oy_, oz_));
        while (mine != 0u) {
            const int l = __builtin_ctz(mine);
            mine &= mine - 1u;
            const float ox = fs_uniform(s_res[1 + 3 * l]), oy = fs_uniform(s_res[2 + 3 * l]), oz = fs_uniform(s_res[3 + 3 * l]);
            update(ox, oy, oz, box_mask(ox, oy, oz, lane < PPT));
        }
        ++round;
    }
    if (mind) {
#pragma unroll
        for (int i = 0; i < PPT; ++i)
            if (pc[i] != 0xffffffffu) mind[kc.decode(pc[i] >> SB)] = pt[i];
    }
}

// KB of dynamic LDS a workgroup of these kernels claims without using it (PRCNN_FPS_LDS_PAD): more than half of a CU's, so that no
// two of them share a CU
static size_t fps_lds_pad()
{
    static const size_t pad = (size_t)(getenv("PRCNN_FPS_LDS_PAD") ? atoi(getenv("PRCNN_FPS_LDS_PAD")) : 84) * 1024;
    return pad;
}

// how many fps_spec2_kernel workgroups the current device holds at once (0: it refuses the dynamic LDS); cached per device
int fps2_capacity()
{
    static std::mutex mu;
    static std::map<int, int> cache;
    const size_t pad = fps_lds_pad();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int cap = 0, per_cu = 0, cus = 0;
    if (ensure_dynamic_lds((const void *)prcnn::fps_spec2_kernel, pad, "furthest_point_sampling(two workgroups)") == PRCNN_OK &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)prcnn::fps_spec2_kernel, 1024, pad) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
        cap = per_cu * cus;
    else
        (void)hipGetLastError();
    if (const char *e = getenv("PRCNN_FPS2_CAPACITY")) cap = atoi(e);    // tests: force the chunked launches / the fallback
    cache[dev] = cap;
    return cap;
}

// 16384 < n <= 32768, fps2_capacity() >= 32 (fps_any checks both).
// the two-workgroup kernel spins on its partner: only where BOTH halves of every cloud of a launch are resident at once.  One such
// workgroup holds a CU (84 KB of LDS); a launch takes at most HALF of what the device can hold (the other geometry stream may be
// running the same kernel: per XCD at most one unpaired block per launch is resident, every other resident block has its partner
// and makes progress), larger batches go as several launches.
int launch_fps_spec2(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, float *new_xyz, hipStream_t st)
{
    // two workgroups per cloud, blocks q and q + 8 (fps_spec2_kernel): the grid is padded to whole sets of 16 blocks
    int *perm = (int *)scratch_for(st, (size_t)b * n * sizeof(int), 1);
    Fps2Table *tables = (Fps2Table *)scratch_for(st, (size_t)b * sizeof(Fps2Table), 13);
    if (!perm || !tables) { set_error("fps: cannot allocate the ordering / exchange scratch"); return PRCNN_ELAUNCH; }
    launch_fps_order(b, n, xyz, perm, nullptr, st);
    if (hipMemsetAsync(tables, 0, (size_t)b * sizeof(Fps2Table), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("fps: cannot reset the exchange tables");
        return PRCNN_ELAUNCH;
    }
    // (the placement hint of the one-workgroup kernel is REQUIRED here: with more than half of a CU's LDS per workgroup no two of
    //  these spinning workgroups share a CU, and every XCD dispatches a cloud's halves back to back)
    const int per = (fps2_capacity() / 2 / 16) * 8;                   // clouds per launch: whole sets of 16 blocks, half the capacity
    for (int off = 0; off < b; off += per) {
        const int nb = b - off < per ? b - off : per;
        const unsigned grid = (unsigned)((nb + 7) / 8) * 16u;
        hipLaunchKernelGGL(fps_spec2_kernel, dim3(grid), dim3(1024), fps_lds_pad(), st, nb, n, m, kc, xyz + (size_t)off * n * 3, perm + (size_t)off * n,
                           temp ? temp + (size_t)off * n : nullptr, idx + (size_t)off * m, new_xyz ? new_xyz + (size_t)off * m * 3 : nullptr,
                           tables + off);
    }
    return check_launch("furthest_point_sampling(two workgroups)");
}

// 2048 < n <= 16384 (fps_any checks it); rejected: clouds to leave alone (NULL: none), see fps_any
int launch_fps_spec(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, float *new_xyz, const int *rejected, hipStream_t st)
{
    int *perm = (int *)scratch_for(st, (size_t)b * n * sizeof(int), 1);
    if (!perm) { set_error("fps: cannot allocate ordering scratch"); return PRCNN_ELAUNCH; }
    launch_fps_order(b, n, xyz, perm, rejected, st);
    // Unused dynamic LDS as a placement hint: with more than half of a CU's LDS requested, two of these
    // latency-bound 1024-thread workgroups (the chains of two batches run on two streams) never share a CU.
    // (+1.2 % end to end; only when the batch is small enough that one workgroup per CU costs no concurrency)
    const size_t pad = b <= 128 ? fps_lds_pad() : 0;
    // 16 waves per cloud: 8 waves x 32 points per lane runs 4.98 ms, 4 waves x 64 points 7.7 ms (16384 -> 4096, 4.2-4.3 ms here):
    // the per-iteration update of the touched tiles parallelises over waves, the exchange does not get cheaper with fewer
    const void *ss[3] = {(const void *)fps_spec_kernel<4>, (const void *)fps_spec_kernel<8>, (const void *)fps_spec_kernel<16>};
    if (pad)
        for (const void *k : ss) {
            const int rc = ensure_dynamic_lds(k, pad, "furthest_point_sampling(speculative)");
            if (rc != PRCNN_OK) return rc;
        }
    if (n <= 4096) hipLaunchKernelGGL((fps_spec_kernel<4>), dim3(b), dim3(1024), pad, st, n, m, kc, xyz, perm, temp, idx, new_xyz, rejected);
    else if (n <= 8192) hipLaunchKernelGGL((fps_spec_kernel<8>), dim3(b), dim3(1024), pad, st, n, m, kc, xyz, perm, temp, idx, new_xyz, rejected);
    else hipLaunchKernelGGL((fps_spec_kernel<16>), dim3(b), dim3(1024), pad, st, n, m, kc, xyz, perm, temp, idx, new_xyz, rejected);
    return check_launch("furthest_point_sampling(speculative)");
}

}  // namespace prcnn
