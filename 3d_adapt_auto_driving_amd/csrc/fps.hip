// fps.hip -- furthest point sampling (K6) for gfx950.
//
// Reference behaviour restated: pointnet2_lib/pointnet2/src/sampling_gpu.cu:86-253 and
// cuda_utils.h:10-13.  The reference runs ONE block of bs = opt_n_threads(n) threads per cloud;
// thread t scans k = t, t+bs, ... keeping its first strict maximum, then a shared-memory tree
// (slot t takes slot t+s only if strictly larger, s = bs/2..1) picks the block winner.  The
// winner among equal maxima is therefore the point minimising the key
//        K(k) = ( bitrev_{log2 bs}(k mod bs) , k div bs )      (lexicographic)
// -- NOT the lowest index.  This file computes the same arg-max with that total order, so the
// launch shape is free: points live in registers (PPT per lane), the per-iteration arg-max is a
// DPP/permute wave reduction followed by one LDS exchange and ONE barrier, and small clouds get
// one wave each (no barrier at all), which is what the 100*B RoI clouds of the RCNN stage need.
// Here: the register-resident kernels, the Morton ordering, the any-n fallback and the dispatch.  The speculative kernels of large
// clouds are in fps_spec.hip, the nested-sampling check in fps_prefix.hip, what they all share in fps_common.hpp.
#include "fps_common.hpp"
#include "cell_sort.hpp"

namespace prcnn {

// Register-resident FPS: one block (WAVES waves) per cloud, PPT points per lane.
// ORDERED: the virtual block size equals the real one (bs == 64*WAVES), so a lane's points
// k = t + i*T have keys increasing with i and a strict '>' scan already keeps the smallest key.
template <int WAVES, int PPT, bool ORDERED>
__global__ __launch_bounds__(64 * WAVES) void fps_reg_kernel(
    int n, int m, KeyCodec kc, const float *__restrict__ xyz, float *__restrict__ temp,
    int *__restrict__ idx, float *__restrict__ new_xyz = nullptr, const int *__restrict__ rejected = nullptr)
{
    // temp == NULL: the running minima start at the reference caller's fill value (1e10, pointnet2_utils.py:26) and are not
    // handed back; new_xyz != NULL: the selected points' coordinates are written as well (prcnn_fps_new_xyz: the caller's
    // fill + index cast + gather launches folded into this one); rejected != NULL (prcnn_fps_new_xyz_nested): a cloud whose
    // entry is 0 passed the prefix check, which wrote its outputs -- nothing to do (one workgroup is one cloud: uniform)
    constexpr int T = 64 * WAVES;
    __shared__ unsigned long long s_best[3];
    const int b = blockIdx.x;
    if (rejected && rejected[b] == 0) return;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    float *__restrict__ mind = temp ? temp + (long)b * n : nullptr;
    int *__restrict__ sel = idx + (long)b * m;
    float *__restrict__ nxyz = new_xyz ? new_xyz + (long)b * m * 3 : nullptr;
    const int t = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);   // latency-bound dependent chain: win issue arbitration (see fps_spec_kernel)

    float px[PPT], py[PPT], pz[PPT], pt[PPT];
    uint32_t pk[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int k = t + i * T;
        if (k < n) {
            px[i] = cloud[3 * k]; py[i] = cloud[3 * k + 1]; pz[i] = cloud[3 * k + 2];
            pt[i] = mind ? mind[k] : 1e10f;
            pk[i] = kc.encode(k);
        } else {
            px[i] = py[i] = pz[i] = 0.f;
            pt[i] = -INFINITY;  // can never win: the reference's "best" starts at -1
            pk[i] = 0xffffffffu;
        }
    }
    if (WAVES > 1 && t < 3) s_best[t] = 0ull;
    if (WAVES > 1) __syncthreads();

    int old = 0;
    if (t == 0) sel[0] = 0;
    for (int j = 1; j < m; ++j) {
        float ox, oy, oz;
        if constexpr (WAVES == 1) {
            // one wave per cloud (the 800 RoI clouds of a batch): the pivot's coordinates come out of the REGISTERS that hold the
            // cloud (point k = lane + 64 i) instead of a dependent scalar load per iteration -- the memory round trip was most
            // of an iteration here (round 3: 138 -> ~50 us for 800 x (512 -> 128))
            const int pl = old & 63, pi = old >> 6;
            ox = oy = oz = 0.f;
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const float vx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px[i]), pl));
                const float vy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py[i]), pl));
                const float vz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[i]), pl));
                if (i == pi) { ox = vx; oy = vy; oz = vz; }
            }
        } else {
            ox = cloud[3 * old]; oy = cloud[3 * old + 1]; oz = cloud[3 * old + 2];
        }
        if (nxyz && t == 0) { nxyz[3 * (j - 1)] = ox; nxyz[3 * (j - 1) + 1] = oy; nxyz[3 * (j - 1) + 2] = oz; }
        float lv = -INFINITY;
        if (kc.hipcc) {
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const float d2 = fminf(fps_dist<true>(px[i], py[i], pz[i], ox, oy, oz), pt[i]);
                pt[i] = d2;
                lv = fmaxf(lv, d2);
            }
        } else {
#pragma unroll
            for (int i = 0; i < PPT; ++i) {
                const float d = sqdist3(px[i], py[i], pz[i], ox, oy, oz);
                const float d2 = fminf(d, pt[i]);  // min(d, temp[k]) of sampling_gpu.cu:134
                pt[i] = d2;
                lv = fmaxf(lv, d2);
            }
        }
        float bv = wave_max_f32(lv);
        uint32_t lk = 0xffffffffu;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const uint32_t c = pt[i] == bv ? pk[i] : 0xffffffffu;
            lk = c < lk ? c : lk;
        }
        uint32_t bkey = wave_min_u32(lk);
        if (WAVES > 1) {
            const int buf = j % 3;
            if ((t & 63) == 0) atomicMax(&s_best[buf], pack_candidate(bv, bkey));
            lds_barrier();     // orders LDS only: __syncthreads() would also drain wave 0's store of sel[j-1] every iteration
            const unsigned long long best = s_best[buf];
            if (t == 0) s_best[(j + 2) % 3] = 0ull;     // the slot of iteration j-1: every wave has read it (barrier j), next used at j+2
            unpack_candidate(best, bv, bkey);
        }
        // no candidate beat the reference's initial (-1, index 0): it would return 0
        old = (bkey == 0xffffffffu || !(bv > -1.0f)) ? 0 : kc.decode(bkey);
        old = __builtin_amdgcn_readfirstlane(old);
        if (t == 0) sel[j] = old;
        if (bv == 0.f) {
            // Every running minimum is 0: all distinct points have been picked, what is left are exact copies (a RoI that holds
            // fewer points than it is sampled to, roipool3d_kernel.cu:152-159).  The arg-max over equal values is the point
            // with the lowest tie key, point 0 -- in this and in every later iteration (min(d, 0) stays 0): the remaining
            // picks are 0 without computing them.  (`old` is already 0 here by the same rule.)
            for (int jj = j + 1 + t; jj < m; jj += T) {
                sel[jj] = 0;
                if (nxyz) { nxyz[3 * (jj - 1)] = cloud[0]; nxyz[3 * (jj - 1) + 1] = cloud[1]; nxyz[3 * (jj - 1) + 2] = cloud[2]; }
            }
            if (nxyz && t == 0) { nxyz[3 * j] = cloud[0]; nxyz[3 * j + 1] = cloud[1]; nxyz[3 * j + 2] = cloud[2]; }   // slot j is written by iteration j + 1 otherwise
            break;
        }
    }
    if (nxyz && t == 0 && m > 0) { nxyz[3 * (m - 1)] = cloud[3 * old]; nxyz[3 * (m - 1) + 1] = cloud[3 * old + 1]; nxyz[3 * (m - 1) + 2] = cloud[3 * old + 2]; }
    if (mind) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int k = t + i * T;
            if (k < n) mind[k] = pt[i];
        }
    }
}

__device__ __forceinline__ unsigned part1by1(unsigned v)   // spread the low 16 bits to even positions
{
    v &= 0xffffu;
    v = (v | (v << 8)) & 0x00ff00ffu;
    v = (v | (v << 4)) & 0x0f0f0f0fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// perm[b][s] = original index of the s-th point in Morton order of a 64 x 64 grid over the cloud's
// (x, z) bounding box.  Any permutation is valid for correctness; this one makes tiles compact.
// (Its users: the speculative kernels, fps_spec.hip -- the comment there says what a tile is -- and point_groups.hip.)
__global__ __launch_bounds__(1024) void fps_order_kernel(int n, const float *__restrict__ xyz, int *__restrict__ perm,
                                                         const int *__restrict__ rejected = nullptr)
{
    __shared__ int cnt[4096];
    __shared__ float red[4][16];
    __shared__ int wsum[16];
    const int b = blockIdx.x, t = threadIdx.x;
    if (rejected && rejected[b] == 0) return;                         // (fps_reg_kernel: the cloud's sampling is skipped, nobody reads its order)
    GlobalPoints<1024> cloud;
    cloud.load(xyz + (long)b * n * 3, n);
    RectXZ r;
    cloud.each([&](int, float x, float, float z, int &) { r.add(x, z); });
    rect_wave_reduce<1024>(r, red);
    for (int i = t; i < 4096; i += 1024) cnt[i] = 0;
    __syncthreads();
    r = rect_total<1024>(red);
    const float x0 = r.x0, z0 = r.z0;
    const float sx = r.x1 > x0 ? 64.f / (r.x1 - x0) : 0.f, sz = r.z1 > z0 ? 64.f / (r.z1 - z0) : 0.f;
    auto code_of = [&](float x, float z) {
        float fx = (x - x0) * sx, fz = (z - z0) * sz;
        fx = fx == fx ? fx : 0.f; fz = fz == fz ? fz : 0.f;            // NaN-safe
        const int cx = min(63, max(0, (int)fx)), cz = min(63, max(0, (int)fz));
        return (int)(part1by1((unsigned)cx) | (part1by1((unsigned)cz) << 1));
    };
    // 4096 counters, four per thread
    cell_sort<1024>(cloud, cnt, 4096, 4, wsum, false, code_of, [](int, int, int) {},
                    [&](int pos, int k, float, float, float) { perm[(long)b * n + pos] = k; });
}

// Any-n fallback: running minima stay in `temp` (global), one 1024-thread block per cloud.
__global__ __launch_bounds__(1024) void fps_generic_kernel(
    int n, int m, KeyCodec kc, const float *__restrict__ xyz, float *__restrict__ temp,
    int *__restrict__ idx)
{
    constexpr int WAVES = 16;
    __shared__ float s_v[2][WAVES];
    __shared__ uint32_t s_k[2][WAVES];
    const int b = blockIdx.x;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    float *__restrict__ mind = temp + (long)b * n;
    int *__restrict__ sel = idx + (long)b * m;
    const int t = threadIdx.x;
    int old = 0;
    if (t == 0) sel[0] = 0;
    for (int j = 1; j < m; ++j) {
        const float ox = cloud[3 * old], oy = cloud[3 * old + 1], oz = cloud[3 * old + 2];
        float bv = -1.0f;
        uint32_t bkey = 0xffffffffu;
        for (int k = t; k < n; k += 1024) {
            const float d = kc.hipcc ? fps_dist<true>(cloud[3 * k], cloud[3 * k + 1], cloud[3 * k + 2], ox, oy, oz)
                                     : sqdist3(cloud[3 * k], cloud[3 * k + 1], cloud[3 * k + 2], ox, oy, oz);
            const float d2 = fminf(d, mind[k]);
            mind[k] = d2;
            take_if_better(d2, kc.encode(k), bv, bkey);
        }
        wave_argmax(bv, bkey);
        const int buf = j & 1;
        if ((t & 63) == 0) { s_v[buf][t >> 6] = bv; s_k[buf][t >> 6] = bkey; }
        __syncthreads();
        bv = s_v[buf][t & 15];
        bkey = s_k[buf][t & 15];
        row16_argmax(bv, bkey);
        old = (bkey == 0xffffffffu) ? 0 : kc.decode(bkey);
        old = __builtin_amdgcn_readfirstlane(old);
        if (t == 0) sel[j] = old;
    }
}

static int host_opt_n_threads(int work_size)
{
    // cuda_utils.h:10-13 (double log ratio truncated, clamped to [1, 1024])
    const int pow_2 = (int)(log((double)work_size) / log(2.0));
    int t = 1 << pow_2;
    if (t > 1024) t = 1024;
    if (t < 1) t = 1;
    return t;
}

template <int WAVES, int PPT>
static void launch_reg(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, hipStream_t st, float *new_xyz = nullptr,
                       const int *rejected = nullptr)
{
    if ((1 << kc.log2bs) == 64 * WAVES)
        hipLaunchKernelGGL((fps_reg_kernel<WAVES, PPT, true>), dim3(b), dim3(64 * WAVES), 0, st, n, m, kc, xyz, temp, idx, new_xyz, rejected);
    else
        hipLaunchKernelGGL((fps_reg_kernel<WAVES, PPT, false>), dim3(b), dim3(64 * WAVES), 0, st, n, m, kc, xyz, temp, idx, new_xyz, rejected);
}

// 0 (default): the distance of sampling_gpu.cu:133 with one rounding per source operation (the parity contract: what the source says,
// whatever a compiler contracts); 1: the arithmetic of the reference's kernel binary as hipcc builds it for gfx950
// ((fma(dy, dy, dx*dx)) + dz*dz: see fps_dist).  Process-wide, read at launch; applies to every FPS entry point of the library.
static int g_fps_hipcc = 0;

__global__ __launch_bounds__(256) void fps_fill_kernel(long count, float v, float *__restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = v;
}
__global__ __launch_bounds__(256) void fps_gather_xyz_kernel(int n, int m, const float *__restrict__ xyz, const int *__restrict__ idx,
                                                             float *__restrict__ new_xyz)
{
    const int chunks = (m + 255) / 256;
    const int b = blockIdx.x / chunks, j = (blockIdx.x % chunks) * 256 + threadIdx.x;
    if (j >= m) return;
    const float *p = xyz + ((long)b * n + idx[(long)b * m + j]) * 3;
    float *o = new_xyz + ((long)b * m + j) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// The tie-key layout of a cloud of n points: the reference's block size opt_n_threads(n) and the bits of k div bs above it
int fps_codec(int n, KeyCodec *kc)
{
    const int bs = host_opt_n_threads(n);
    kc->hipcc = g_fps_hipcc;
    kc->log2bs = 0;
    while ((1 << kc->log2bs) < bs) ++kc->log2bs;
    const int nq = (n + bs - 1) / bs;  // values of k div bs: 0 .. nq-1
    kc->sh = 0;
    while ((1 << kc->sh) < nq) ++kc->sh;
    PRCNN_REQUIRE(kc->sh + kc->log2bs <= 31, "fps: n=%d too large for the 32-bit tie key", n);
    return PRCNN_OK;
}

void launch_fps_order(int b, int n, const float *xyz, int *perm, const int *rejected, hipStream_t st)
{
    hipLaunchKernelGGL(fps_order_kernel, dim3(b), dim3(1024), 0, st, n, xyz, perm, rejected);
}

// n <= 1024: one wave per cloud, the whole cloud in its registers; few clouds of more than 512 points: four waves each
static void launch_reg_small(int b, int n, int m, KeyCodec kc, const float *xyz, float *temp, int *idx, float *new_xyz, const int *rejected,
                             hipStream_t st)
{
    if (n <= 128) launch_reg<1, 2>(b, n, m, kc, xyz, temp, idx, st, new_xyz, rejected);
    else if (n <= 256) launch_reg<1, 4>(b, n, m, kc, xyz, temp, idx, st, new_xyz, rejected);
    else if (n <= 512) launch_reg<1, 8>(b, n, m, kc, xyz, temp, idx, st, new_xyz, rejected);
    else if (b >= 128) launch_reg<1, 16>(b, n, m, kc, xyz, temp, idx, st, new_xyz, rejected);
    else launch_reg<4, 4>(b, n, m, kc, xyz, temp, idx, st, new_xyz, rejected);
}

// new_xyz != NULL (prcnn_fps_new_xyz; temp may then be NULL): the speculative kernel (2048 < n <= 16384, m >= 256) writes the
// coordinates itself; every other route (few samples, small clouds, n > 32768 or a device that cannot hold the two-workgroup kernel) runs its kernel over an
// internal distance scratch filled with the reference caller's 1e10 and gathers the coordinates behind it -- same indices, same
// coordinates, two small launches more (round 5; ADVICE r4: those routes used to refuse)
// rejected != NULL (prcnn_fps_new_xyz_nested, n <= 16384): per cloud, 0 = the prefix check accepted it and wrote its outputs, the
// sampling kernels leave it alone.  Every other caller passes NULL: same launches, same code path as before the check existed.
static int fps_any(int b, int n, int m, const float *xyz, float *temp, int *idx, float *new_xyz, void *stream, const int *rejected = nullptr)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && m >= 0, "fps: bad sizes b=%d n=%d m=%d", b, n, m);
    if (b == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(n > 0, "fps: empty cloud with m=%d", m);
    PRCNN_REQUIRE(xyz && (temp || new_xyz) && idx, "fps: null pointer");
    hipStream_t st = (hipStream_t)stream;
    PRCNN_REQUIRE(!rejected || n <= 16384, "fps: the skip flags serve n <= 16384 (n=%d)", n);   // never the two-workgroup kernel and its spin

    KeyCodec kc;
    if (const int rc = fps_codec(n, &kc)) return rc;

    // large clouds: Morton ordering + pruned scan (exact; fps_spec.hip).  It needs (n ints) of scratch per scene and pays
    // off when the sample count is large enough for the pruning radius to shrink.
    // A device that refuses the two-workgroup kernel's LDS (64 KB parts) or has fewer than 32 slots for it keeps fps_generic_kernel
    const bool spec_shape = n > 2048 && n <= 16384 && m >= 256;
    const bool pair_ok = n > 16384 && n <= 32768 && m >= 256 && fps2_capacity() >= 32;
    if (new_xyz && !(spec_shape || pair_ok)) {
        if (!temp) {
            temp = (float *)scratch_for(st, (size_t)b * n * sizeof(float), 12);
            if (!temp) { set_error("fps_new_xyz: cannot allocate the distance scratch"); return PRCNN_ELAUNCH; }
            hipLaunchKernelGGL(fps_fill_kernel, dim3((unsigned)(((long)b * n + 255) / 256)), dim3(256), 0, st, (long)b * n, 1e10f, temp);
        }
        const int rc = fps_any(b, n, m, xyz, temp, idx, nullptr, stream, rejected);
        if (rc != PRCNN_OK) return rc;                                // (the gather serves an accepted cloud too: its idx is 0 .. m-1)
        hipLaunchKernelGGL(fps_gather_xyz_kernel, dim3((unsigned)((long)((m + 255) / 256) * b)), dim3(256), 0, st, n, m, xyz, idx, new_xyz);
        return check_launch("fps_new_xyz(gather)");
    }
    if (pair_ok) return launch_fps_spec2(b, n, m, kc, xyz, temp, idx, new_xyz, st);
    if (spec_shape) return launch_fps_spec(b, n, m, kc, xyz, temp, idx, new_xyz, rejected, st);
    if (n <= 1024) launch_reg_small(b, n, m, kc, xyz, temp, idx, nullptr, rejected, st);
    else if (n <= 4096) launch_reg<16, 4>(b, n, m, kc, xyz, temp, idx, st, nullptr, rejected);
    else if (n <= 8192) launch_reg<16, 8>(b, n, m, kc, xyz, temp, idx, st, nullptr, rejected);
    else if (n <= 16384) launch_reg<16, 16>(b, n, m, kc, xyz, temp, idx, st, nullptr, rejected);
    else hipLaunchKernelGGL(fps_generic_kernel, dim3(b), dim3(1024), 0, st, n, m, kc, xyz, temp, idx);
    return check_launch("furthest_point_sampling");
}

// FPS of many small clouds (n <= 1024: one wave per cloud, everything in registers) with the selected coordinates written
// alongside the indices: what furthest_point_sample + gather_operation (pointnet2_modules.py:40-46) produce, without the
// caller's 1e10 fill of the distance scratch, the index cast and the gather launch.  idx (b,m), new_xyz (b,m,3).
int fps_new_xyz_any(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream, const int *rejected)
{
    if (n > 1024) return fps_any(b, n, m, xyz, nullptr, idx, new_xyz, stream, rejected);      // round 4: the speculative kernel writes them too
    KeyCodec kc;
    if (const int rc = fps_codec(n, &kc)) return rc;
    launch_reg_small(b, n, m, kc, xyz, nullptr, idx, new_xyz, rejected, (hipStream_t)stream);   // (as prcnn_furthest_point_sampling)
    return check_launch("fps_new_xyz");
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_opt_n_threads(int work_size) { return work_size > 0 ? host_opt_n_threads(work_size) : 1; }

// selects the arithmetic of every FPS entry point of the library (g_fps_hipcc above)
extern "C" int prcnn_set_fps_arithmetic(int mode)
{
    PRCNN_REQUIRE(mode == 0 || mode == 1, "set_fps_arithmetic: mode %d", mode);
    g_fps_hipcc = mode;
    return PRCNN_OK;
}

extern "C" int prcnn_furthest_point_sampling(int b, int n, int m, const float *xyz, float *temp,
                                             int *idx, void *stream)
{
    PRCNN_REQUIRE(temp || b == 0 || m == 0, "fps: null pointer");
    return fps_any(b, n, m, xyz, temp, idx, nullptr, stream);
}

extern "C" int prcnn_fps_new_xyz(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n > 0 && m >= 0, "fps_new_xyz: b=%d n=%d m=%d", b, n, m);
    if (b == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && idx && new_xyz, "fps_new_xyz: null pointer");
    return fps_new_xyz_any(b, n, m, xyz, idx, new_xyz, stream, nullptr);
}
