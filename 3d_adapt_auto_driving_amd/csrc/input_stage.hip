// input_stage.hip -- the network-input stage of the KITTI loader on the device: lidar -> rectified camera frame,
// validity filter, and the 16384-point near/far random sampler
// (pointrcnn/lib/datasets/kitti_rcnn_dataset.py:249-324 get_lidar / get_valid_flag / the sampling block;
//  lib/utils/calibration.py:51-71 lidar_to_rect / rect_to_img).
//
// The reference does this per scene in numpy inside DataLoader workers; at the rate the rest of the path runs
// (~1.3 ms per scene) the host stage is the bottleneck, and the cross-domain clouds are 10x larger (~180 k raw
// points).  Here ONE workgroup per scene runs the whole stage on raw points that were uploaded as they sit in
// the .bin file:
//   1. every raw point: rect = R0 * (V2C * [p;1]), image projection with P2, validity (inside the image, depth >= 0,
//      inside PC_AREA_SCOPE), near (z < 40) / far class, and a 32-bit random key;
//   2. a random subset WITHOUT replacement of size K = the K smallest keys.  Keys are a bijection of the point index
//      (murmur3 finaliser of index ^ seed), hence distinct, so "key <= K-th smallest key" selects exactly K points;
//      the K-th smallest key is found by a 4-pass 8-bit radix select with an LDS histogram;
//   3. the reference's final np.random.shuffle = sorting the chosen indices by a second key (bitonic sort of
//      <= 16384 64-bit entries in LDS).
// Sampling rules as the reference: more valid points than npoints -> all far points (at most npoints_faraway of them,
// chosen at random) + a random subset of the near ones; fewer -> every point + random extra copies.
// Against the reference's np.random the choice is another draw of the same distribution.  Against its OWN rule the sampler
// is pinned pick for pick: given the class of every raw point and the seed, every output row is determined, and
// tests/input_stage_ref.py (numpy) is that rule's definition -- tests/test_gpu_input_stage.py compares choice, stats and out
// with it bit for bit on every branch.  What the definition fixes beyond the steps above:
//   - copies WITH replacement pick "the taken point of rank (hash mod taken) in ascending raw index": the taken points are
//     compacted in index order (ballot + prefix) on that branch, never by the arrival order of an LDS atomic;
//   - a scene in which nothing is taken (npoints_faraway = 0 and more than npoints valid points, all of them far) is an
//     empty scene: zeros, choice = -1, stats as counted;
//   - the scope test compares the f32 coordinates with the f64 PC_AREA_SCOPE in double (70.4 is not an f32), as
//     point_chains.hpp rect_valid_point and kitti_io.valid_flag do;
//   - the shuffle word sb is fmix32(high seed word ^ 0x9e3779b9), and the loader's seeds (seed + scene id) are below 2^32:
//     sb is one constant there, so the relative output order of two raw indices is the same in every scene.  Harmless
//     for the network, and the driver's dumped detections depend on it: it is part of the definition, not a defect.
// The transform and the filter ARE bitwise the reference's (round 4): flags and rectified coordinates equal what the
// reference's own numpy code produced on the fixture scenes (tests/golden g11).
#include "common.hpp"
#include "point_chains.hpp"
#include <math.h>
#include <algorithm>
#include <mutex>
#include <string.h>
#include <vector>

namespace prcnn {

constexpr int IS_THREADS = 1024;
constexpr int IS_MAX_OUT = 16384;

__device__ __forceinline__ unsigned fmix32(unsigned h)
{
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;                // a bijection on 32-bit words
}

// The scope rule: the f32 coordinates are compared with the f64 PC_AREA_SCOPE in double, as in rect_valid_point (point_chains.hpp):
// f32(70.4) > 70.4 is outside.  No f32 lies strictly between a double B and the f32 nearest to it, so for every f32 x (NaN
// included: all false)   (double)x >= B  <=>  x >= the smallest f32 that is >= B,   (double)x <= B  <=>  x <= the largest f32 that
// is <= B.  The entries round the six bounds that way on the host and the kernels compare with those six f32 thresholds: the
// per-point test IS the double comparison and costs what the f32 one did.
//
// -> DEVICE pointer to the six thresholds x0, x1, y0, y1, z0, z1 of this scope on the current device (null: set_error was called).
// A scope is uploaded once, with a blocking copy, the first time it is seen, and kept: a driver has one scope, so no call after the
// first uploads anything, and no host buffer has to outlive a call.
static const float *scope_thresholds(const double *scope)
{
    struct Slot { int device; double bounds[6]; float *dev; };
    static std::mutex mu;
    static std::vector<Slot> slots;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { set_error("input_stage: no current device"); return nullptr; }
    std::lock_guard<std::mutex> lock(mu);
    for (const Slot &s : slots)
        if (s.device == device && memcmp(s.bounds, scope, sizeof(s.bounds)) == 0) return s.dev;
    float thr[6];
    for (int k = 0; k < 6; ++k) {
        float f = (float)scope[k];                                   // nearest f32 (beyond the f32 range: +-inf)
        if ((k & 1) == 0 && (double)f < scope[k]) f = nextafterf(f, INFINITY);
        if ((k & 1) == 1 && (double)f > scope[k]) f = nextafterf(f, -INFINITY);
        thr[k] = f;
    }
    Slot s;
    s.device = device;
    memcpy(s.bounds, scope, sizeof(s.bounds));
    if (hipMalloc((void **)&s.dev, sizeof(thr)) != hipSuccess || hipMemcpy(s.dev, thr, sizeof(thr), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("input_stage: scope upload failed");
        return nullptr;
    }
    slots.push_back(s);
    return s.dev;
}

// -> class: 0 = invalid, 1 = near (z < far_depth), 2 = far; x, y, z = rectified coordinates
__device__ __forceinline__ int classify_point(const SceneCalib &cb, const LidarToRect &l2r, int lidar_frame, int image_filter,
                                              const float *__restrict__ scope, float far_depth, float px, float py, float pz,
                                              float &x, float &y, float &z)
{
    x = px; y = py; z = pz;
    if (lidar_frame) { x = l2r.row(0, px, py, pz); y = l2r.row(1, px, py, pz); z = l2r.row(2, px, py, pz); }
    bool ok = true;
    if (image_filter) ok = in_image(cb, x, y, z);
    if (scope)
        ok = ok && x >= scope[0] && x <= scope[1] && y >= scope[2] && y <= scope[3] && z >= scope[4] && z <= scope[5];
    return !ok ? 0 : (z < far_depth ? 1 : 2);
}

__device__ __forceinline__ int block_sum(int v, int *red)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int i = 0; i < IS_THREADS / 64; ++i) s += red[i];
    return s;
}

// K-th smallest key (1-based K) among the points whose class bit is set in `classes` (bit c = class c); keys are distinct.
__device__ unsigned radix_select(int n, const unsigned *__restrict__ key, const unsigned char *__restrict__ cls, int classes,
                                 int K, unsigned *hist, unsigned *bcast)
{
    unsigned prefix = 0, mask = 0;
    int remaining = K;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();
        for (int i = threadIdx.x; i < 256; i += IS_THREADS) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += IS_THREADS)
            if (((classes >> cls[i]) & 1) && (key[i] & mask) == prefix) atomicAdd(&hist[(key[i] >> shift) & 255u], 1u);
        __syncthreads();
        if (threadIdx.x == 0) {
            int cum = 0, bin = 0;
            for (; bin < 256; ++bin) {
                if (cum + (int)hist[bin] >= remaining) break;
                cum += (int)hist[bin];
            }
            bcast[0] = (unsigned)bin;
            bcast[1] = (unsigned)cum;
        }
        __syncthreads();
        prefix |= bcast[0] << shift;
        mask |= 255u << shift;
        remaining -= (int)bcast[1];
    }
    return prefix;
}

// The with-replacement branch of the sampler: the taken points into entries[0 .. have) in ASCENDING RAW INDEX, then `extra` copies
// behind them.  The copies address the taken points by position, so the position must be a function of the cloud, not the order in
// which an LDS atomic is served.  Rounds of IS_THREADS consecutive indices; within a round a ballot orders the lanes of a wave and
// red[] the waves (the trip count is block-uniform, so the barriers are).  Exactly `have` points pass the take test -- `have` is
// computed from the same counts and thresholds (keys are distinct) -- so the first `have` entries are all written and every pick
// reads a real index; have >= 1 (the caller's exit).  Copy e: the taken point of rank (hash(e) mod have); when the pool is one
// class (extra_cls), picks of the other class are re-drawn, at most 16 times; after that the last pick stands.
__device__ __forceinline__ void copies_with_replacement(int n, const unsigned *__restrict__ ky, const unsigned char *__restrict__ cl,
                                                     bool near_on, bool far_on, unsigned thr_near, unsigned thr_far, bool near_thr,
                                                     bool far_thr, int have, int extra, int extra_cls, unsigned sb, unsigned sc,
                                                     unsigned long long *entries, int *red)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += IS_THREADS) {
        const int i = i0 + t;
        bool take = false;
        if (i < n) {
            const int c = cl[i];
            if (c == 1) take = near_on && (!near_thr || ky[i] <= thr_near);
            if (c == 2) take = far_on && (!far_thr || ky[i] <= thr_far);
        }
        const unsigned long long ballot = __ballot(take);
        if (lane == 0) red[wave] = __popcll(ballot);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < IS_THREADS / 64; ++w) {
            const int cw = red[w];
            before += (w < wave) ? cw : 0;
            total += cw;
        }
        if (take)
            entries[before + __popcll(ballot & ((1ull << lane) - 1ull))] = ((unsigned long long)fmix32((unsigned)i ^ sb) << 32) | (unsigned)i;
        base += total;
        __syncthreads();      // red[] is rewritten by the next round
    }
    for (int e = t; e < extra; e += IS_THREADS) {
        unsigned h = fmix32((unsigned)e ^ sc);
        unsigned i = (unsigned)entries[h % (unsigned)have];
        for (int tries = 0; tries < 16 && extra_cls && cl[i] != extra_cls; ++tries) {
            h = fmix32(h + 0x632be5abu);
            i = (unsigned)entries[h % (unsigned)have];
        }
        entries[have + e] = ((unsigned long long)fmix32(h ^ sb ^ 0x51ed270bu) << 32) | i;
    }
}

__global__ __launch_bounds__(IS_THREADS) void input_stage_kernel(
    int n_max, int stride, int lidar_frame, int image_filter, const int *__restrict__ counts, const float *__restrict__ raw,
    const SceneCalib *__restrict__ calib, const float *__restrict__ scope, int npoints, int npad, float far_depth,
    int npoints_faraway, const unsigned long long *__restrict__ seeds, float *__restrict__ rect,
    unsigned *__restrict__ key, unsigned char *__restrict__ cls, float *__restrict__ out, int *__restrict__ stats, int *__restrict__ choice)
{
    extern __shared__ unsigned long long entries[];      // npad sort entries: (shuffle key << 32) | point index
    __shared__ unsigned hist[256];
    __shared__ unsigned bcast[2];
    __shared__ int red[IS_THREADS / 64];
    __shared__ int cursor;

    const int b = blockIdx.x, t = threadIdx.x;
    const int n = min(counts[b], n_max);
    const float *__restrict__ src = raw + (long)b * n_max * stride;
    float *__restrict__ rc = rect + (long)b * n_max * 3;
    unsigned *__restrict__ ky = key + (long)b * n_max;
    unsigned char *__restrict__ cl = cls + (long)b * n_max;
    const unsigned long long seed = seeds[b];
    const unsigned sa = fmix32((unsigned)seed), sb = fmix32((unsigned)(seed >> 32) ^ 0x9e3779b9u), sc = sa ^ 0x7f4a7c15u;
    const SceneCalib cb = calib[b];
    LidarToRect l2r;
    l2r.set(cb);

    // ---- 1. transform + filter + classify
    int n_near = 0, n_far = 0;
    for (int i = t; i < n; i += IS_THREADS) {
        const float px = src[(long)i * stride], py = src[(long)i * stride + 1], pz = src[(long)i * stride + 2];
        float x, y, z;
        const int c = classify_point(cb, l2r, lidar_frame, image_filter, scope, far_depth, px, py, pz, x, y, z);
        rc[3 * (long)i] = x; rc[3 * (long)i + 1] = y; rc[3 * (long)i + 2] = z;
        ky[i] = fmix32((unsigned)i ^ sa);
        cl[i] = (unsigned char)c;
        n_near += (c == 1);
        n_far += (c == 2);
    }
    n_near = block_sum(n_near, red);
    n_far = block_sum(n_far, red);
    const int n_valid = n_near + n_far;
    if (t == 0) { stats[3 * b] = n_valid; stats[3 * b + 1] = n_near; stats[3 * b + 2] = n_far; cursor = 0; }
    float *__restrict__ o = out + (long)b * npoints * 3;
    if (n_valid == 0) {
        for (int j = t; j < npoints * 3; j += IS_THREADS) o[j] = 0.f;
        if (choice)
            for (int j = t; j < npoints; j += IS_THREADS) choice[(long)b * npoints + j] = -1;
        return;
    }
    __syncthreads();          // rc / ky / cl written by this block are read below

    // ---- 2. who is taken.  Per class: nothing / everything / keys <= threshold.  `extra` further entries are copies.
    enum { NONE = 0, ALL = 1, THR = 2 };
    int near_mode = ALL, far_mode = ALL, extra = 0;
    unsigned thr_near = 0, thr_far = 0, thr_extra = 0;
    bool extra_distinct = false;               // extras = the `extra` smallest keys over all valid points (no replacement)
    int extra_cls = 0;                         // extras with replacement are drawn from this class (0 = any taken point)
    // how many points are taken: block-uniform, from the counts alone (a cap above npoints would ask for a negative near count)
    const int far_keep = min(min(n_far, npoints_faraway), npoints);
    const int have = n_valid > npoints ? far_keep + min(n_near, npoints - far_keep) : n_valid;
    if (n_valid > npoints) {
        if (far_keep == 0) far_mode = NONE;
        else if (far_keep < n_far) { far_mode = THR; thr_far = radix_select(n, ky, cl, 1 << 2, far_keep, hist, bcast); }
        const int need_near = npoints - far_keep;
        if (need_near == 0) near_mode = NONE;
        else if (need_near < n_near) { near_mode = THR; thr_near = radix_select(n, ky, cl, 1 << 1, need_near, hist, bcast); }
        else if (need_near > n_near) { extra = need_near - n_near; extra_cls = n_near > 0 ? 1 : 0; }   // every near point + copies
    } else {
        extra = npoints - n_valid;
        if (extra > 0 && extra <= n_valid) {
            extra_distinct = true;
            if (extra < n_valid) thr_extra = radix_select(n, ky, cl, (1 << 1) | (1 << 2), extra, hist, bcast);
            else thr_extra = 0xffffffffu;
        }
    }
    __syncthreads();
    // Nothing taken -- npoints_faraway = 0 with more than npoints valid points that are all far (no selection ran above: far_mode
    // NONE, no near point) -- is the empty scene again: zeros, choice = -1, stats as counted.  Everything below runs with
    // have >= 1, so no `%` sees a zero.
    if (have == 0) {
        for (int j = t; j < npoints * 3; j += IS_THREADS) o[j] = 0.f;
        if (choice)
            for (int j = t; j < npoints; j += IS_THREADS) choice[(long)b * npoints + j] = -1;
        return;
    }

    // ---- 3. compaction into sort entries
    for (int j = t; j < npad; j += IS_THREADS) entries[j] = ~0ull;
    __syncthreads();
    const bool with_replacement = extra > 0 && !extra_distinct;
    if (!with_replacement) {
        // the SET of entries is what matters here (the sort below orders it): slots in the order the LDS atomic serves them
        for (int i = t; i < n; i += IS_THREADS) {
            const int c = cl[i];
            if (c == 0) continue;
            const int mode = (c == 1) ? near_mode : far_mode;
            const unsigned thr = (c == 1) ? thr_near : thr_far;
            if (mode == ALL || (mode == THR && ky[i] <= thr)) {
                const int pos = atomicAdd(&cursor, 1);
                if (pos < npoints) entries[pos] = ((unsigned long long)fmix32((unsigned)i ^ sb) << 32) | (unsigned)i;
            }
            if (extra_distinct && ky[i] <= thr_extra) {
                const int pos = atomicAdd(&cursor, 1);
                if (pos < npoints) entries[pos] = ((unsigned long long)fmix32((unsigned)i ^ sc) << 32) | (unsigned)i;
            }
        }
    } else {
        copies_with_replacement(n, ky, cl, near_mode != NONE, far_mode != NONE, thr_near, thr_far, near_mode == THR,
                                far_mode == THR, have, extra, extra_cls, sb, sc, entries, red);
    }
    __syncthreads();

    // ---- 4. shuffle = sort by the random 32-bit key (ties by index)
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = t; i < npad / 2; i += IS_THREADS) {
                const int lo = ((i / j) * 2 * j) + (i % j), hi = lo + j;
                const bool up = ((lo & k) == 0);
                const unsigned long long a = entries[lo], c = entries[hi];
                if ((a > c) == up) { entries[lo] = c; entries[hi] = a; }
            }
            __syncthreads();
        }

    // ---- 5. gather
    for (int j = t; j < npoints; j += IS_THREADS) {
        const unsigned long long e = entries[j];
        // Unreachable: exactly npoints entries are written above -- `have` taken points (the thresholds are K-th smallest DISTINCT
        // keys, so a threshold passes exactly K points) plus npoints - have extras -- and ~0ull sorts behind every real entry, so
        // slots 0 .. npoints-1 are real.  tests/test_gpu_input_stage.py compares every row with the definition on every branch.
        if (e == ~0ull) { o[3 * j] = 0.f; o[3 * j + 1] = 0.f; o[3 * j + 2] = 0.f; continue; }
        const unsigned i = (unsigned)e;
        o[3 * j] = rc[3 * (long)i]; o[3 * j + 1] = rc[3 * (long)i + 1]; o[3 * j + 2] = rc[3 * (long)i + 2];
        if (choice) choice[(long)b * npoints + j] = (int)i;
    }
}

// the front half alone (get_valid_flag + lidar_to_rect as an operator): rect (b, n_max, 3), cls (b, n_max) u8
__global__ __launch_bounds__(256) void valid_flags_kernel(int n_max, int stride, int lidar_frame, int image_filter,
                                                           const int *__restrict__ counts, const float *__restrict__ raw,
                                                           const SceneCalib *__restrict__ calib, const float *__restrict__ scope,
                                                           float far_depth, float *__restrict__ rect, unsigned char *__restrict__ cls)
{
    const int b = blockIdx.y;
    const int n = min(counts[b], n_max);
    const SceneCalib cb = calib[b];
    LidarToRect l2r;
    l2r.set(cb);
    const float *__restrict__ src = raw + (long)b * n_max * stride;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_max; i += gridDim.x * blockDim.x) {
        float x = 0.f, y = 0.f, z = 0.f;
        int c = 0;
        if (i < n)
            c = classify_point(cb, l2r, lidar_frame, image_filter, scope, far_depth, src[(long)i * stride], src[(long)i * stride + 1],
                               src[(long)i * stride + 2], x, y, z);
        if (rect) { float *r = rect + ((long)b * n_max + i) * 3; r[0] = x; r[1] = y; r[2] = z; }
        cls[(long)b * n_max + i] = (unsigned char)c;
    }
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace prcnn

using namespace prcnn;

// raw (b, n_max, stride) f32 with stride 3 or 4 (x, y, z[, intensity]) as read from velodyne/*.bin (lidar_frame = 1)
// or already in the rectified camera frame (lidar_frame = 0: V2C / R0 are ignored); counts (b) i32 = points per scene;
// image_filter = 0 skips the in-image / depth test (synthetic clouds); calib (b, 35) f32 = V2C (3x4) | R0 (3x3) | P2 (3x4) |
// image height, width; scope = 6 HOST doubles x0,x1,y0,y1,z0,z1
// (PC_AREA_SCOPE, compared in double: scope_thresholds; read before the call returns) or NULL; seeds (b) u64 DEVICE.  -> out (b, npoints, 3), stats (b, 3) i32 = #valid, #near, #far,
// choice (b, npoints) i32 = raw index of every output point (optional, may be NULL; -1 for a scene in which nothing is taken:
// no valid point, or npoints_faraway = 0 with more than npoints valid points that are all far -- out is zeros there).
extern "C" int prcnn_input_stage(int b, int n_max, int stride, int lidar_frame, int image_filter, const int *counts, const float *raw,
                                 const float *calib, const double *scope_host, int npoints, float far_depth,
                                 int npoints_faraway, const unsigned long long *seeds, float *out, int *stats, int *choice,
                                 void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n_max >= 0 && (stride == 3 || stride == 4), "input_stage: bad sizes (stride 3 or 4)");
    PRCNN_REQUIRE(npoints > 0 && npoints <= IS_MAX_OUT, "input_stage: npoints=%d not in 1..%d", npoints, IS_MAX_OUT);
    PRCNN_REQUIRE(npoints_faraway >= 0, "input_stage: bad npoints_faraway");
    PRCNN_REQUIRE(sizeof(SceneCalib) == PRCNN_CALIB_ROW * sizeof(float), "input_stage: calib layout");
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(counts && calib && seeds && out && stats && (raw || n_max == 0), "input_stage: null pointer");
    hipStream_t st = (hipStream_t)stream;
    int npad = 1;
    while (npad < npoints) npad <<= 1;
    const size_t o_rect = 0;
    const size_t o_key = o_rect + up256((size_t)b * n_max * 3 * sizeof(float));
    const size_t o_cls = o_key + up256((size_t)b * n_max * sizeof(unsigned));
    const size_t need = o_cls + up256((size_t)b * n_max) + 256;
    char *base = scratch_for(st, need, 5);
    if (!base) { set_error("input_stage: cannot allocate %zu bytes of scratch", need); return PRCNN_ELAUNCH; }
    const float *scope_dev = nullptr;
    if (scope_host && !(scope_dev = scope_thresholds(scope_host))) return PRCNN_ELAUNCH;
    const size_t lds = (size_t)npad * sizeof(unsigned long long);
    {
        const int rc = ensure_dynamic_lds((const void *)input_stage_kernel, 140 * 1024, "input_stage");
        if (rc != PRCNN_OK) return rc;
    }
    hipLaunchKernelGGL(input_stage_kernel, dim3(b), dim3(IS_THREADS), lds, st, n_max, stride, lidar_frame, image_filter, counts, raw,
                       (const SceneCalib *)calib, scope_dev, npoints, npad, far_depth, npoints_faraway, seeds,
                       (float *)(base + o_rect), (unsigned *)(base + o_key), (unsigned char *)(base + o_cls), out, stats, choice);
    return check_launch("input_stage");
}


// get_valid_flag (kitti_rcnn_dataset.py:201-222) + Calibration.lidar_to_rect / rect_to_img (calibration.py:51-71) for whole
// batches: the front half of prcnn_input_stage as an operator of its own, same arguments.  -> cls (b, n_max) u8: 0 = not valid,
// 1 = valid with z < far_depth, 2 = valid beyond (rows >= counts[b]: 0); rect (b, n_max, 3) f32 rectified coordinates (may be
// NULL).  Bit-identical to the reference's numpy results (float32 np.dot = fma chains; tests/golden g11).
extern "C" int prcnn_valid_flags(int b, int n_max, int stride, int lidar_frame, int image_filter, const int *counts, const float *raw,
                                 const float *calib, const double *scope_host, float far_depth, float *rect, unsigned char *cls,
                                 void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n_max >= 0 && (stride == 3 || stride == 4), "valid_flags: bad sizes (stride 3 or 4)");
    if (b == 0 || n_max == 0) return PRCNN_OK;
    PRCNN_REQUIRE(counts && calib && raw && cls, "valid_flags: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const float *scope_dev = nullptr;
    if (scope_host && !(scope_dev = scope_thresholds(scope_host))) return PRCNN_ELAUNCH;
    const int gx = (int)std::min<long>(1024, ((long)n_max + 255) / 256);
    hipLaunchKernelGGL(valid_flags_kernel, dim3(gx, b), dim3(256), 0, st, n_max, stride, lidar_frame, image_filter, counts, raw,
                       (const SceneCalib *)calib, scope_dev, far_depth, rect, cls);
    return check_launch("valid_flags");
}
