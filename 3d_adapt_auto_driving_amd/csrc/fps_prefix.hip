// fps_prefix.hip -- nested furthest point sampling: where the answer is the prefix 0 .. m-1 it is checked in parallel instead of sampled.
#include "fps_common.hpp"

namespace prcnn {
// ---- nested sampling: is the answer the prefix?  (prcnn_fps_new_xyz_nested) ------------------------------------------------
// The RPN backbone samples 16384 -> 4096 -> 1024 -> 256 -> 64, every level from the previous level's new_xyz: the previous picks in
// pick order.  FPS is a greedy arg-max, so it is prefix-consistent: pick s of the outer run is the arg-max of the running minima over
// the whole outer cloud, it lies in the inner cloud P[0..n) (the first n picks), so it is the arg-max over P as well -- computed from
// the same coordinates, the same fps_dist and the same pivots in the same order.  By induction the inner run picks 0, 1, ..., m-1.
// The one way this fails is an exact tie at a maximum: the tie key depends on n and on a point's position, so the inner run may break
// a tie differently (an integer lattice does).  Whether a cloud's answer IS the prefix has no dependent chain and is checked in
// parallel, n * m distance evaluations.  With T_s[j] = min(1e10, min_{i < s} fps_dist(P[j], P[i])) and D[s] = T_s[s] the sampling
// kernels pick s at step s, for every s in 1 .. m-1, if and only if
//     D[s] > 0                                                       (beats the picked points and their copies, T = 0, and the -1 start)
//     for every j > s:  D[s] > T_s[j],  or  D[s] == T_s[j] and encode(s) < encode(j)     (the kernels' total order: better())
// -- every condition a positive comparison, and every coordinate finite, so a NaN or an infinity rejects.  An accepted cloud's
// outputs are idx = 0 .. m-1 and new_xyz = P[0..m): fps_prefix_pivots_kernel writes them for EVERY cloud, the sampling kernels skip
// the accepted clouds and overwrite the rejected ones.  Two launches:
//   fps_prefix_pivots_kernel   D[s] into scratch: a workgroup per 64 pivots, its four waves split the i < s range, pivots from LDS
//   fps_prefix_check_kernel    a thread per point j walks s = 1 .. min(j, m) - 1 with its running minimum against D[s]; pivots and
//                              D staged in LDS 256 at a time; a workgroup leaves as soon as the cloud is known to be rejected
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int FPX_T = 256;                                            // threads of both kernels = pivots staged per pass

template <bool HIPCC>
__global__ __launch_bounds__(FPX_T) void fps_prefix_pivots_kernel(int n, int m, const float *__restrict__ xyz, float *__restrict__ dpiv,
                                                                  int *__restrict__ rejected, int *__restrict__ idx, float *__restrict__ new_xyz)
{
    __shared__ float s_p[FPX_T][3];
    __shared__ float s_part[4][64];
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    if (blockIdx.x == 0 && t == 0) rejected[b] = 0;                   // the flag's reset, on-stream in front of the check
    const int s = blockIdx.x * 64 + lane;                             // this lane's pivot (the four waves hold the same 64)
    const int sc = min(s, m - 1);
    const float x = cloud[3 * sc], y = cloud[3 * sc + 1], z = cloud[3 * sc + 2];
    const int iend = min(blockIdx.x * 64 + 63, m - 1);                // i < s <= iend
    float d = 1e10f;                                                  // the reference caller's fill value (pointnet2_utils.py:26)
    for (int i0 = 0; i0 < iend; i0 += FPX_T) {
        __syncthreads();
        if (i0 + t < iend) { s_p[t][0] = cloud[3 * (i0 + t)]; s_p[t][1] = cloud[3 * (i0 + t) + 1]; s_p[t][2] = cloud[3 * (i0 + t) + 2]; }
        __syncthreads();
        const int k1 = min(64, iend - i0 - 64 * w);
#pragma unroll 4
        for (int k = 0; k < k1; ++k) {
            const int q = 64 * w + k;
            const float e = fps_dist<HIPCC>(x, y, z, s_p[q][0], s_p[q][1], s_p[q][2]);
            d = (i0 + q < s) ? fminf(e, d) : d;                       // min(d, temp[k]) of sampling_gpu.cu:134
        }
    }
    s_part[w][lane] = d;
    __syncthreads();
    if (w == 0 && s < m) {
        dpiv[(long)b * m + s] = fminf(fminf(s_part[0][lane], s_part[1][lane]), fminf(s_part[2][lane], s_part[3][lane]));
        if (idx) idx[(long)b * m + s] = s;
        if (new_xyz) { float *o = new_xyz + ((long)b * m + s) * 3; o[0] = x; o[1] = y; o[2] = z; }
    }
}

template <bool HIPCC>
__global__ __launch_bounds__(FPX_T) void fps_prefix_check_kernel(int n, int m, KeyCodec kc, const float *__restrict__ xyz,
                                                                 const float *__restrict__ dpiv, int *__restrict__ rejected)
{
    __shared__ float4 s_p[FPX_T];                                     // (P[i], D[i + 1]): step s = i + 1 compares D[s] with the minimum over i < s
    const int b = blockIdx.y, t = threadIdx.x;
    const float *__restrict__ cloud = xyz + (long)b * n * 3;
    const float *__restrict__ D = dpiv + (long)b * m;
    const int j = blockIdx.x * FPX_T + t, jc = min(j, n - 1);         // (a thread beyond the cloud repeats point n-1: same verdict)
    const float x = cloud[3 * jc], y = cloud[3 * jc + 1], z = cloud[3 * jc + 2];
    const uint32_t kj = kc.encode(jc);
    bool ok = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
    if (jc >= 1 && jc < m) ok &= D[jc] > 0.f;
    const int jmax = min(n, (int)(blockIdx.x + 1) * FPX_T) - 1;       // the block's last point: steps s <= min(m, jmax) - 1
    const int iend = min(m, jmax) - 1;                                // pivots i = s - 1 < iend
    float r = 1e10f;
    for (int i0 = 0; ; i0 += FPX_T) {
        // uniform exit: somebody (this workgroup or another one of the cloud) has rejected -- or the walk is over
        const int seen = __hip_atomic_load(rejected + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__syncthreads_or(!ok || seen != 0) || i0 >= iend) break;
        if (i0 + t < iend) {
            const int i = i0 + t;
            s_p[t] = make_float4(cloud[3 * i], cloud[3 * i + 1], cloud[3 * i + 2], D[i + 1]);
        }
        __syncthreads();
        const int k1 = min(FPX_T, iend - i0);
#pragma unroll 4
        for (int k = 0; k < k1; ++k) {
            const float4 p = s_p[k];
            const int s = i0 + k + 1;
            r = fminf(fps_dist<HIPCC>(x, y, z, p.x, p.y, p.z), r);
            bool win = p.w > r;
            if (p.w == r) win = kc.encode(s) < kj;                    // an exact tie (rare): the kernels' key order decides
            ok = ok && (win || s >= jc);
        }
    }
    if (!ok) rejected[b] = 1;
}
}  // namespace prcnn

using namespace prcnn;

// the shapes the check serves (everything else goes to prcnn_fps_new_xyz as it is): a pick to decide, the sampling kernels that take the flag
extern "C" int prcnn_fps_nested_supported(int n, int m) { return m >= 2 && m <= n && n <= 16384; }

static int fps_prefix_any(int b, int n, int m, const KeyCodec &kc, const float *xyz, int *idx, float *new_xyz, float *dpiv, int *rejected,
                          hipStream_t st)
{
    const dim3 g1((unsigned)((m + 63) / 64), (unsigned)b), g2((unsigned)((n + FPX_T - 1) / FPX_T), (unsigned)b);
    if (kc.hipcc) {
        hipLaunchKernelGGL(fps_prefix_pivots_kernel<true>, g1, dim3(FPX_T), 0, st, n, m, xyz, dpiv, rejected, idx, new_xyz);
        hipLaunchKernelGGL(fps_prefix_check_kernel<true>, g2, dim3(FPX_T), 0, st, n, m, kc, xyz, dpiv, rejected);
    } else {
        hipLaunchKernelGGL(fps_prefix_pivots_kernel<false>, g1, dim3(FPX_T), 0, st, n, m, xyz, dpiv, rejected, idx, new_xyz);
        hipLaunchKernelGGL(fps_prefix_check_kernel<false>, g2, dim3(FPX_T), 0, st, n, m, kc, xyz, dpiv, rejected);
    }
    return check_launch("fps_prefix_check");
}

// The check alone (tests, profiles/fps_nested_probe.py: the acceptance rate): rejected (b) <- 0 where sampling m of the cloud's n points
// returns 0 .. m-1, 1 where it may not; idx / new_xyz (NULL: not wanted) <- the prefix, for every cloud.
extern "C" int prcnn_fps_prefix_check(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, int *rejected, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && b <= 65535 && prcnn_fps_nested_supported(n, m), "fps_prefix_check: b=%d n=%d m=%d", b, n, m);
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && rejected, "fps_prefix_check: null pointer");
    hipStream_t st = (hipStream_t)stream;
    KeyCodec kc;
    if (const int rc = fps_codec(n, &kc)) return rc;
    float *dpiv = (float *)scratch_for(st, (size_t)b * m * sizeof(float), 15);
    if (!dpiv) { set_error("fps_prefix_check: cannot allocate the pivot scratch"); return PRCNN_ELAUNCH; }
    return fps_prefix_any(b, n, m, kc, xyz, idx, new_xyz, dpiv, rejected, st);
}

// The sampling launches of prcnn_fps_new_xyz_nested WITHOUT its check, under a verdict the caller made up (tests: a cloud whose entry
// is 0 must come back untouched, whatever it holds; one whose entry is not 0 sampled as by prcnn_fps_new_xyz).  rejected (b) on the device.
extern "C" int prcnn_fps_new_xyz_flagged(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, const int *rejected, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && prcnn_fps_nested_supported(n, m), "fps_new_xyz_flagged: b=%d n=%d m=%d", b, n, m);
    if (b == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && idx && new_xyz && rejected, "fps_new_xyz_flagged: null pointer");
    return fps_new_xyz_any(b, n, m, xyz, idx, new_xyz, stream, rejected);
}

// prcnn_fps_new_xyz for a caller that EXPECTS the prefix (xyz is an earlier sampling's new_xyz): same outputs for any input -- the
// check decides per cloud, the hint only says that running it is worth its n * m evaluations.  No allocation or host synchronisation
// once the stream's scratch exists: capturable like the plain entry.
extern "C" int prcnn_fps_new_xyz_nested(int b, int n, int m, const float *xyz, int *idx, float *new_xyz, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n > 0 && m >= 0, "fps_new_xyz_nested: b=%d n=%d m=%d", b, n, m);
    if (b == 0 || m == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && idx && new_xyz, "fps_new_xyz_nested: null pointer");
    if (!prcnn_fps_nested_supported(n, m) || b > 65535) return fps_new_xyz_any(b, n, m, xyz, idx, new_xyz, stream, nullptr);
    hipStream_t st = (hipStream_t)stream;
    KeyCodec kc;
    if (const int rc = fps_codec(n, &kc)) return rc;
    float *dpiv = (float *)scratch_for(st, ((size_t)b * m + (size_t)b) * sizeof(float), 15);     // D (b, m), then the flags (b)
    if (!dpiv) { set_error("fps_new_xyz_nested: cannot allocate the check's scratch"); return PRCNN_ELAUNCH; }
    int *rejected = (int *)(dpiv + (size_t)b * m);
    if (const int rc = fps_prefix_any(b, n, m, kc, xyz, idx, new_xyz, dpiv, rejected, st)) return rc;
    return fps_new_xyz_any(b, n, m, xyz, idx, new_xyz, stream, rejected);
}
