// train_layer.hip -- the order-fixed TRAINING layer for gfx950: forward and backward of a 1x1 convolution, BatchNorm on batch
// statistics and ReLU (pytorch_utils.Conv1d / Conv2d in training mode).  include/prcnn_hip.h states the
// arithmetic contract; this comment says how the kernels meet it.
//
// Tensors stay in torch's layout: x (B, Cin, P), w (Cout, Cin), z / y / dz (B, Cout, P).  A cloud's positions are cut into chunks of
// PRCNN_TRAIN_CHUNK; every reduction over positions is "inside a chunk in a fixed tree, then the chunks left to right", so its shape
// depends on (B, Cin, Cout, P) and the constants below alone -- never on the grid, the CU count or an arrival order.  No atomics.
//
//   tl_gemm_kernel    out[b] = A . X[b] on v_mfma_f32_32x32x2_f32: forward (A = w) and dx (A = w transposed, X = dz).  A workgroup
//                     (4 waves) owns ONE chunk of one cloud and 32 * MT output rows; a wave owns 32 of the 128 positions of a
//                     sub-tile.  The B operand is x[b, k, p0 + lane % 32], a coalesced row straight from global memory; the weight
//                     tile is staged in LDS, zero-padded past M and K.  k runs ascending: an element is the fmaf chain over ci = 0,
//                     1, ... from +0.0f (a padded term adds fma(0, 0, acc) = acc).  Epilogues: plain store, bias (+ ReLU) store,
//                     or store z and add it to per-lane f64 sums of z and z * z, reduced once per chunk.
//   tl_bn_finish      one workgroup: partials in (cloud, chunk) order -> mean, rstd (f64) and the running statistics.
//   tl_bn_apply       y = max(gamma (z - mean) rstd + beta, 0) per element in f64.
//   tl_bwd_partials   g = dy where the recomputed pre-activation is > 0; f64 chunk partials of sum g and sum g zhat.
//   tl_bwd_finish     partials in order -> s1, s2 (f64), dbeta / dbias and dgamma.
//   tl_bn_dz          dz = gamma rstd (g - s1 / n - zhat s2 / n) per element in f64.
//   tl_dw_kernel      one f32 partial (Cout, Cin) per chunk: MFMA whose k dimension is the position, both operands transposed
//                     through LDS; k ascending inside the chunk.
//   tl_dw_reduce      the partials in (cloud, chunk) order in f64, rounded once.
#include "common.hpp"
#include <limits.h>

namespace prcnn {

constexpr int TL_CHUNK = PRCNN_TRAIN_CHUNK;
constexpr int TL_PT = 128;        // positions of a sub-tile: 4 waves x 32 columns
constexpr int TL_KT = 32;         // k of one LDS stage
constexpr int TL_SUBS = TL_CHUNK / TL_PT;
static_assert(TL_CHUNK % TL_PT == 0 && TL_CHUNK % 256 == 0 && TL_CHUNK % TL_KT == 0, "a chunk is whole sub-tiles, whole stages, whole rounds of 256 threads");

enum { TL_EPI_PLAIN = 0, TL_EPI_BIAS = 1, TL_EPI_STATS = 2 };

// accumulator register v of lane `lane` is row 8 * (v / 4) + 4 * (lane / 32) + v % 4, column lane % 32
__device__ __forceinline__ int tl_acc_row(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }

// the sum over the 32 lanes of a half-wave (W = 32) or the 64 of a wave, as a fixed xor tree: distance 1, 2, 4, ...
template <int W>
__device__ __forceinline__ double tl_tree_sum(double s)
{
#pragma unroll
    for (int d = 1; d < W; d <<= 1) s += __shfl_xor(s, d);
    return s;
}

// zhat and the pre-activation of the BatchNorm block, in f64 from the f32 z: forward and backward share it, so they share the mask
__device__ __forceinline__ double tl_zhat(float z, double mean, double rstd) { return ((double)z - mean) * rstd; }
__device__ __forceinline__ double tl_preact(double zhat, float gamma, float beta) { return zhat * (double)gamma + (double)beta; }

// out (B, M, P)[b][m][p] = sum over k of A(m, k) * X (B, K, P)[b][k][p], A(m, k) = a[m * K + k] (TRANS = false) or a[k * M + m].
// grid (chunks of a cloud, ceil(M / (32 MT)), B); 256 threads.
template <int MT, int EPI, bool TRANS>
__global__ __launch_bounds__(256) void tl_gemm_kernel(int M, int K, int P, int nchunk, const float *__restrict__ a, const float *__restrict__ X,
                                                      const float *__restrict__ bias, int relu, float *__restrict__ out,
                                                      double *__restrict__ part)
{
    __shared__ float wt[MT * 32][TL_KT + 1];
    __shared__ double red[EPI == TL_EPI_STATS ? 4 : 1][MT * 32][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = blockIdx.x, m0 = blockIdx.y * (MT * 32), b = blockIdx.z;
    const float *xb = X + (long)b * K * P;
    float *ob = out + (long)b * M * P;
    const int nks = (K + TL_KT - 1) / TL_KT;
    double s1[EPI == TL_EPI_STATS ? MT : 1][16], s2[EPI == TL_EPI_STATS ? MT : 1][16];
    if (EPI == TL_EPI_STATS) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 16; ++v) s1[mt][v] = s2[mt][v] = 0.0;
    }
    for (int sub = 0; sub < TL_SUBS; ++sub) {
        const long pbase = (long)chunk * TL_CHUNK + sub * TL_PT;
        if (pbase >= P) break;                                   // workgroup-uniform
        const long p = pbase + wave * 32 + (lane & 31);
        const bool pin = p < P;
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[mt][v] = 0.0f;
        for (int ks = 0; ks < nks; ++ks) {
            const int k0 = ks * TL_KT;
            if (nks > 1 || sub == 0) {                           // a weight panel of one stage is staged once per workgroup
                __syncthreads();
                for (int i = t; i < MT * 32 * TL_KT; i += 256) {
                    const int r = TRANS ? i % (MT * 32) : i / TL_KT, kk = TRANS ? i / (MT * 32) : i % TL_KT;
                    const int m = m0 + r, k = k0 + kk;
                    wt[r][kk] = (m < M && k < K) ? (TRANS ? a[(long)k * M + m] : a[(long)m * K + k]) : 0.0f;
                }
                __syncthreads();
            }
            float bv[TL_KT / 2];
#pragma unroll
            for (int j = 0; j < TL_KT / 2; ++j) {
                const int k = k0 + 2 * j + (lane >> 5);
                bv[j] = (pin && k < K) ? xb[(long)k * P + p] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < TL_KT / 2; ++j)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[mt * 32 + (lane & 31)][2 * j + (lane >> 5)], bv[j], acc[mt], 0, 0, 0);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + mt * 32 + tl_acc_row(v, lane);
                float val = acc[mt][v];
                if (EPI == TL_EPI_STATS) {                       // (a position or a row out of range holds an exact zero)
                    s1[mt][v] += (double)val;
                    s2[mt][v] += (double)val * (double)val;
                }
                if (m < M && pin) {
                    if (EPI == TL_EPI_BIAS) {
                        if (bias) val = __fadd_rn(val, bias[m]);
                        if (relu) val = fmaxf(val, 0.0f);
                    }
                    ob[(long)m * P + p] = val;
                }
            }
    }
    if (EPI == TL_EPI_STATS) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const double a1 = tl_tree_sum<32>(s1[mt][v]), a2 = tl_tree_sum<32>(s2[mt][v]);
                if ((lane & 31) == 0) {
                    red[wave][mt * 32 + tl_acc_row(v, lane)][0] = a1;
                    red[wave][mt * 32 + tl_acc_row(v, lane)][1] = a2;
                }
            }
        __syncthreads();
        if (t < MT * 32 && m0 + t < M) {
            double *pp = part + ((long)b * nchunk + chunk) * 2 * M;
            pp[m0 + t] = ((red[0][t][0] + red[1][t][0]) + red[2][t][0]) + red[3][t][0];
            pp[M + m0 + t] = ((red[0][t][1] + red[1][t][1]) + red[2][t][1]) + red[3][t][1];
        }
    }
}

// One workgroup.  part (nparts, 2, c) f64 in (cloud, chunk) order -> stats (2, c): mean, rstd; the running statistics in place.
__global__ __launch_bounds__(256) void tl_bn_finish_kernel(int c, long nparts, double n, const double *__restrict__ part, double eps, double mom,
                                                           float *__restrict__ rmean, float *__restrict__ rvar, double *__restrict__ stats)
{
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        double S1 = 0.0, S2 = 0.0;
        for (long i = 0; i < nparts; ++i) {
            S1 += part[i * 2 * c + ch];
            S2 += part[(i * 2 + 1) * c + ch];
        }
        const double mean = S1 / n;
        const double var = fmax(S2 / n - mean * mean, 0.0);
        stats[ch] = mean;
        stats[c + ch] = 1.0 / sqrt(var + eps);
        if (rmean) rmean[ch] = (float)((1.0 - mom) * (double)rmean[ch] + mom * mean);
        if (rvar) rvar[ch] = (float)((1.0 - mom) * (double)rvar[ch] + mom * (var * n / (n - 1.0)));
    }
}

// grid (B * c rows, chunks); a thread takes positions chunk0 + t + 256 j
__global__ __launch_bounds__(256) void tl_bn_apply_kernel(int c, int P, int relu, const float *__restrict__ z, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const double *__restrict__ stats, float *__restrict__ y)
{
    const long row = blockIdx.x;
    const int ch = (int)(row % c);
    const double mean = stats[ch], rstd = stats[c + ch];
    const float ga = gamma[ch], be = beta[ch];
#pragma unroll
    for (int j = 0; j < TL_CHUNK / 256; ++j) {
        const long p = (long)blockIdx.y * TL_CHUNK + j * 256 + threadIdx.x;
        if (p < P) {
            const double pre = tl_preact(tl_zhat(z[row * P + p], mean, rstd), ga, be);
            y[row * P + p] = (float)(relu ? fmax(pre, 0.0) : pre);
        }
    }
}

// Chunk partials of the backward's two sums.  BN: zy = z, g = dy where pre > 0, s1 += g, s2 += g zhat.  No BN: zy = y (read only with
// relu), g = dy where y > 0, s1 += g, and g is written to gout where that is not NULL.  Order inside a chunk: a thread adds its
// positions t, t + 256, ... left to right, the 64 lanes of a wave in the xor tree, the four waves left to right.
template <bool BN>
__global__ __launch_bounds__(256) void tl_bwd_partials_kernel(int c, int P, int nchunk, int relu, const float *__restrict__ dy,
                                                              const float *__restrict__ zy, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, const double *__restrict__ stats,
                                                              float *__restrict__ gout, double *__restrict__ part)
{
    __shared__ double red[4][2];
    const long row = blockIdx.x;
    const int ch = (int)(row % c), b = (int)(row / c), chunk = blockIdx.y, t = threadIdx.x;
    const double mean = BN ? stats[ch] : 0.0, rstd = BN ? stats[c + ch] : 0.0;
    const float ga = BN ? gamma[ch] : 0.0f, be = BN ? beta[ch] : 0.0f;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < TL_CHUNK / 256; ++j) {
        const long p = (long)chunk * TL_CHUNK + j * 256 + t;
        if (p < P) {
            float g = dy[row * P + p];
            if (BN) {
                const double zh = tl_zhat(zy[row * P + p], mean, rstd);
                if (relu && !(tl_preact(zh, ga, be) > 0.0)) g = 0.0f;
                s2 += (double)g * zh;
            } else {
                if (relu && !(zy[row * P + p] > 0.0f)) g = 0.0f;
                if (gout) gout[row * P + p] = g;
            }
            s1 += (double)g;
        }
    }
    s1 = tl_tree_sum<64>(s1);
    s2 = tl_tree_sum<64>(s2);
    if ((t & 63) == 0) {
        red[t >> 6][0] = s1;
        red[t >> 6][1] = s2;
    }
    __syncthreads();
    if (t < 2) part[(((long)b * nchunk + chunk) * 2 + t) * c + ch] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// One workgroup.  part (nparts, 2, c) -> sums (2, c) f64; dbeta (or dbias) = s1 and dgamma = s2, rounded once (either may be NULL).
__global__ __launch_bounds__(256) void tl_bwd_finish_kernel(int c, long nparts, int bn, const double *__restrict__ part, double *__restrict__ sums,
                                                            float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    for (int ch = threadIdx.x; ch < c; ch += 256) {
        double S1 = 0.0, S2 = 0.0;
        for (long i = 0; i < nparts; ++i) {
            S1 += part[i * 2 * c + ch];
            if (bn) S2 += part[(i * 2 + 1) * c + ch];
        }
        sums[ch] = S1;
        sums[c + ch] = S2;
        if (dbeta) dbeta[ch] = (float)S1;
        if (bn && dgamma) dgamma[ch] = (float)S2;
    }
}

__global__ __launch_bounds__(256) void tl_bn_dz_kernel(int c, int P, int relu, double n, const float *__restrict__ dy, const float *__restrict__ z,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const double *__restrict__ stats, const double *__restrict__ sums, float *__restrict__ dz)
{
    const long row = blockIdx.x;
    const int ch = (int)(row % c);
    const double mean = stats[ch], rstd = stats[c + ch];
    const float ga = gamma[ch], be = beta[ch];
    const double m1 = sums[ch] / n, m2 = sums[c + ch] / n, scale = (double)ga * rstd;
#pragma unroll
    for (int j = 0; j < TL_CHUNK / 256; ++j) {
        const long p = (long)blockIdx.y * TL_CHUNK + j * 256 + threadIdx.x;
        if (p < P) {
            const double zh = tl_zhat(z[row * P + p], mean, rstd);
            const double g = (relu && !(tl_preact(zh, ga, be) > 0.0)) ? 0.0 : (double)dy[row * P + p];
            dz[row * P + p] = (float)(scale * ((g - m1) - zh * m2));
        }
    }
}

// dwp (B * nchunk, cout, cin)[part][co][ci] = the fmaf chain over the chunk's positions, ascending, of dz[b][co][p] * x[b][ci][p].
// grid (B * nchunk, ceil(cout / 64), ceil(cin / 64)); wave w owns the 32 x 32 tile (co tile w / 2, ci tile w % 2).
__global__ __launch_bounds__(256) void tl_dw_kernel(int cin, int cout, int P, int nchunk, const float *__restrict__ dz, const float *__restrict__ x,
                                                    float *__restrict__ dwp)
{
    __shared__ float ta[64][TL_KT + 1], tb[64][TL_KT + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long partid = blockIdx.x;
    const int b = (int)(partid / nchunk), chunk = (int)(partid % nchunk);
    const int co0 = blockIdx.y * 64, ci0 = blockIdx.z * 64;
    const float *dzb = dz + (long)b * cout * P, *xb = x + (long)b * cin * P;
    const int cot = wave >> 1, cit = wave & 1;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
    for (int st = 0; st < TL_CHUNK / TL_KT; ++st) {
        const long pbase = (long)chunk * TL_CHUNK + st * TL_KT;
        if (pbase >= P) break;                                   // workgroup-uniform
        __syncthreads();
        for (int i = t; i < 64 * TL_KT; i += 256) {
            const int r = i / TL_KT, j = i % TL_KT;
            const long p = pbase + j;
            ta[r][j] = (co0 + r < cout && p < P) ? dzb[(long)(co0 + r) * P + p] : 0.0f;
            tb[r][j] = (ci0 + r < cin && p < P) ? xb[(long)(ci0 + r) * P + p] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TL_KT / 2; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ta[cot * 32 + (lane & 31)][2 * j + (lane >> 5)],
                                                       tb[cit * 32 + (lane & 31)][2 * j + (lane >> 5)], acc, 0, 0, 0);
    }
    float *o = dwp + partid * cout * cin;
    const int ci = ci0 + cit * 32 + (lane & 31);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int co = co0 + cot * 32 + tl_acc_row(v, lane);
        if (co < cout && ci < cin) o[(long)co * cin + ci] = acc[v];
    }
}

__global__ __launch_bounds__(256) void tl_dw_reduce_kernel(long elems, long nparts, const float *__restrict__ dwp, float *__restrict__ dw)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    double s = 0.0;
    for (long i = 0; i < nparts; ++i) s += (double)dwp[i * elems + e];
    dw[e] = (float)s;
}

template <int EPI, bool TRANS>
static void launch_gemm(int b, int M, int K, int P, int nchunk, const float *a, const float *X, const float *bias, int relu, float *out,
                        double *part, hipStream_t st)
{
    if (M <= 32)
        hipLaunchKernelGGL((tl_gemm_kernel<1, EPI, TRANS>), dim3(nchunk, ceil_div(M, 32), b), dim3(256), 0, st, M, K, P, nchunk, a, X, bias, relu, out, part);
    else
        hipLaunchKernelGGL((tl_gemm_kernel<2, EPI, TRANS>), dim3(nchunk, ceil_div(M, 64), b), dim3(256), 0, st, M, K, P, nchunk, a, X, bias, relu, out, part);
}

static int tl_sizes(const char *what, int b, int cin, int cout, int p, int *nchunk)
{
    PRCNN_REQUIRE(b >= 1 && cin >= 1 && cout >= 1 && p >= 1, "%s: bad sizes b=%d cin=%d cout=%d p=%d", what, b, cin, cout, p);
    *nchunk = ceil_div(p, TL_CHUNK);
    PRCNN_REQUIRE(b <= 65535 && *nchunk <= 65535 && cin <= 65535 * 32 && cout <= 65535 * 32, "%s: b=%d cin=%d cout=%d p=%d exceed a launch", what, b, cin,
                  cout, p);
    PRCNN_REQUIRE((long)b * cout <= INT_MAX && (long)b * cin <= INT_MAX && (long)b * *nchunk <= INT_MAX, "%s: b=%d cin=%d cout=%d p=%d too large", what,
                  b, cin, cout, p);
    return PRCNN_OK;
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_train_layer_workspace(int b, int cin, int cout, int p, long *stat_f64, long *dw_f32)
{
    int nchunk;
    const int rc = tl_sizes("train_layer_workspace", b, cin, cout, p, &nchunk);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(stat_f64 && dw_f32, "train_layer_workspace: null pointer");
    const long parts = (long)b * nchunk;
    *stat_f64 = (parts + 1) * 2 * cout;                          // the chunk partials, then the two finished sums of the backward
    *dw_f32 = parts * cout * cin;
    return PRCNN_OK;
}

extern "C" int prcnn_train_layer_forward(int b, int cin, int cout, int p, int bn, int relu, const float *x, const float *w, const float *gamma,
                                         const float *beta, double eps, double momentum, float *running_mean, float *running_var, float *z,
                                         float *y, double *stats, double *work, void *stream)
{
    int nchunk;
    const int rc = tl_sizes("train_layer_forward", b, cin, cout, p, &nchunk);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(x && w && y, "train_layer_forward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!bn) {                                                   // beta is the bias (NULL: none)
        launch_gemm<TL_EPI_BIAS, false>(b, cout, cin, p, nchunk, w, x, beta, relu, y, nullptr, st);
        return check_launch("train_layer_forward");
    }
    PRCNN_REQUIRE((long)b * p > 1, "train_layer_forward: BatchNorm on batch statistics needs more than one value per channel (b * p = 1)");
    PRCNN_REQUIRE(gamma && beta && z && stats && work, "train_layer_forward: null pointer (BatchNorm)");
    launch_gemm<TL_EPI_STATS, false>(b, cout, cin, p, nchunk, w, x, nullptr, 0, z, work, st);
    hipLaunchKernelGGL(tl_bn_finish_kernel, dim3(1), dim3(256), 0, st, cout, (long)b * nchunk, (double)b * (double)p, work, eps, momentum, running_mean,
                       running_var, stats);
    hipLaunchKernelGGL(tl_bn_apply_kernel, dim3((unsigned)((long)b * cout), nchunk), dim3(256), 0, st, cout, p, relu, z, gamma, beta, stats, y);
    return check_launch("train_layer_forward");
}

extern "C" int prcnn_train_layer_backward(int b, int cin, int cout, int p, int bn, int relu, const float *dy, const float *x, const float *w,
                                          const float *zy, const float *gamma, const float *beta, const double *stats, float *dz, float *dx,
                                          float *dw, float *dgamma, float *dbeta, double *work, float *dw_work, void *stream)
{
    int nchunk;
    const int rc = tl_sizes("train_layer_backward", b, cin, cout, p, &nchunk);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(dy && x && w, "train_layer_backward: null pointer");
    PRCNN_REQUIRE(!bn || (zy && gamma && beta && stats && dz && work), "train_layer_backward: null pointer (BatchNorm)");
    PRCNN_REQUIRE(bn || !relu || (zy && dz), "train_layer_backward: null pointer (ReLU)");
    PRCNN_REQUIRE(bn || !(relu || dbeta) || work, "train_layer_backward: null pointer (workspace)");
    PRCNN_REQUIRE(!dw || dw_work, "train_layer_backward: null pointer (weight)");
    hipStream_t st = (hipStream_t)stream;
    const long parts = (long)b * nchunk;
    const dim3 rows_chunks((unsigned)((long)b * cout), nchunk);
    double *sums = work ? work + parts * 2 * cout : nullptr;
    const float *g = dy;                                         // the gradient at the convolution's output
    if (bn) {
        hipLaunchKernelGGL(tl_bwd_partials_kernel<true>, rows_chunks, dim3(256), 0, st, cout, p, nchunk, relu, dy, zy, gamma, beta, stats,
                           (float *)nullptr, work);
        hipLaunchKernelGGL(tl_bwd_finish_kernel, dim3(1), dim3(256), 0, st, cout, parts, 1, work, sums, dgamma, dbeta);
        hipLaunchKernelGGL(tl_bn_dz_kernel, rows_chunks, dim3(256), 0, st, cout, p, relu, (double)b * (double)p, dy, zy, gamma, beta, stats, sums, dz);
        g = dz;
    } else if (relu || dbeta) {
        hipLaunchKernelGGL(tl_bwd_partials_kernel<false>, rows_chunks, dim3(256), 0, st, cout, p, nchunk, relu, dy, zy, (const float *)nullptr,
                           (const float *)nullptr, (const double *)nullptr, relu ? dz : (float *)nullptr, work);
        if (dbeta) hipLaunchKernelGGL(tl_bwd_finish_kernel, dim3(1), dim3(256), 0, st, cout, parts, 0, work, sums, (float *)nullptr, dbeta);
        if (relu) g = dz;
    }
    if (dx) launch_gemm<TL_EPI_PLAIN, true>(b, cin, cout, p, nchunk, w, g, nullptr, 0, dx, nullptr, st);
    if (dw) {
        hipLaunchKernelGGL(tl_dw_kernel, dim3((unsigned)parts, ceil_div(cout, 64), ceil_div(cin, 64)), dim3(256), 0, st, cin, cout, p, nchunk, g, x, dw_work);
        const long elems = (long)cout * cin;
        hipLaunchKernelGGL(tl_dw_reduce_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, elems, parts, dw_work, dw);
    }
    return check_launch("train_layer_backward");
}
