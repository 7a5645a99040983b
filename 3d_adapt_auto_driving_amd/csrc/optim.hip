// optim.hip -- the weight step of training: gradient-norm clip, decoupled weight decay and Adam over EVERY parameter tensor of a model
// in three launches (tools/train_utils/train_utils.py Trainer._train_it clip_grad_norm_, fastai_optim.py OptimWrapper.step, torch.optim.Adam):
// prcnn_optim_sumsq, prcnn_optim_finish, prcnn_optim_update (include/prcnn_hip.h; optim.py).
// The tensors are described by a table of plain device arrays (optim.py builds it; nothing here allocates or copies):
//   per tensor  param / grad / exp_avg / exp_avg_sq addresses (0: absent), numel, flags (bit 0 decay, bit 1 adam), step
//   per chunk   tensor index and start offset; a chunk is OPT_CHUNK consecutive elements of ONE tensor (the last one of a tensor is short)
//   optim_sumsq_kernel    one workgroup per chunk: f64 sum of squares of the f32 grads -> work[2 + chunk] (0 where the tensor has no grad)
//   optim_finish_kernel   one workgroup: the partials in a fixed order -> work[0] = total_norm, work[1] = coef; step += 1 where "adam"
//   optim_update_kernel   one workgroup per chunk: the elementwise step
// The rule of losses.hip holds here too: the arithmetic runs in f64 from the f32 state and every stored value is rounded to f32 once.  Sums
// go through per-thread accumulators over a FIXED element assignment (the same one on the wide and the scalar path), a butterfly over the
// wave, four LDS words and per-chunk partials: no atomics, so the same input gives the same bits.  A kernel boundary, not a fence, hands
// the partials and the coefficient to the next launch.  Grads are read, never written.
#include "common.hpp"
#include <math.h>

namespace prcnn {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = PRCNN_OPTIM_CHUNK;        // elements per workgroup: 2 x float4 per thread
constexpr int OPT_PER_THREAD = OPT_CHUNK / OPT_THREADS;
constexpr int OPT_VEC = OPT_PER_THREAD / 4;        // float4 loads per thread and array
constexpr int OPT_MAX_CHUNKS = 1 << 22;
constexpr unsigned OPT_DECAY = 1u, OPT_ADAM = 2u;
static_assert(OPT_PER_THREAD % 4 == 0, "whole float4s per thread");

// element e of thread t's v-th float4 sits at v * (4 * OPT_THREADS) + 4 * t + e: consecutive lanes read consecutive 16 bytes
__device__ __forceinline__ int elem_of(int v, int e) { return v * (4 * OPT_THREADS) + 4 * (int)threadIdx.x + e; }

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the block's sum in every thread (losses.hip block_sum with one value): butterfly over the wave, then the four waves in wave order
__device__ __forceinline__ double block_sum1(double v, double *sm)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    __syncthreads();
    return v;
}

__global__ void __launch_bounds__(OPT_THREADS) optim_sumsq_kernel(const unsigned long long *__restrict__ grad_addr, const long long *__restrict__ numel,
                                                                   const int *__restrict__ chunk_tensor, const long long *__restrict__ chunk_start,
                                                                   int n_tensors, double *__restrict__ work)
{
    __shared__ double sm[4];
    const int c = blockIdx.x, t = chunk_tensor[c];
    const float *g = (unsigned)t < (unsigned)n_tensors ? (const float *)grad_addr[t] : nullptr;
    if (!g) {                                      // (uniform over the workgroup)
        if (threadIdx.x == 0) work[2 + c] = 0.0;
        return;
    }
    const long long start = chunk_start[c];
    const long long left = numel[t] - start;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    g += start;
    float x[OPT_PER_THREAD];
    if (n == OPT_CHUNK && aligned16(g)) {
#pragma unroll
        for (int v = 0; v < OPT_VEC; ++v) {
            const float4 q = *(const float4 *)(g + elem_of(v, 0));
            x[4 * v] = q.x; x[4 * v + 1] = q.y; x[4 * v + 2] = q.z; x[4 * v + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int v = 0; v < OPT_VEC; ++v) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = elem_of(v, e);
                x[4 * v + e] = i < n ? g[i] : 0.f;
            }
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_PER_THREAD; ++k) s += (double)x[k] * (double)x[k];
    s = block_sum1(s, sm);
    if (threadIdx.x == 0) work[2 + c] = s;
}

__global__ void __launch_bounds__(OPT_THREADS) optim_finish_kernel(const unsigned char *__restrict__ flags, int *__restrict__ steps, int n_tensors,
                                                                    int n_chunks, double max_norm, double *__restrict__ work)
{
    __shared__ double sm[4];
    double s = 0.0;
    for (int c = threadIdx.x; c < n_chunks; c += OPT_THREADS) s += work[2 + c];
    s = block_sum1(s, sm);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        const double c = max_norm / (norm + 1e-6);
        work[0] = norm;
        work[1] = c < 1.0 ? c : (c != c ? c : 1.0);          // clamp(max = 1) as torch clamps: a NaN norm stays NaN
    }
    for (int t = threadIdx.x; t < n_tensors; t += OPT_THREADS) {
        if (flags[t] & OPT_ADAM) steps[t] += 1;
    }
}

struct OptHyper {
    double lr, beta1, beta2, eps, wd;
};

// one element: (p, g, m, v) -> (p, m, v), every result rounded to f32 once
template <bool ADAM>
__device__ __forceinline__ void step_elem(float &p, float g, float &m, float &v, double coef, double decay, double one_m_b1, double beta2,
                                          double one_m_b2, double step_size, double sqrt_bc2, double eps)
{
    double pd = (double)p * decay;
    if (ADAM) {
        const double gd = (double)g * coef;
        const double md = (double)m + (gd - (double)m) * one_m_b1;
        const double vd = beta2 * (double)v + one_m_b2 * gd * gd;
        m = (float)md;
        v = (float)vd;
        pd -= step_size * md / (sqrt(vd) / sqrt_bc2 + eps);
    }
    p = (float)pd;
}

template <bool ADAM>
__device__ __forceinline__ void step_chunk(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, int n,
                                           double coef, double decay, double one_m_b1, double beta2, double one_m_b2, double step_size,
                                           double sqrt_bc2, double eps)
{
    const bool wide = n == OPT_CHUNK && aligned16(p) && (!ADAM || (aligned16(g) && aligned16(m) && aligned16(v)));
    if (wide) {
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            const int i = elem_of(k, 0);
            float4 pq = *(float4 *)(p + i), gq = make_float4(0.f, 0.f, 0.f, 0.f), mq = gq, vq = gq;
            if (ADAM) {
                gq = *(const float4 *)(g + i);
                mq = *(float4 *)(m + i);
                vq = *(float4 *)(v + i);
            }
            step_elem<ADAM>(pq.x, gq.x, mq.x, vq.x, coef, decay, one_m_b1, beta2, one_m_b2, step_size, sqrt_bc2, eps);
            step_elem<ADAM>(pq.y, gq.y, mq.y, vq.y, coef, decay, one_m_b1, beta2, one_m_b2, step_size, sqrt_bc2, eps);
            step_elem<ADAM>(pq.z, gq.z, mq.z, vq.z, coef, decay, one_m_b1, beta2, one_m_b2, step_size, sqrt_bc2, eps);
            step_elem<ADAM>(pq.w, gq.w, mq.w, vq.w, coef, decay, one_m_b1, beta2, one_m_b2, step_size, sqrt_bc2, eps);
            *(float4 *)(p + i) = pq;
            if (ADAM) {
                *(float4 *)(m + i) = mq;
                *(float4 *)(v + i) = vq;
            }
        }
    } else {
        for (int i = threadIdx.x; i < n; i += OPT_THREADS) {
            float pe = p[i], ge = 0.f, me = 0.f, ve = 0.f;
            if (ADAM) {
                ge = g[i]; me = m[i]; ve = v[i];
            }
            step_elem<ADAM>(pe, ge, me, ve, coef, decay, one_m_b1, beta2, one_m_b2, step_size, sqrt_bc2, eps);
            p[i] = pe;
            if (ADAM) {
                m[i] = me; v[i] = ve;
            }
        }
    }
}

__global__ void __launch_bounds__(OPT_THREADS) optim_update_kernel(const unsigned long long *__restrict__ param_addr,
                                                                    const unsigned long long *__restrict__ grad_addr,
                                                                    const unsigned long long *__restrict__ m_addr,
                                                                    const unsigned long long *__restrict__ v_addr, const long long *__restrict__ numel,
                                                                    const unsigned char *__restrict__ flags, const int *__restrict__ steps,
                                                                    const int *__restrict__ chunk_tensor, const long long *__restrict__ chunk_start,
                                                                    int n_tensors, const OptHyper h, const double *__restrict__ work)
{
    const int c = blockIdx.x, t = chunk_tensor[c];
    if ((unsigned)t >= (unsigned)n_tensors) return;
    const unsigned f = flags[t];
    if (!(f & (OPT_DECAY | OPT_ADAM))) return;     // frozen: never touched (uniform over the workgroup)
    const long long start = chunk_start[c];
    const long long left = numel[t] - start;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    float *p = (float *)param_addr[t] + start;
    const double decay = (f & OPT_DECAY) ? 1.0 - h.wd * h.lr : 1.0;
    if (f & OPT_ADAM) {
        const double step = (double)steps[t];      // already incremented by the finish launch
        const double bc1 = 1.0 - pow(h.beta1, step), bc2 = 1.0 - pow(h.beta2, step);
        step_chunk<true>(p, (const float *)grad_addr[t] + start, (float *)m_addr[t] + start, (float *)v_addr[t] + start, n, work[1], decay,
                         1.0 - h.beta1, h.beta2, 1.0 - h.beta2, h.lr / bc1, sqrt(bc2), h.eps);
    } else {
        step_chunk<false>(p, nullptr, nullptr, nullptr, n, 1.0, decay, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
    }
}

int check_table(const char *what, int n_tensors, int n_chunks)
{
    PRCNN_REQUIRE(n_tensors >= 1, "%s: n_tensors = %d", what, n_tensors);
    PRCNN_REQUIRE(n_chunks >= 1 && n_chunks <= OPT_MAX_CHUNKS, "%s: n_chunks = %d (1 .. %d)", what, n_chunks, OPT_MAX_CHUNKS);
    return PRCNN_OK;
}

}  // namespace
}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_optim_workspace(int n_chunks)
{
    PRCNN_REQUIRE(n_chunks >= 0 && n_chunks <= OPT_MAX_CHUNKS, "optim_workspace: n_chunks = %d (0 .. %d)", n_chunks, OPT_MAX_CHUNKS);
    return 2 + n_chunks;
}

extern "C" int prcnn_optim_sumsq(const unsigned long long *grad_addr, const long long *numel, const int *chunk_tensor, const long long *chunk_start,
                                 int n_tensors, int n_chunks, double *work, void *stream)
{
    const int rc = check_table("optim_sumsq", n_tensors, n_chunks);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(grad_addr && numel && chunk_tensor && chunk_start && work, "optim_sumsq: null pointer");
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, grad_addr, numel, chunk_tensor, chunk_start,
                       n_tensors, work);
    return check_launch("optim_sumsq");
}

extern "C" int prcnn_optim_finish(const unsigned char *flags, int *steps, int n_tensors, int n_chunks, double max_norm, double *work, void *stream)
{
    const int rc = check_table("optim_finish", n_tensors, n_chunks);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(flags && steps && work, "optim_finish: null pointer");
    PRCNN_REQUIRE(max_norm > 0.0, "optim_finish: max_norm = %g", max_norm);
    hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, flags, steps, n_tensors, n_chunks, max_norm, work);
    return check_launch("optim_finish");
}

extern "C" int prcnn_optim_update(const unsigned long long *param_addr, const unsigned long long *grad_addr, const unsigned long long *exp_avg_addr,
                                  const unsigned long long *exp_avg_sq_addr, const long long *numel, const unsigned char *flags, const int *steps,
                                  const int *chunk_tensor, const long long *chunk_start, int n_tensors, int n_chunks, double lr, double beta1,
                                  double beta2, double eps, double wd, const double *work, void *stream)
{
    const int rc = check_table("optim_update", n_tensors, n_chunks);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(param_addr && grad_addr && exp_avg_addr && exp_avg_sq_addr && numel && flags && steps && chunk_tensor && chunk_start && work,
                  "optim_update: null pointer");
    PRCNN_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && wd >= 0.0,
                  "optim_update: lr %g beta1 %g beta2 %g eps %g wd %g", lr, beta1, beta2, eps, wd);
    const OptHyper h = {lr, beta1, beta2, eps, wd};
    hipLaunchKernelGGL(optim_update_kernel, dim3(n_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, param_addr, grad_addr, exp_avg_addr,
                       exp_avg_sq_addr, numel, flags, steps, chunk_tensor, chunk_start, n_tensors, h, work);
    return check_launch("optim_update");
}
