// grad_bucket.hip -- the two kernels of data-parallel training that run over the weight step's chunk table (optim.hip, optim.py) with one
// extra per-tensor column, slot_start: prcnn_grad_pack, prcnn_param_digest (include/prcnn_hip.h; dist_train.py).
//   grad_pack_kernel      one workgroup per chunk: the chunk's f32 gradients -> bucket[slot_start[tensor] + chunk_start ...], ONE launch for
//                         every tensor of the model.  The bucket is what one all-reduce exchanges; after it the table's grad addresses
//                         point INTO the bucket and the three launches of optim.hip read the reduced gradients there.
//   digest_partial_kernel one workgroup per chunk: sum of bits(p[j]) * (2 (slot_start + j) + 1) mod 2^64 -> work[1 + chunk]
//   digest_finish_kernel  one workgroup: the partials -> work[0]
// A slot starts at a multiple of 64 elements of a 16-byte aligned bucket and a chunk at a multiple of OPT_CHUNK, so the destination of a
// chunk is always 16-byte aligned; the SOURCE need not be (a gradient may be a view at an odd element offset), which selects the scalar
// loads.  Padding between slots is never written (dist_train.py zeroes it at allocation).  The digest is integer arithmetic mod 2^64:
// every order of summation gives the same value, so it needs no fixed shape to be reproducible.
#include "common.hpp"

namespace prcnn {
namespace {

constexpr int GB_THREADS = 256;
constexpr int GB_CHUNK = PRCNN_OPTIM_CHUNK;
constexpr int GB_VEC = GB_CHUNK / (4 * GB_THREADS);  // float4s per thread
constexpr int GB_MAX_CHUNKS = 1 << 22;
static_assert(GB_CHUNK % (4 * GB_THREADS) == 0, "whole float4s per thread");

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the chunk's extent, or 0 where the table's row is unusable (out of range, no address, past the tensor's end)
__device__ __forceinline__ int chunk_extent(int t, int n_tensors, const unsigned long long *addr, const long long *numel, long long start)
{
    if ((unsigned)t >= (unsigned)n_tensors || !addr[t]) return 0;
    const long long left = numel[t] - start;
    if (start < 0 || left <= 0) return 0;
    return left < GB_CHUNK ? (int)left : GB_CHUNK;
}

__global__ void __launch_bounds__(GB_THREADS) grad_pack_kernel(const unsigned long long *__restrict__ src_addr, const long long *__restrict__ numel,
                                                                const long long *__restrict__ slot_start, const int *__restrict__ chunk_tensor,
                                                                const long long *__restrict__ chunk_start, int n_tensors,
                                                                float *__restrict__ bucket, long long bucket_numel)
{
    const int c = blockIdx.x, t = chunk_tensor[c];
    const long long start = chunk_start[c];
    const int n = chunk_extent(t, n_tensors, src_addr, numel, start);  // (uniform over the workgroup)
    if (n == 0) return;
    const long long at = slot_start[t] + start;
    if (at < 0 || at + n > bucket_numel) return;   // a table that does not fit its bucket writes nothing
    const float *g = (const float *)src_addr[t] + start;
    float *dst = bucket + at;
    if (n == GB_CHUNK && aligned16(g) && aligned16(dst)) {
#pragma unroll
        for (int v = 0; v < GB_VEC; ++v) {
            const int i = v * (4 * GB_THREADS) + 4 * (int)threadIdx.x;
            *(float4 *)(dst + i) = *(const float4 *)(g + i);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += GB_THREADS) dst[i] = g[i];
    }
}

// the block's sum mod 2^64 in thread 0
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long *sm)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, WAVE);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ void __launch_bounds__(GB_THREADS) digest_partial_kernel(const unsigned long long *__restrict__ param_addr,
                                                                     const long long *__restrict__ numel, const long long *__restrict__ slot_start,
                                                                     const int *__restrict__ chunk_tensor, const long long *__restrict__ chunk_start,
                                                                     int n_tensors, unsigned long long *__restrict__ work)
{
    __shared__ unsigned long long sm[GB_THREADS / WAVE];
    const int c = blockIdx.x, t = chunk_tensor[c];
    const long long start = chunk_start[c];
    const int n = chunk_extent(t, n_tensors, param_addr, numel, start);
    unsigned long long s = 0;
    if (n) {
        const unsigned *p = (const unsigned *)param_addr[t] + start;
        const unsigned long long at = (unsigned long long)(slot_start[t] + start);
        for (int i = threadIdx.x; i < n; i += GB_THREADS) s += (unsigned long long)p[i] * (2ull * (at + (unsigned long long)i) + 1ull);
    }
    s = block_sum_u64(s, sm);
    if (threadIdx.x == 0) work[1 + c] = s;
}

__global__ void __launch_bounds__(GB_THREADS) digest_finish_kernel(int n_chunks, unsigned long long *__restrict__ work)
{
    __shared__ unsigned long long sm[GB_THREADS / WAVE];
    unsigned long long s = 0;
    for (int c = threadIdx.x; c < n_chunks; c += GB_THREADS) s += work[1 + c];
    s = block_sum_u64(s, sm);
    if (threadIdx.x == 0) work[0] = s;
}

int check_bucket_table(const char *what, int n_tensors, int n_chunks)
{
    PRCNN_REQUIRE(n_tensors >= 1, "%s: n_tensors = %d", what, n_tensors);
    PRCNN_REQUIRE(n_chunks >= 1 && n_chunks <= GB_MAX_CHUNKS, "%s: n_chunks = %d (1 .. %d)", what, n_chunks, GB_MAX_CHUNKS);
    return PRCNN_OK;
}

}  // namespace
}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_grad_pack(const unsigned long long *src_addr, const long long *numel, const long long *slot_start, const int *chunk_tensor,
                               const long long *chunk_start, int n_tensors, int n_chunks, float *bucket, long long bucket_numel, void *stream)
{
    const int rc = check_bucket_table("grad_pack", n_tensors, n_chunks);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(src_addr && numel && slot_start && chunk_tensor && chunk_start && bucket, "grad_pack: null pointer");
    PRCNN_REQUIRE(bucket_numel >= 1, "grad_pack: bucket_numel = %lld", bucket_numel);
    PRCNN_REQUIRE(((uintptr_t)bucket & 15u) == 0, "grad_pack: the bucket is not 16-byte aligned");
    hipLaunchKernelGGL(grad_pack_kernel, dim3(n_chunks), dim3(GB_THREADS), 0, (hipStream_t)stream, src_addr, numel, slot_start, chunk_tensor,
                       chunk_start, n_tensors, bucket, bucket_numel);
    return check_launch("grad_pack");
}

extern "C" int prcnn_param_digest(const unsigned long long *param_addr, const long long *numel, const long long *slot_start, const int *chunk_tensor,
                                  const long long *chunk_start, int n_tensors, int n_chunks, unsigned long long *work, void *stream)
{
    const int rc = check_bucket_table("param_digest", n_tensors, n_chunks);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(param_addr && numel && slot_start && chunk_tensor && chunk_start && work, "param_digest: null pointer");
    hipLaunchKernelGGL(digest_partial_kernel, dim3(n_chunks), dim3(GB_THREADS), 0, (hipStream_t)stream, param_addr, numel, slot_start, chunk_tensor,
                       chunk_start, n_tensors, work);
    hipLaunchKernelGGL(digest_finish_kernel, dim3(1), dim3(GB_THREADS), 0, (hipStream_t)stream, n_chunks, work);
    return check_launch("param_digest");
}
