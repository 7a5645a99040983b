// packed_valu.hip -- the two VALU kernels beside the MFMA layers of csrc/packed_layer.hip: layer 1 of a wide packed level over the
// rows of a list (gather + affine, no matrix product: the per-point part P was multiplied once per point), and the GEMV of the
// 1..4-wide last layer of the classification heads.
#include "layer_tile.hpp"

namespace prcnn {

struct PGProblem {
    int n, c1; const unsigned int *hdr; const float4 *rowdxyz; const float4 *P; const float4 *wxyz; const unsigned int *rowinfo;
    const int *tilecloud; float4 *out;
};
struct PGBatch { PGProblem p[PL_MAX_BATCH]; };

__global__ __launch_bounds__(256) void packed_gather_affine_kernel(const PGBatch bt)
{
    const PGProblem &pb = bt.p[blockIdx.z];
    const int n = pb.n, c1 = pb.c1;
    const unsigned int *__restrict__ hdr = pb.hdr;
    const float4 *__restrict__ rowdxyz = pb.rowdxyz;
    const float4 *__restrict__ P = pb.P;
    const float4 *__restrict__ wxyz = pb.wxyz;
    const unsigned int *__restrict__ rowinfo = pb.rowinfo;
    const int *__restrict__ tilecloud = pb.tilecloud;
    float4 *__restrict__ out = pb.out;
    const long t = blockIdx.x;
    if (t >= (long)hdr[0]) return;
    const int cloud = tilecloud[t];
    const int q4 = c1 / 4;                                 // float4 chunks per row
    const long pbase = (long)cloud * n;
    for (int e = threadIdx.x; e < PL_ROWS * q4; e += 256) {
        const int row = e / q4, q = e - row * q4;
        const int k = (int)(rowinfo[t * PL_ROWS + row] & 0xffffu);
        const float4 d = rowdxyz[t * PL_ROWS + row];
        const float dx = d.x, dy = d.y, dz = d.z;
        const float4 base = P[(pbase + k) * q4 + q];
        const float4 wx = wxyz[q], wy = wxyz[q4 + q], wz = wxyz[2 * q4 + q];
        const float4 v = affine_relu4(base, wx, wy, wz, dx, dy, dz);
        out[(t * PL_ROWS + row) * q4 + q] = v;
    }
}

// out[r][0..n) = A[r][0..K) @ W + bias for n <= 4 output columns (the 1-wide last layer of the classification heads): a
// GEMV per output, no MFMA tile to fill.  32 lanes per row: lane l accumulates k = l, l + 32, ... as one fma chain (from 0),
// the 32 partial sums are added in an xor butterfly (16, 8, 4, 2, 1), then the bias.  oracle/mlp_oracle.c orc_rows_dot
// restates that order.
__global__ __launch_bounds__(256) void rows_dot_kernel(long rows, int K, int n, const float *__restrict__ A, long lda,
                                                       const float *__restrict__ W, const float *__restrict__ bias,
                                                       float *__restrict__ out, long ldo)
{
    const long r = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int l = threadIdx.x & 31;
    const long rr = r < rows ? r : rows - 1;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = l; k < K; k += 32) {
        const float a = A[rr * lda + k];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < n) acc[c] = fmaf(a, W[(long)k * n + c], acc[c]);
    }
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], __shfl_xor(acc[c], d, 32));
    if (l == 0 && r < rows)
        for (int c = 0; c < n; ++c) out[r * ldo + c] = __fadd_rn(acc[c], bias[c]);
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_rows_dot(long rows, int K, int n, const float *A, long lda, const float *W, const float *bias, float *out,
                              long ldo, void *stream)
{
    PRCNN_REQUIRE(rows >= 0 && K > 0 && n >= 1 && n <= 4 && lda >= K && ldo >= n, "rows_dot: bad sizes (n <= 4)");
    if (rows == 0) return PRCNN_OK;
    PRCNN_REQUIRE(A && W && bias && out, "rows_dot: null pointer");
    PRCNN_REQUIRE((rows + 7) / 8 <= 0x7fffffffL, "rows_dot: too many rows");
    hipLaunchKernelGGL(rows_dot_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, (hipStream_t)stream, rows, K, n, A, lda, W,
                       bias, out, ldo);
    return check_launch("rows_dot");
}

// A1 (max_tiles*64, c1) = relu(P[point] + wxyz . rowdxyz) for every packed row (prcnn_ball_pack: rowdxyz = xyz[point] - centre);
// P (b,n,c1), wxyz (3,c1), c1 % 4 == 0.  Up to 4 problems (the scales of one MSG level) share one launch.
extern "C" int prcnn_packed_gather_affine_batch(int nprob, const prcnn_gather_problem *pr, void *stream)
{
    PRCNN_REQUIRE(nprob >= 0 && nprob <= PL_MAX_BATCH && (nprob == 0 || pr), "packed_gather_affine: 0..%d problems", PL_MAX_BATCH);
    PGBatch bt;
    int k = 0;
    long grid_x = 0;
    for (int i = 0; i < nprob; ++i) {
        const prcnn_gather_problem &q = pr[i];
        PRCNN_REQUIRE(q.b >= 0 && q.n >= 0 && q.max_tiles >= 0 && q.c1 > 0 && q.c1 % 4 == 0, "packed_gather_affine: bad sizes");
        if (q.max_tiles == 0) continue;
        PRCNN_REQUIRE(q.P && q.wxyz && q.rowinfo && q.rowdxyz && q.tilecloud && q.hdr && q.out, "packed_gather_affine: null pointer");
        PRCNN_REQUIRE((((uintptr_t)q.P | (uintptr_t)q.wxyz | (uintptr_t)q.out) & 15) == 0, "packed_gather_affine: 16-byte alignment required");
        PRCNN_REQUIRE(q.max_tiles <= 0x7fffffffL, "packed_gather_affine: too many tiles");
        bt.p[k++] = PGProblem{q.n, q.c1, q.hdr, (const float4 *)q.rowdxyz, (const float4 *)q.P, (const float4 *)q.wxyz, q.rowinfo,
                              q.tilecloud, (float4 *)q.out};
        if (q.max_tiles > grid_x) grid_x = q.max_tiles;
    }
    if (k == 0) return PRCNN_OK;
    hipLaunchKernelGGL(packed_gather_affine_kernel, dim3((unsigned)grid_x, 1, k), dim3(256), 0, (hipStream_t)stream, bt);
    return check_launch("packed_gather_affine");
}

extern "C" int prcnn_packed_gather_affine(int b, int n, int c1, long max_tiles, const float *P, const float *wxyz,
                                          const unsigned int *rowinfo, const float *rowdxyz, const int *tilecloud,
                                          const unsigned int *hdr, float *out, void *stream)
{
    const prcnn_gather_problem q = {b, n, c1, max_tiles, P, wxyz, rowinfo, rowdxyz, tilecloud, hdr, out};
    return prcnn_packed_gather_affine_batch(1, &q, stream);
}
