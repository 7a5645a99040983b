// object_scale.hip -- random object scaling of a training batch (object_scale.py; no counterpart in the reference): every point that a
// labelled box owns is scaled about the box's bottom centre by the box's factor.
//
// One launch, one thread per point, a grid of (ceil(n / 256), b).  The scene's boxes are staged through LDS in chunks of OS_CHUNK
// records of OS_REC doubles (X, Y, Z, h, l / 2, w / 2, cos, sin, factor), the way rpn_labels_kernel stages its boxes, and visited in
// order k = 0 .. count - 1: the FIRST box that contains the point owns it, and a point that has an owner skips the boxes behind it.
// A thread leaves the chunk loop only with its whole workgroup (the staging barriers).  Ownership is decided on the input boxes and the
// input coordinates alone, so no thread reads what another writes: the launch works in place.
//
//   dx = px - X, dz = pz - Z, v = Y - py, a = dx c - dz s, b = dx s + dz c         (a along the length, b along the width, v the height
//   inside iff |a| <= l / 2 && |b| <= w / 2 && 0 <= v && v <= h                     above the bottom face; y points down)
//   r != 1:  a' = a r, b' = b r, v' = v r;  px' = f32(X + (a' c + b' s)), py' = f32(Y - v'), pz' = f32(Z + (b' c - a' s))
//
// All of it in f64 on values widened from f32, one rounding per operation (-ffp-contract=off), no transcendental: cos / sin of ry come
// from the host.  A NaN coordinate fails every comparison and is inside nothing.  r == 1 keeps the point's bits (no store at all).
// hits[s, k] = points that box k owns, whatever its factor: per box and wave a ballot over the lanes that found their owner in this
// box, one u32 atomicAdd by the wave's first lane where the ballot is not empty -- integer sums, the same bits in any order.
#include "common.hpp"

namespace prcnn {

constexpr int OS_THREADS = 256;
constexpr int OS_CHUNK = 16;                     // boxes per LDS chunk (16 x OS_REC doubles = 1152 bytes)
constexpr int OS_REC = 9;                        // X, Y, Z, h, l / 2, w / 2, cos, sin, factor

__global__ __launch_bounds__(OS_THREADS) void object_scale_kernel(int n, int g, float *__restrict__ pts, float *__restrict__ extra, int ec,
                                                                  const float *__restrict__ gt, const int *__restrict__ counts,
                                                                  const float *__restrict__ trig, const double *__restrict__ factors,
                                                                  unsigned int *__restrict__ hits)
{
    __shared__ double sbox[OS_CHUNK * OS_REC];
    const int s = blockIdx.y;
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    const bool live = i < n;
    const long row = (long)s * n + i;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = pts[3 * row]; fy = pts[3 * row + 1]; fz = pts[3 * row + 2]; }
    const double px = fx, py = fy, pz = fz;
    const int nb = min(max(counts[s], 0), g);
    const long box0 = (long)s * g;
    bool owned = false;
    double oa = 0.0, ob = 0.0, ov = 0.0, oX = 0.0, oY = 0.0, oZ = 0.0, oc = 1.0, os = 0.0, orr = 1.0;
    for (int k0 = 0; k0 < nb; k0 += OS_CHUNK) {
        const int kn = min(OS_CHUNK, nb - k0);
        __syncthreads();
        if ((int)threadIdx.x < kn) {
            const long k = box0 + k0 + threadIdx.x;
            double *r = sbox + threadIdx.x * OS_REC;
            r[0] = gt[7 * k]; r[1] = gt[7 * k + 1]; r[2] = gt[7 * k + 2]; r[3] = gt[7 * k + 3];
            r[4] = (double)gt[7 * k + 5] * 0.5; r[5] = (double)gt[7 * k + 4] * 0.5;
            r[6] = trig[2 * k]; r[7] = trig[2 * k + 1]; r[8] = factors[k];
        }
        __syncthreads();
        for (int kk = 0; kk < kn; ++kk) {
            if (!__any(live && !owned)) break;                  // the whole wave has its owners: nothing left to test or to count
            const double *r = sbox + kk * OS_REC;
            bool in = false;
            if (live && !owned) {
                const double dx = px - r[0], dz = pz - r[2], v = r[1] - py;
                const double a = dx * r[6] - dz * r[7], b = dx * r[7] + dz * r[6];
                in = fabs(a) <= r[4] && fabs(b) <= r[5] && 0.0 <= v && v <= r[3];
                if (in) {
                    owned = true;
                    oa = a; ob = b; ov = v; oX = r[0]; oY = r[1]; oZ = r[2]; oc = r[6]; os = r[7]; orr = r[8];
                }
            }
            const unsigned long long m = __ballot(in);
            if (m && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(hits + box0 + k0 + kk, (unsigned int)__popcll(m));
        }
    }
    if (owned && orr != 1.0) {
        const double a2 = oa * orr, b2 = ob * orr, v2 = ov * orr;
        const float nx = (float)(oX + (a2 * oc + b2 * os));
        const float ny = (float)(oY - v2);
        const float nz = (float)(oZ + (b2 * oc - a2 * os));
        pts[3 * row] = nx; pts[3 * row + 1] = ny; pts[3 * row + 2] = nz;
        if (extra) {
            float *e = extra + (long)ec * row;
            e[0] = nx; e[1] = ny; e[2] = nz;
        }
    }
}
}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_object_scale(int b, int n, int g, float *pts, float *extra, int extra_channels, const float *gt, const int *counts,
                                  const float *trig, const double *factors, unsigned int *hits, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && g >= 0, "object_scale: bad sizes");
    PRCNN_REQUIRE((long long)b * n < (1ll << 31) / 4 && (long long)b * g < (1 << 24) && b <= 65535, "object_scale: batch too large");
    PRCNN_REQUIRE(!extra || extra_channels == 3 || extra_channels == 4, "object_scale: extra has 3 or 4 channels");
    if (b == 0 || n == 0 || g == 0) return PRCNN_OK;
    PRCNN_REQUIRE(pts && gt && counts && trig && factors && hits, "object_scale: null pointer");
    hipLaunchKernelGGL(object_scale_kernel, dim3((unsigned)((n + OS_THREADS - 1) / OS_THREADS), (unsigned)b), dim3(OS_THREADS), 0,
                       (hipStream_t)stream, n, g, pts, extra, extra_channels, gt, counts, trig, factors, hits);
    return check_launch("object_scale");
}
