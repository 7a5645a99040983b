// rpn_labels.hip -- per-point RPN labels (lib/datasets/kitti_rcnn_dataset.py:385-414 generate_rpn_training_labels) and the
// segmentation counters of eval_one_epoch_rpn (tools/eval_rcnn.py:205-209) for a batch of ragged scenes.
//
// Two passes:
//   prep    one thread per (scene, box): the 8 corners of the box and of its enlarged box (kitti_utils.boxes3d_to_corners3d /
//           enlarge_box3d(0.2)) in f32 in numpy's order, then each hull's 12 facet planes in f64 (RL_REC doubles per box);
//   label   one thread per point, the scene's boxes staged through LDS in chunks of RL_CHUNK and visited in order k = 0..G-1
//           (a later box overrides an earlier one): inside k -> 1 and reg = (center - pt, h, w, l, ry);
//           inside k xor inside enlarged k -> -1.  Then (correct, fg, pred) per wave, one atomic each per wave.
// "Inside" is the reference's Delaunay(corners).find_simplex(p) >= 0: the point lies in the convex hull of the 8 corners, a boundary
// point counts as inside.  Each quad face of the box is split along the diagonal whose two triangles are both supporting planes of
// the 8 corners (f32 rounding can bend a rotated face), and p is inside when n . (p - a) <= 100 eps * H for all 12 triangles, H the
// largest inward distance of a corner (find_simplex's barycentric tolerance).  A box whose hull is flat (QhullError) is empty.
// Corner arithmetic: x' = x cos + z sin, z' = x (-sin) + z cos, a product per term and one add (np.matmul of (8,3) @ (3,3) f32,
// pinned by tests/golden g16); cos / sin of ry come from the host (numpy's f32 trig is not the correctly rounded one).
// rpn_eval.py's numpy path restates every operation in the same order; all of it is compiled with -ffp-contract=off.
#include "common.hpp"
#include <math.h>
#include <algorithm>

namespace prcnn {

constexpr int RL_THREADS = 256;
constexpr int RL_CHUNK = 16;                     // boxes per LDS chunk (16 x RL_REC doubles = 23.5 KiB)
constexpr int RL_PLANE = 7;                      // nx, ny, nz, ax, ay, az, tol
constexpr int RL_NPL = 12;                       // facet triangles per hull
// per-box f64 record: label values, hull validity, cheap reject (both hulls), the two hulls' planes
constexpr int RL_PAR = 0, RL_VALID = 7, RL_REJ = 9, RL_HULL0 = 14, RL_HULL1 = RL_HULL0 + RL_NPL * RL_PLANE, RL_REC = 184;
static_assert(RL_HULL1 + RL_NPL * RL_PLANE <= RL_REC, "record layout");

__constant__ int c_faces[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};

// corners of [x, y, z, h, w, l] turned by (c, s), boxes3d_to_corners3d(rotate=True) (kitti_utils.py:66-101)
__device__ __forceinline__ void box_corners(float x, float y, float z, float h, float w, float l, float c, float s, double out[8][3])
{
    const float l2 = __fdiv_rn(l, 2.0f), w2 = __fdiv_rn(w, 2.0f);
    const float sx[8] = {1.f, 1.f, -1.f, -1.f, 1.f, 1.f, -1.f, -1.f}, sz[8] = {1.f, -1.f, -1.f, 1.f, 1.f, -1.f, -1.f, 1.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xc = __fmul_rn(l2, sx[j]), zc = __fmul_rn(w2, sz[j]);
        const float xr = __fadd_rn(__fmul_rn(xc, c), __fmul_rn(zc, s));
        const float zr = __fadd_rn(__fmul_rn(xc, -s), __fmul_rn(zc, c));
        out[j][0] = (double)__fadd_rn(x, xr);
        out[j][1] = (double)(j < 4 ? y : __fadd_rn(y, -h));
        out[j][2] = (double)__fadd_rn(z, zr);
    }
}

// plane of triangle (a, b, c) oriented outward with its tolerance; false if some corner lies on each side
__device__ __forceinline__ bool facet(const double P[8][3], int ia, int ib, int ic, double *pl)
{
    const double *a = P[ia];
    const double e1x = P[ib][0] - a[0], e1y = P[ib][1] - a[1], e1z = P[ib][2] - a[2];
    const double e2x = P[ic][0] - a[0], e2y = P[ic][1] - a[1], e2z = P[ic][2] - a[2];
    double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    double smin = 0.0, smax = 0.0;
    for (int j = 0; j < 8; ++j) {
        const double v = (nx * (P[j][0] - a[0]) + ny * (P[j][1] - a[1])) + nz * (P[j][2] - a[2]);
        smin = fmin(smin, v);
        smax = fmax(smax, v);
    }
    double H;
    if (smax <= 0.0) {
        H = -smin;
    } else if (smin >= 0.0) {
        nx = -nx; ny = -ny; nz = -nz;
        H = smax;
    } else {
        H = -1.0;
    }
    pl[0] = nx; pl[1] = ny; pl[2] = nz; pl[3] = a[0]; pl[4] = a[1]; pl[5] = a[2];
    pl[6] = (100.0 * 2.220446049250313e-16) * (H > 0.0 ? H : 0.0);
    return H >= 0.0;
}

// 12 facet planes of one hull -> rec; returns 1 when the hull has volume (no facet with all corners in its plane)
__device__ int hull_planes(const double P[8][3], double *rec)
{
    int valid = 1;
    for (int f = 0; f < 6; ++f) {
        const int q0 = c_faces[f][0], q1 = c_faces[f][1], q2 = c_faces[f][2], q3 = c_faces[f][3];
        double *p0 = rec + (2 * f) * RL_PLANE, *p1 = rec + (2 * f + 1) * RL_PLANE;
        const bool a0 = facet(P, q0, q1, q2, p0);
        const bool a1 = facet(P, q0, q2, q3, p1);
        if (!(a0 && a1)) {
            facet(P, q0, q1, q3, p0);
            facet(P, q1, q2, q3, p1);
        }
        valid &= (p0[6] > 0.0) & (p1[6] > 0.0);
    }
    return valid;
}

__global__ __launch_bounds__(64) void rpn_labels_prep_kernel(int b, int g, const float *__restrict__ gt, const int *__restrict__ counts,
                                                             const float *__restrict__ trig, double *__restrict__ rec)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= b * g) return;
    const int s = i / g, k = i - s * g;
    if (k >= min(counts[s], g)) return;
    const float *bx = gt + (long)i * 7;
    const float x = bx[0], y = bx[1], z = bx[2], h = bx[3], w = bx[4], l = bx[5], ry = bx[6];
    const float c = trig[2 * (long)i], sn = trig[2 * (long)i + 1];
    double *r = rec + (long)i * RL_REC;
    // label values: center3d[1] -= h / 2 (f32), then h, w, l, ry
    r[RL_PAR + 0] = x; r[RL_PAR + 1] = __fsub_rn(y, __fdiv_rn(h, 2.0f)); r[RL_PAR + 2] = z;
    r[RL_PAR + 3] = h; r[RL_PAR + 4] = w; r[RL_PAR + 5] = l; r[RL_PAR + 6] = ry;
    double P[8][3], Q[8][3];
    box_corners(x, y, z, h, w, l, c, sn, P);
    // enlarge_box3d(extra_width=0.2): h, w, l += 0.4 and y += 0.2 in f32
    box_corners(x, __fadd_rn(y, 0.2f), z, __fadd_rn(h, 0.4f), __fadd_rn(w, 0.4f), __fadd_rn(l, 0.4f), c, sn, Q);
    r[RL_VALID] = hull_planes(P, r + RL_HULL0);
    r[RL_VALID + 1] = hull_planes(Q, r + RL_HULL1);
    // cheap reject: y range and bounding circle about (x, z) of all 16 corners, padded far beyond any rounding
    double ylo = P[0][1], yhi = P[0][1], r2 = 0.0;
    for (int j = 0; j < 8; ++j) {
        ylo = fmin(ylo, fmin(P[j][1], Q[j][1]));
        yhi = fmax(yhi, fmax(P[j][1], Q[j][1]));
        const double dx = P[j][0] - x, dz = P[j][2] - z, ex = Q[j][0] - x, ez = Q[j][2] - z;
        r2 = fmax(r2, fmax(dx * dx + dz * dz, ex * ex + ez * ez));
    }
    const double pad = 1e-3 + 1e-6 * (fabs((double)x) + fabs((double)y) + fabs((double)z));
    const double rr = sqrt(r2) + pad;
    r[RL_REJ + 0] = ylo - pad; r[RL_REJ + 1] = yhi + pad; r[RL_REJ + 2] = x; r[RL_REJ + 3] = z; r[RL_REJ + 4] = rr * rr;
}

__device__ __forceinline__ bool in_hull(const double *pl, double px, double py, double pz)
{
    bool in = true;
#pragma unroll
    for (int q = 0; q < RL_NPL; ++q, pl += RL_PLANE) {
        const double v = (pl[0] * (px - pl[3]) + pl[1] * (py - pl[4])) + pl[2] * (pz - pl[5]);
        in = in && (v <= pl[6]);
    }
    return in;
}

__global__ __launch_bounds__(RL_THREADS) void rpn_labels_kernel(int n, int g, const float *__restrict__ pts, const int *__restrict__ counts,
                                                                const double *__restrict__ rec, const float *__restrict__ scores,
                                                                float thresh, int *__restrict__ cls, float *__restrict__ reg,
                                                                int *__restrict__ stats)
{
    __shared__ double sbox[RL_CHUNK * RL_REC];
    const int s = blockIdx.y;
    const int i = blockIdx.x * RL_THREADS + threadIdx.x;
    const bool live = i < n;
    const long row = (long)s * n + i;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    if (live) { fx = pts[3 * row]; fy = pts[3 * row + 1]; fz = pts[3 * row + 2]; }
    const double px = fx, py = fy, pz = fz;
    int label = 0;
    float rg[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int nb = min(counts[s], g);
    const double *srec = rec + (long)s * g * RL_REC;
    for (int k0 = 0; k0 < nb; k0 += RL_CHUNK) {
        const int kn = min(RL_CHUNK, nb - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < kn * RL_REC; e += RL_THREADS) sbox[e] = srec[(long)k0 * RL_REC + e];
        __syncthreads();
        if (!live) continue;
        for (int kk = 0; kk < kn; ++kk) {
            const double *r = sbox + kk * RL_REC;
            const double dx = px - r[RL_REJ + 2], dz = pz - r[RL_REJ + 3];
            if (py < r[RL_REJ] || py > r[RL_REJ + 1] || dx * dx + dz * dz > r[RL_REJ + 4]) continue;
            const bool in0 = r[RL_VALID] != 0.0 && in_hull(r + RL_HULL0, px, py, pz);
            const bool in1 = r[RL_VALID + 1] != 0.0 && in_hull(r + RL_HULL1, px, py, pz);
            if (in0) {
                label = 1;
                rg[0] = __fsub_rn((float)r[RL_PAR + 0], fx);
                rg[1] = __fsub_rn((float)r[RL_PAR + 1], fy);
                rg[2] = __fsub_rn((float)r[RL_PAR + 2], fz);
#pragma unroll
                for (int q = 3; q < 7; ++q) rg[q] = (float)r[RL_PAR + q];
            }
            if (in0 != in1) label = -1;
        }
    }
    if (live) {
        cls[row] = label;
        if (reg) {
#pragma unroll
            for (int q = 0; q < 7; ++q) reg[7 * row + q] = rg[q];
        }
    }
    if (stats) {
        const bool pred = live && scores && rpn_seg_fg(scores[row], thresh);
        const bool fg = live && label > 0;
        const unsigned long long mc = __ballot(pred && fg), mf = __ballot(fg), mp = __ballot(pred);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
            if (mc) atomicAdd(stats + 3 * s + 0, __popcll(mc));
            if (mf) atomicAdd(stats + 3 * s + 1, __popcll(mf));
            if (mp) atomicAdd(stats + 3 * s + 2, __popcll(mp));
        }
    }
}
}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_rpn_labels_workspace(int b, int g, long long *bytes)
{
    PRCNN_REQUIRE(b >= 0 && g >= 0 && bytes, "rpn_labels_workspace: bad arguments");
    *bytes = (long long)b * g * RL_REC * (long long)sizeof(double);
    return PRCNN_OK;
}

extern "C" int prcnn_rpn_labels(int b, int n, int g, const float *pts, const float *gt, const int *counts, const float *trig,
                                const float *scores, float thresh, int *cls, float *reg, int *stats, double *work, void *stream)
{
    PRCNN_REQUIRE(b >= 0 && n >= 0 && g >= 0, "rpn_labels: bad sizes");
    PRCNN_REQUIRE((long long)b * n < (1ll << 31) / 7 && (long long)b * g < (1 << 24) && b <= 65535, "rpn_labels: batch too large");
    if (b == 0 || n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(pts && counts && cls, "rpn_labels: null pointer");
    PRCNN_REQUIRE(g == 0 || (gt && trig && work), "rpn_labels: null box pointer");
    hipStream_t st = (hipStream_t)stream;
    if (g > 0) hipLaunchKernelGGL(rpn_labels_prep_kernel, dim3((unsigned)((b * g + 63) / 64)), dim3(64), 0, st, b, g, gt, counts, trig, work);
    hipLaunchKernelGGL(rpn_labels_kernel, dim3((unsigned)((n + RL_THREADS - 1) / RL_THREADS), (unsigned)b), dim3(RL_THREADS), 0, st, n, g,
                       pts, counts, work, scores, thresh, cls, reg, stats);
    return check_launch("rpn_labels");
}
