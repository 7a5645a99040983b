// losses.hip -- the training losses of both stages with their gradients (lib/net/train_functions.py get_rpn_loss / get_rcnn_loss,
// lib/utils/loss_utils.py DiceLoss / SigmoidFocalClassificationLoss / get_reg_loss): prcnn_loss_stats, prcnn_cls_loss, prcnn_reg_loss
// (include/prcnn_hip.h; losses.py).  Four launches per stage, no host read between them:
//   loss_stats_kernel   one pass over the labels (and, for Dice, the logits): counts and the two Dice sums -> per-block partials
//   cls_loss_kernel     elementwise: every block re-reduces the stats partials (<= 512 rows, fixed order), then value terms and grad_cls
//   reg_loss_kernel     16 lanes per row of the (n, c) prediction: bin labels, log-sum-exp cross-entropies, smooth-L1 terms, grad_reg
//   loss_finish_kernel  one block: all partials in a fixed order -> parts
// The rule of this unit: DECISIONS (bin labels, the fold of the fine heading, BCE's f32 sigmoid with its clamps) are taken in f32 by the
// reference's own operation sequence; the ARITHMETIC on top of them and every sum run in f64 and are rounded to f32 once.  Sums go through
// per-thread accumulators (fixed loop order), a butterfly over the wave, four LDS words and per-block partials: no atomics anywhere, so
// the same input gives the same bits.  A kernel boundary, not a fence, makes the partials visible to the next stage.
#include "common.hpp"
#include <math.h>

namespace prcnn {
namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_ELEM_BLOCKS = 512;     // stats / cls grids
constexpr int LS_MAX_ROW_BLOCKS = 1024;     // reg grid
constexpr int LS_LANES = 16;                // lanes per regression row
constexpr int LS_COLS = 5;                  // columns per lane: c <= 80
constexpr int LS_NSTAT = 6;                 // pos, neg, valid, reg fg, dice min, dice max
constexpr int LS_NCLS = 3;                  // sum, its positive part, its negative part
constexpr int LS_NREG = 10;                 // x_bin z_bin x_res z_res y_bin y_res y_offset ry_bin ry_res size (sum over rows of the 3 terms)
constexpr int LS_OFF_CLS = LS_MAX_ELEM_BLOCKS * LS_NSTAT;
constexpr int LS_OFF_REG = LS_OFF_CLS + LS_MAX_ELEM_BLOCKS * LS_NCLS;
constexpr int LS_WORK = LS_OFF_REG + LS_MAX_ROW_BLOCKS * LS_NREG;

static inline int elem_blocks(int n) { return max(1, min(LS_MAX_ELEM_BLOCKS, ceil_div(n, LS_THREADS * 4))); }
static inline int row_blocks(int n) { return max(1, min(LS_MAX_ROW_BLOCKS, ceil_div(n, (LS_THREADS / LS_LANES) * 8))); }

// the block's sum of K values per thread, in every thread: butterfly over the wave (a + b == b + a bit for bit, so every lane holds
// the same value), then the four waves' sums in wave order
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *sm)
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, WAVE);
    }
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sm[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((sm[k] + sm[K + k]) + sm[2 * K + k]) + sm[3 * K + k];
    __syncthreads();
}

// rows of `rows` x K partials (written by an earlier launch) -> their sum in every thread
template <int K>
__device__ __forceinline__ void sum_partials(const double *part, int rows, double (&v)[K], double *sm)
{
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int b = threadIdx.x; b < rows; b += LS_THREADS) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[(long)b * K + k];
    }
    block_sum<K>(v, sm);
}

__device__ __forceinline__ double sigmoid64(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

__global__ void __launch_bounds__(LS_THREADS) loss_stats_kernel(const prcnn_loss_args a)
{
    __shared__ double sm[4 * LS_NSTAT];
    double s[LS_NSTAT] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * LS_THREADS + threadIdx.x; i < a.n; i += (long)gridDim.x * LS_THREADS) {
        const long long lab = a.label[i];
        s[0] += lab > 0 ? 1.0 : 0.0;
        s[1] += lab == 0 ? 1.0 : 0.0;
        s[2] += lab >= 0 ? 1.0 : 0.0;
        const bool fg = a.reg_mask ? a.reg_mask[i] > 0 : lab > 0;
        s[3] += fg ? 1.0 : 0.0;
        if (a.cls_kind == PRCNN_LOSS_DICE && lab != -1) {                   // DiceLoss: mask = (target != ignore_target)
            const double p = sigmoid64(a.cls[i]), t = (double)lab;
            s[4] += fmin(p, t);
            s[5] += fmax(p, t);
        }
    }
    block_sum<LS_NSTAT>(s, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < LS_NSTAT; ++k) a.work[(long)blockIdx.x * LS_NSTAT + k] = s[k];
    }
}

__global__ void __launch_bounds__(LS_THREADS) cls_loss_kernel(const prcnn_loss_args a, const int stat_rows)
{
    __shared__ double sm[4 * LS_NSTAT];
    double st[LS_NSTAT];
    sum_partials<LS_NSTAT>(a.work, stat_rows, st, sm);
    const double inv_pos = 1.0 / fmax(st[0], 1.0), inv_valid = 1.0 / fmax(st[2], 1.0);
    // Dice: loss = 1 - I / clamp(U, min = 1); clamp's backward passes the gradient where U >= 1
    const double uc = fmax(st[5], 1.0), d_i = -1.0 / uc, d_u = st[5] >= 1.0 ? st[4] / (uc * uc) : 0.0;
    const double gamma = (double)a.gamma, alpha = (double)a.alpha;
    double s[LS_NCLS] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * LS_THREADS + threadIdx.x; i < a.n; i += (long)gridDim.x * LS_THREADS) {
        const long long lab = a.label[i];
        double g = 0.0;
        if (a.cls_kind == PRCNN_LOSS_DICE ? lab != -1 : lab >= 0) {       // an ignored entry's logit is never read
            const float x = a.cls[i];
            const bool t = lab > 0;
            if (a.cls_kind == PRCNN_LOSS_FOCAL) {
                // _sigmoid_cross_entropy_with_logits' stable form clamp(x, min=0) - x t + log1p(exp(-|x|)) and ITS derivative (at x == 0
                // clamp's backward gives 1 and |x|'s gives 0: 1 - t there, not 1/2 - t)
                const double xd = (double)x, e = exp(-fabs(xd)), r = e / (1.0 + e);
                const double ce = fmax(xd, 0.0) - (t ? xd : 0.0) + log1p(e);
                const double dce = (xd >= 0.0 ? 1.0 : 0.0) - (t ? 1.0 : 0.0) - (xd > 0.0 ? r : (xd < 0.0 ? -r : 0.0));
                const double p = xd >= 0.0 ? 1.0 / (1.0 + e) : r;
                const double om = t ? 1.0 - p : p;                          // 1 - p_t
                const double at = t ? alpha : 1.0 - alpha;
                double mod = 1.0, dmod = 0.0;
                if (gamma != 0.0) {
                    mod = pow(om, gamma);
                    if (om > 0.0 || gamma >= 1.0) dmod = gamma * pow(om, gamma - 1.0) * (t ? -1.0 : 1.0) * p * (1.0 - p);
                }
                const double l = mod * at * ce * inv_pos;
                g = at * inv_pos * (dmod * ce + mod * dce);
                s[0] += l;
                s[t ? 1 : 2] += l;
            } else if (a.cls_kind == PRCNN_LOSS_BCE) {
                // F.binary_cross_entropy(torch.sigmoid(x), t, weight): the f32 sigmoid 1 / (1 + exp(-x)) saturates, log(p) and log1p(-p) are
                // clamped at -100, the backward divides by max((1 - p) p, 1e-12) and sigmoid's backward multiplies by (1 - p) p
                const float e32 = (float)exp(-(double)x);
                const float p32 = __fdiv_rn(1.0f, __fadd_rn(1.0f, e32)), q32 = __fsub_rn(1.0f, p32);
                const double w = t ? (double)a.fg_weight : 1.0;
                const double lp = fmax(t ? log((double)p32) : log1p(-(double)p32), -100.0);    // torch: log(p) and log1p(-p)
                const float pq32 = __fmul_rn(q32, p32);
                s[0] += -w * lp;
                g = w * ((double)p32 - (t ? 1.0 : 0.0)) / (double)fmaxf(pq32, 1e-12f) * (double)pq32 * inv_valid;
            } else {
                // torch.min / torch.max split the gradient on a tie; sigmoid's backward multiplies by p (1 - p)
                const double p = sigmoid64(x), tl = (double)lab;
                const double dmin = p < tl ? 1.0 : (p == tl ? 0.5 : 0.0), dmax = p > tl ? 1.0 : (p == tl ? 0.5 : 0.0);
                g = (d_i * dmin + d_u * dmax) * p * (1.0 - p);
            }
        }
        a.grad_cls[i] = (float)(g * (double)a.w_cls);
    }
    block_sum<LS_NCLS>(s, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < LS_NCLS; ++k) a.work[LS_OFF_CLS + (long)blockIdx.x * LS_NCLS + k] = s[k];
    }
}

// Python's % on f32 as torch's remainder kernel computes it: fmod, then + b where the signs differ
__device__ __forceinline__ float pymod_f32(float v, float b)
{
    float m = fmodf(v, b);
    if (m != 0.0f && ((b < 0.0f) != (m < 0.0f))) m = __fadd_rn(m, b);
    return m;
}
__device__ __forceinline__ double pymod_f64(double v, double b)
{
    double m = fmod(v, b);
    if (m != 0.0 && ((b < 0.0) != (m < 0.0))) m += b;
    return m;
}

// clamp(offset + scope, 0, 2 scope - 1e-3) -> floor(shift / bin) decided in f32; the shift itself in f64 for the residual
__device__ __forceinline__ int loc_bin_label(float off, float scope, float bin, int nbin, double *shift64)
{
    const float hi32 = (float)((double)scope * 2.0 - 1e-3);
    const float shift32 = fminf(fmaxf(__fadd_rn(off, scope), 0.0f), hi32);
    *shift64 = fmin(fmax((double)off + (double)scope, 0.0), (double)scope * 2.0 - 1e-3);
    const int b = (int)floorf(__fdiv_rn(shift32, bin));
    return min(max(b, 0), nbin - 1);                                       // (a label outside the group raises in the reference)
}

__device__ __forceinline__ double smooth_l1(double d, double *slope)
{
    const double ad = fabs(d);
    if (ad < 1.0) {
        *slope = d;
        return 0.5 * d * d;
    }
    *slope = d > 0.0 ? 1.0 : -1.0;
    return ad - 0.5;
}

struct RowCtx {
    int l16;
    double scale;
    double v[LS_COLS];
    double g[LS_COLS];
};

template <typename F>
__device__ __forceinline__ double group_reduce(double x, F f)
{
#pragma unroll
    for (int off = LS_LANES / 2; off >= 1; off >>= 1) x = f(x, __shfl_xor(x, off, LS_LANES));
    return x;
}

// cross-entropy lse - logit[label] of the bin group [l, l + nb) against label b, added to *acc in two pieces (the lane that owns the
// label's column subtracts the logit, the group's first lane adds the log-sum-exp: the block's sum joins them); leaves
// (softmax - one-hot) x scale in the group's gradient columns
__device__ __forceinline__ void bin_ce(RowCtx &r, int l, int nb, int b, double *acc)
{
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LS_COLS; ++k) {
        const int col = r.l16 + LS_LANES * k;
        if (col >= l && col < l + nb) m = fmax(m, r.v[k]);
    }
    m = group_reduce(m, [](double x, double y) { return fmax(x, y); });
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LS_COLS; ++k) {
        const int col = r.l16 + LS_LANES * k;
        if (col >= l && col < l + nb) s += exp(r.v[k] - m);
    }
    s = group_reduce(s, [](double x, double y) { return x + y; });
    const double lse = m + log(s);
#pragma unroll
    for (int k = 0; k < LS_COLS; ++k) {
        const int col = r.l16 + LS_LANES * k;
        if (col >= l && col < l + nb) {
            const bool hit = col == l + b;
            if (hit) *acc -= r.v[k];
            r.g[k] = (exp(r.v[k] - lse) - (hit ? 1.0 : 0.0)) * r.scale;
        }
    }
    if (r.l16 == 0) *acc += lse;
}

// smooth-L1 of the logit at column `col` against `target`: the owning lane returns the term and sets its gradient column
__device__ __forceinline__ double pick_sl1(RowCtx &r, int col, double target)
{
    double loss = 0.0;
#pragma unroll
    for (int k = 0; k < LS_COLS; ++k) {
        if (r.l16 + LS_LANES * k == col) {
            double slope;
            loss = smooth_l1(r.v[k] - target, &slope);
            r.g[k] = slope * r.scale;
        }
    }
    return loss;
}

__global__ void __launch_bounds__(LS_THREADS) reg_loss_kernel(const prcnn_loss_args a, const int stat_rows)
{
    __shared__ double sm[4 * LS_NREG];
    double st[LS_NSTAT];
    sum_partials<LS_NSTAT>(a.work, stat_rows, st, sm);
    RowCtx r;
    r.l16 = threadIdx.x & (LS_LANES - 1);
    // every term is a mean over the fg rows (the size term over 3 fg elements, then x 3), weighted by the stage's regression weight
    r.scale = (double)a.w_reg / fmax(st[3], 1.0);
    const int grp = threadIdx.x / LS_LANES, c = a.c, nb = a.nbin_loc;
    int off = a.xz_fine ? 4 * nb : 2 * nb;
    const int y_l = off;
    off += a.y_by_bin ? 2 * a.nbin_y : 1;
    const int ry_l = off, sz_l = off + 2 * a.nbin_head;
    double comp[LS_NREG];
#pragma unroll
    for (int k = 0; k < LS_NREG; ++k) comp[k] = 0.0;

    for (long row = (long)blockIdx.x * (LS_THREADS / LS_LANES) + grp; row < a.n; row += (long)gridDim.x * (LS_THREADS / LS_LANES)) {
        const bool fg = a.reg_mask ? a.reg_mask[row] > 0 : a.label[row] > 0;
        float *gout = a.grad_reg + row * c;
        if (!fg) {                                                          // zeros, and the prediction row is never read
#pragma unroll
            for (int k = 0; k < LS_COLS; ++k) {
                const int col = r.l16 + LS_LANES * k;
                if (col < c) gout[col] = 0.0f;
            }
            continue;
        }
        const float *pred = a.reg + row * c;
#pragma unroll
        for (int k = 0; k < LS_COLS; ++k) {
            const int col = r.l16 + LS_LANES * k;
            r.v[k] = col < c ? (double)pred[col] : 0.0;
            r.g[k] = 0.0;
        }
        const float *lab = a.reg_label + row * 7;
        double shift;
        // x, z
        const int xb = loc_bin_label(lab[0], a.loc_scope, a.loc_bin, nb, &shift);
        bin_ce(r, 0, nb, xb, &comp[0]);
        const double x_res = (shift - ((double)xb * (double)a.loc_bin + (double)a.loc_bin / 2.0)) / (double)a.loc_bin;
        const int zb = loc_bin_label(lab[2], a.loc_scope, a.loc_bin, nb, &shift);
        bin_ce(r, nb, nb, zb, &comp[1]);
        const double z_res = (shift - ((double)zb * (double)a.loc_bin + (double)a.loc_bin / 2.0)) / (double)a.loc_bin;
        if (a.xz_fine) {
            comp[2] += pick_sl1(r, 2 * nb + xb, x_res);
            comp[3] += pick_sl1(r, 3 * nb + zb, z_res);
        }
        // y
        if (a.y_by_bin) {
            const int yb = loc_bin_label(lab[1], a.y_scope, a.y_bin, a.nbin_y, &shift);
            bin_ce(r, y_l, a.nbin_y, yb, &comp[4]);
            const double y_res = (shift - ((double)yb * (double)a.y_bin + (double)a.y_bin / 2.0)) / (double)a.y_bin;
            comp[5] += pick_sl1(r, y_l + a.nbin_y + yb, y_res);
        } else {
            comp[6] += pick_sl1(r, y_l, (double)lab[1]);
        }
        // heading: the f32 chain decides (fold, wraps, bin); the f64 chain gives the residual unless a wrap fell differently in it
        const double two_pi = 2.0 * M_PI;
        const float two_pi32 = (float)two_pi;
        float shift32;
        double shift64, apc;
        if (a.ry_fine) {
            apc = (M_PI / 2.0) / (double)a.nbin_head;
            float ry32 = pymod_f32(lab[6], two_pi32);
            double ry64 = pymod_f64((double)lab[6], two_pi);
            if (ry32 > (float)(M_PI * 0.5) && ry32 < (float)(M_PI * 1.5)) {
                ry32 = pymod_f32(__fadd_rn(ry32, (float)M_PI), two_pi32);
                ry64 = pymod_f64(ry64 + M_PI, two_pi);
            }
            shift32 = pymod_f32(__fadd_rn(ry32, (float)(M_PI * 0.5)), two_pi32);
            shift32 = fminf(fmaxf(__fsub_rn(shift32, (float)(M_PI * 0.25)), (float)1e-3), (float)(M_PI * 0.5 - 1e-3));
            shift64 = pymod_f64(ry64 + M_PI * 0.5, two_pi);
            shift64 = fmin(fmax(shift64 - M_PI * 0.25, 1e-3), M_PI * 0.5 - 1e-3);
        } else {
            apc = two_pi / (double)a.nbin_head;
            const float h32 = pymod_f32(lab[6], two_pi32);
            shift32 = pymod_f32(__fadd_rn(h32, (float)(apc / 2.0)), two_pi32);
            shift64 = pymod_f64(pymod_f64((double)lab[6], two_pi) + apc / 2.0, two_pi);
        }
        if (fabs(shift64 - (double)shift32) > 1e-4) shift64 = (double)shift32;
        const int rb = min(max((int)floorf(__fdiv_rn(shift32, (float)apc)), 0), a.nbin_head - 1);
        bin_ce(r, ry_l, a.nbin_head, rb, &comp[7]);
        const double ry_res = (shift64 - ((double)rb * apc + apc / 2.0)) / (apc / 2.0);
        comp[8] += pick_sl1(r, ry_l + a.nbin_head + rb, ry_res);
        // size
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double anc = a.anchors ? (double)a.anchors[row * 7 + 3 + j] : (double)a.anchor[j];
            comp[9] += pick_sl1(r, sz_l + j, ((double)lab[3 + j] - anc) / anc);
        }
#pragma unroll
        for (int k = 0; k < LS_COLS; ++k) {
            const int col = r.l16 + LS_LANES * k;
            if (col < c) gout[col] = (float)r.g[k];
        }
    }
    block_sum<LS_NREG>(comp, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < LS_NREG; ++k) a.work[LS_OFF_REG + (long)blockIdx.x * LS_NREG + k] = comp[k];
    }
}

__global__ void __launch_bounds__(LS_THREADS) loss_finish_kernel(const prcnn_loss_args a, const int stat_rows, const int cls_rows, const int reg_rows)
{
    __shared__ double sm[4 * LS_NREG];
    double st[LS_NSTAT], cl[LS_NCLS], rg[LS_NREG];
    sum_partials<LS_NSTAT>(a.work, stat_rows, st, sm);
    sum_partials<LS_NCLS>(a.work + LS_OFF_CLS, cls_rows, cl, sm);
    sum_partials<LS_NREG>(a.work + LS_OFF_REG, reg_rows, rg, sm);
    if (threadIdx.x != 0) return;
    double cls = 0.0, cls_pos = 0.0, cls_neg = 0.0;
    if (a.cls_kind == PRCNN_LOSS_DICE) {
        cls = 1.0 - st[4] / fmax(st[5], 1.0);
    } else if (a.cls_kind == PRCNN_LOSS_FOCAL) {
        cls = cl[0];
        cls_pos = cl[1];
        cls_neg = cl[2];
    } else {
        cls = cl[0] / fmax(st[2], 1.0);
    }
    const double inv_fg = 1.0 / fmax(st[3], 1.0);                            // no fg row: every sum is 0 and so is every term
    double t[LS_NREG];
#pragma unroll
    for (int k = 0; k < LS_NREG; ++k) t[k] = rg[k] * inv_fg;
    const double size_raw = t[9] / 3.0;
    const double loc = t[0] + t[1] + t[2] + t[3] + t[4] + t[5] + t[6], angle = t[7] + t[8], size = 3.0 * size_raw;
    const double reg = loc + angle + size;
    float *o = a.parts;
    o[PRCNN_LP_LOSS] = (float)(cls * (double)a.w_cls + reg * (double)a.w_reg);
    o[PRCNN_LP_CLS] = (float)cls;
    o[PRCNN_LP_REG] = (float)reg;
    o[PRCNN_LP_LOC] = (float)loc;
    o[PRCNN_LP_ANGLE] = (float)angle;
    o[PRCNN_LP_SIZE] = (float)size;
    o[PRCNN_LP_CLS_POS] = (float)cls_pos;
    o[PRCNN_LP_CLS_NEG] = (float)cls_neg;
    o[PRCNN_LP_X_BIN] = (float)t[0];
    o[PRCNN_LP_Z_BIN] = (float)t[1];
    o[PRCNN_LP_X_RES] = (float)t[2];
    o[PRCNN_LP_Z_RES] = (float)t[3];
    o[PRCNN_LP_Y_BIN] = (float)t[4];
    o[PRCNN_LP_Y_RES] = (float)t[5];
    o[PRCNN_LP_Y_OFFSET] = (float)t[6];
    o[PRCNN_LP_RY_BIN] = (float)t[7];
    o[PRCNN_LP_RY_RES] = (float)t[8];
    o[PRCNN_LP_SIZE_RAW] = (float)size_raw;
    o[PRCNN_LP_N_POS] = (float)st[0];
    o[PRCNN_LP_N_NEG] = (float)st[1];
    o[PRCNN_LP_N_VALID] = (float)st[2];
    o[PRCNN_LP_N_REG_FG] = (float)st[3];
    o[PRCNN_LP_DICE_MIN] = (float)st[4];
    o[PRCNN_LP_DICE_MAX] = (float)st[5];
}

int check_args(const prcnn_loss_args *a, const char *what)
{
    PRCNN_REQUIRE(a, "%s: null pointer", what);
    PRCNN_REQUIRE(a->n >= 1 && a->n <= (1 << 24), "%s: n = %d (1 .. 2^24: the counts are carried in f32)", what, a->n);
    PRCNN_REQUIRE(a->cls_kind >= PRCNN_LOSS_DICE && a->cls_kind <= PRCNN_LOSS_BCE, "%s: cls_kind %d", what, a->cls_kind);
    PRCNN_REQUIRE(a->nbin_loc >= 1 && a->nbin_head >= 1 && (!a->y_by_bin || a->nbin_y >= 1), "%s: bin counts %d %d %d", what, a->nbin_loc,
                  a->nbin_y, a->nbin_head);
    const int c = a->nbin_loc * (a->xz_fine ? 4 : 2) + (a->y_by_bin ? 2 * a->nbin_y : 1) + 2 * a->nbin_head + 3;
    PRCNN_REQUIRE(a->c == c, "%s: %d regression channels, the configuration needs %d", what, a->c, c);
    PRCNN_REQUIRE(c <= LS_LANES * LS_COLS, "%s: %d regression channels (at most %d)", what, c, LS_LANES * LS_COLS);
    PRCNN_REQUIRE((long long)a->n * c < (1LL << 31), "%s: n x c too large", what);
    PRCNN_REQUIRE(a->loc_bin > 0.f && a->loc_scope > 0.f && (!a->y_by_bin || (a->y_bin > 0.f && a->y_scope > 0.f)), "%s: scopes / bin sizes", what);
    PRCNN_REQUIRE(a->anchors || (a->anchor[0] > 0.f && a->anchor[1] > 0.f && a->anchor[2] > 0.f), "%s: anchor size", what);
    PRCNN_REQUIRE(a->cls && a->label && a->reg && a->reg_label && a->grad_cls && a->grad_reg && a->parts && a->work, "%s: null pointer", what);
    return PRCNN_OK;
}

}  // namespace
}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_loss_workspace(void) { return LS_WORK; }

extern "C" int prcnn_loss_stats(const prcnn_loss_args *a, void *stream)
{
    const int rc = check_args(a, "loss_stats");
    if (rc != PRCNN_OK) return rc;
    hipLaunchKernelGGL(loss_stats_kernel, dim3(elem_blocks(a->n)), dim3(LS_THREADS), 0, (hipStream_t)stream, *a);
    return check_launch("loss_stats");
}

extern "C" int prcnn_cls_loss(const prcnn_loss_args *a, void *stream)
{
    const int rc = check_args(a, "cls_loss");
    if (rc != PRCNN_OK) return rc;
    hipLaunchKernelGGL(cls_loss_kernel, dim3(elem_blocks(a->n)), dim3(LS_THREADS), 0, (hipStream_t)stream, *a, elem_blocks(a->n));
    return check_launch("cls_loss");
}

extern "C" int prcnn_reg_loss(const prcnn_loss_args *a, void *stream)
{
    const int rc = check_args(a, "reg_loss");
    if (rc != PRCNN_OK) return rc;
    const int eb = elem_blocks(a->n), rb = row_blocks(a->n);
    hipLaunchKernelGGL(reg_loss_kernel, dim3(rb), dim3(LS_THREADS), 0, (hipStream_t)stream, *a, eb);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LS_THREADS), 0, (hipStream_t)stream, *a, eb, eb, rb);
    return check_launch("reg_loss");
}
