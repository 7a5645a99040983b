// kitti_ap.hip -- the statistics of the KITTI AP evaluator on the device (evaluate/eval2.py:8-349, 460-569): ignore flags,
// image-box and 3D overlaps in f64, both greedy matching passes, the recall thresholds and the PR sums of a whole split,
// for every (difficulty, overlap level) group of one class at once.  The host path (kitti_stats.hip + kitti_eval.py) is the
// definition; every stage here gives its bits:
//   * flags and overlaps are the host's IEEE operations in the host's order (the library is built without contraction);
//   * both passes run the ONE scan of kitti_match.hpp that the host entries run;
//   * tp / fp / fn are integers (integer atomics: order cannot change an integer sum);
//   * the orientation similarity adds host-made cosine terms (prcnn_kitti_pair_cos) in ground-truth order per image, and the
//     per-image sums in image order per (group, threshold) -- no floating-point atomic anywhere.
// No kernel waits on another; every loop is bounded by an image's n_gt x n_dt (or by the image count in the last reduction).
#include "common.hpp"
#include "kitti_match.hpp"

namespace prcnn {

constexpr int AP_SAMPLE_PTS = PRCNN_AP_SAMPLE_PTS;
constexpr int AP_REG_DETS = PRCNN_AP_REG_DETS;      // detections per image whose scan flags stay in two 64-bit registers
constexpr int AP_MAX_DIFF = 8;

// the split table (include/prcnn_hip.h: the PRCNN_AP_* words), as the kernels take it by value
struct ApSplit {
    int n_img, max_dt;
    long long n_gt, n_dt, n_dc, n_pair;
    const long long *gt_off, *dt_off, *dc_off, *pair_off;
    const int *ws_slot;
    const signed char *gt_code, *dt_code;
    const double *gt_occluded, *gt_truncated, *gt_bbox, *gt_depth, *gt_box3d;
    const double *dt_bbox, *dt_depth, *dt_score, *dt_box3d;
    const double *dc_bbox;
    const float *gt_bev, *dt_bev;
};

struct FlagCaps {
    double max_occ[AP_MAX_DIFF], max_trunc[AP_MAX_DIFF], lo[AP_MAX_DIFF], hi[AP_MAX_DIFF], min_height[AP_MAX_DIFF];
};

// clean_data (eval2.py:28-98; eval_old.py:28-91 with metric_old) for every row of the split and every difficulty
__global__ __launch_bounds__(256) void ap_flags_kernel(ApSplit sp, int cls, int sibling, int metric_old, int n_diff,
                                                       FlagCaps caps, signed char *__restrict__ ignored_gt,
                                                       signed char *__restrict__ ignored_dt, int *__restrict__ num_valid)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < sp.n_gt) {
        const int code = sp.gt_code[e];
        const bool own = code == cls, sib = code == sibling;
        const double occ = sp.gt_occluded[e], trunc = sp.gt_truncated[e], depth = sp.gt_depth[e];
        const double height = sp.gt_bbox[4 * e + 3] - sp.gt_bbox[4 * e + 1];
        for (int d = 0; d < n_diff; ++d) {
            const bool capped = (occ > caps.max_occ[d]) | (trunc > caps.max_trunc[d]) |
                                (metric_old ? (height <= caps.min_height[d]) : !((caps.lo[d] < depth) & (depth < caps.hi[d])));
            const int flag = (sib || (own && capped)) ? 1 : (own ? 0 : -1);
            ignored_gt[(long long)d * sp.n_gt + e] = (signed char)flag;
            if (flag == 0) atomicAdd(num_valid + d, 1);
        }
    } else if (e < sp.n_gt + sp.n_dt) {
        const long long j = e - sp.n_gt;
        const bool own = sp.dt_code[j] == cls;
        const double depth = sp.dt_depth[j];
        const double height = fabs(sp.dt_bbox[4 * j + 3] - sp.dt_bbox[4 * j + 1]);
        for (int d = 0; d < n_diff; ++d) {
            const bool in_band = metric_old ? !(height < caps.min_height[d]) : ((caps.lo[d] < depth) & (depth < caps.hi[d]));
            ignored_dt[(long long)d * sp.n_dt + j] = (signed char)(in_band ? (own ? 0 : -1) : 1);
        }
    }
}

// last image whose first pair is <= e (images without pairs share their offset with the next one and are skipped)
__device__ __forceinline__ int image_of_pair(const long long *__restrict__ pair_off, int n_img, long long e)
{
    int lo = 0, hi = n_img;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// kind 0: image_box_overlap(dt bbox, gt bbox, -1) (eval2.py:102-128); kind 2: the f64 step of d3_box_overlap (eval2.py:136-161)
// on the f32 raw BEV intersection `rinc` of the segmented rotated-IoU launch (criterion 2).  Operation order as kitti_eval.py.
__global__ __launch_bounds__(256) void ap_overlaps_kernel(ApSplit sp, int kind, const float *__restrict__ rinc,
                                                          double *__restrict__ out)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= sp.n_pair) return;
    const int m = image_of_pair(sp.pair_off, sp.n_img, e);
    const long long local = e - sp.pair_off[m];
    const long long ng = sp.gt_off[m + 1] - sp.gt_off[m];
    const long long j = sp.dt_off[m] + local / ng, i = sp.gt_off[m] + local % ng;
    if (kind == 0) {
        const double *b = sp.dt_bbox + 4 * j, *q = sp.gt_bbox + 4 * i;
        const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
        const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
        const double barea = (b[2] - b[0]) * (b[3] - b[1]);
        const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
        const double inter = iw * ih;
        const double ua = barea + qarea - inter;
        out[e] = (iw > 0 && ih > 0) ? inter / ua : 0.0;
    } else {
        const double *b = sp.dt_box3d + 7 * j, *q = sp.gt_box3d + 7 * i;      // x y z l h w ry
        const double r = (double)rinc[e];
        const double iw = fmin(b[1], q[1]) - fmax(b[1] - b[4], q[1] - q[4]);
        const double area1 = b[3] * b[4] * b[5];
        const double area2 = q[3] * q[4] * q[5];
        const double inc = iw * r;
        const double val = inc / (area1 + area2 - inc);
        out[e] = r > 0 ? (iw > 0 ? val : 0.0) : r;
    }
}

// one image's columns in the split table, for one difficulty
struct SplitView {
    const double *overlaps, *dt_score, *dt_bbox, *dc_bbox;
    const signed char *ig, *id;
    long long n_gt;
    __device__ int ignored_gt(int i) const { return ig[i]; }
    __device__ int ignored_det(int j) const { return id[j]; }
    __device__ double score(int j) const { return dt_score[j]; }
    __device__ double overlap(int j, int i) const { return overlaps[(long long)j * n_gt + i]; }
    __device__ const double *det_box(int j) const { return dt_bbox + 4 * j; }
    __device__ const double *dc_box(int i) const { return dc_bbox + 4 * i; }
};

// the scan's per-detection flags: two register words up to AP_REG_DETS detections, else words of the caller's workspace
// (word w at glob[w * stride])
struct ScanBits {
    unsigned long long r0, r1;
    unsigned long long *glob;
    long long stride;
    __device__ void clear(int n_dt)
    {
        r0 = r1 = 0;
        if (glob)
            for (int w = 0; w < (n_dt + 63) / 64; ++w) glob[w * stride] = 0;
    }
    __device__ bool get(int j) const
    {
        const unsigned long long w = glob ? glob[(j >> 6) * stride] : (j < 64 ? r0 : r1);
        return (w >> (j & 63)) & 1ull;
    }
    __device__ void set(int j)
    {
        const unsigned long long bit = 1ull << (j & 63);
        if (glob) glob[(j >> 6) * stride] |= bit;
        else if (j < 64) r0 |= bit;
        else r1 |= bit;
    }
};

__device__ __forceinline__ SplitView view_of(const ApSplit &sp, int m, int d, const signed char *ignored_gt,
                                               const signed char *ignored_dt, const double *overlaps)
{
    SplitView v;
    v.overlaps = overlaps + sp.pair_off[m];
    v.dt_score = sp.dt_score + sp.dt_off[m];
    v.dt_bbox = sp.dt_bbox + 4 * sp.dt_off[m];
    v.dc_bbox = sp.dc_bbox + 4 * sp.dc_off[m];
    v.ig = ignored_gt + (long long)d * sp.n_gt + sp.gt_off[m];
    v.id = ignored_dt + (long long)d * sp.n_dt + sp.dt_off[m];
    v.n_gt = sp.gt_off[m + 1] - sp.gt_off[m];
    return v;
}

// Pass 1 (eval2.py:512-527): one thread per (image, group); group = difficulty * n_lev + level.  The matched detection's score goes
// to the slot of its ground-truth box in the group's row; every slot of the image is written (-inf and mark 0 when unmatched).
__global__ __launch_bounds__(256) void ap_scores_kernel(ApSplit sp, const signed char *__restrict__ ignored_gt,
                                                        const signed char *__restrict__ ignored_dt, int n_diff, int n_lev,
                                                        const double *__restrict__ min_overlaps,
                                                        const double *__restrict__ overlaps, int kind,
                                                        double *__restrict__ scores, signed char *__restrict__ valid,
                                                        unsigned long long *__restrict__ ws, long long ws_words)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int G = n_diff * n_lev;
    if (t >= (long long)sp.n_img * G) return;
    const int m = (int)(t / G), g = (int)(t % G);
    const SplitView v = view_of(sp, m, g / n_lev, ignored_gt, ignored_dt, overlaps);
    const int n_gt = (int)v.n_gt, n_dt = (int)(sp.dt_off[m + 1] - sp.dt_off[m]);
    double *row = scores + (long long)g * sp.n_gt + sp.gt_off[m];
    signed char *mark = valid + (long long)g * sp.n_gt + sp.gt_off[m];
    for (int i = 0; i < n_gt; ++i) {
        row[i] = -INFINITY;
        mark[i] = 0;
    }
    ScanBits assigned, below;
    assigned.glob = below.glob = nullptr;
    assigned.stride = below.stride = 1;
    if (n_dt > AP_REG_DETS) assigned.glob = ws + ((long long)sp.ws_slot[m] * G + g) * ws_words;
    assigned.clear(n_dt);
    below.clear(0);
    match_image(v, n_gt, n_dt, 0, kind, min_overlaps[g % n_lev], false, assigned, below, [&](int i, int det_idx) {
        row[i] = v.score(det_idx);
        mark[i] = 1;
    });
}

// get_thresholds (eval2.py:8-25), the loop as written: one thread per group over its descending row.  At most AP_SAMPLE_PTS
// values are stored; n_thr counts all the loop takes, so the caller sees it if a row ever took more.
__global__ __launch_bounds__(64) void ap_thresholds_kernel(int G, int n_lev, long long n_gt_total,
                                                           const double *__restrict__ sorted, const int *__restrict__ count,
                                                           const int *__restrict__ num_valid,
                                                           double *__restrict__ thresholds, int *__restrict__ n_thr)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    const int n = count[g];
    const double num_gt = (double)num_valid[g / n_lev];
    const double *s = sorted + (long long)g * n_gt_total;
    double current_recall = 0.0;
    int taken = 0;
    for (int i = 0; i < n; ++i) {
        const double l_recall = (double)(i + 1) / num_gt;
        const double r_recall = i < n - 1 ? (double)(i + 2) / num_gt : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
        if (taken < AP_SAMPLE_PTS) thresholds[g * AP_SAMPLE_PTS + taken] = s[i];
        taken += 1;
        current_recall += 1 / (AP_SAMPLE_PTS - 1.0);
    }
    for (int k = taken; k < AP_SAMPLE_PTS; ++k) thresholds[g * AP_SAMPLE_PTS + k] = 0.0;
    n_thr[g] = taken;
}

// Pass 2 (fused_compute_statistics, eval2.py:300-349): one wave per (image, group), lane = threshold index.  The lanes share the
// loop bounds and the pair values; only the branch outcomes differ.
__global__ __launch_bounds__(256) void ap_pr_kernel(ApSplit sp, const signed char *__restrict__ ignored_gt,
                                                    const signed char *__restrict__ ignored_dt, int n_diff, int n_lev,
                                                    const double *__restrict__ min_overlaps,
                                                    const double *__restrict__ overlaps, int kind,
                                                    const double *__restrict__ thresholds, const int *__restrict__ n_thr,
                                                    const double *__restrict__ pair_cos,
                                                    unsigned long long *__restrict__ counts, double *__restrict__ sim_img,
                                                    unsigned long long *__restrict__ ws, long long ws_words)
{
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = lane_id();
    const int G = n_diff * n_lev;
    if (wave >= (long long)sp.n_img * G) return;
    const int m = (int)(wave / G), g = (int)(wave % G);
    if (lane >= AP_SAMPLE_PTS) return;
    double *sim_out = sim_img ? sim_img + ((long long)m * G + g) * AP_SAMPLE_PTS + lane : nullptr;
    if (lane >= n_thr[g]) {
        if (sim_out) *sim_out = -1.0;
        return;
    }
    const double thresh = thresholds[g * AP_SAMPLE_PTS + lane];
    const SplitView v = view_of(sp, m, g / n_lev, ignored_gt, ignored_dt, overlaps);
    const int n_gt = (int)v.n_gt, n_dt = (int)(sp.dt_off[m + 1] - sp.dt_off[m]), n_dc = (int)(sp.dc_off[m + 1] - sp.dc_off[m]);
    ScanBits assigned, below;
    assigned.glob = below.glob = nullptr;
    assigned.stride = below.stride = 64;
    if (n_dt > AP_REG_DETS) {
        assigned.glob = ws + ((long long)sp.ws_slot[m] * G + g) * 2 * ws_words * 64 + lane;
        below.glob = assigned.glob + ws_words * 64;
    }
    assigned.clear(n_dt);
    below.clear(n_dt);
    for (int j = 0; j < n_dt; ++j)
        if (v.score(j) < thresh) below.set(j);
    const double *cosv = pair_cos ? pair_cos + sp.pair_off[m] : nullptr;
    double sim = 0.0;
    const MatchCounts c = match_image(v, n_gt, n_dt, n_dc, kind, min_overlaps[g % n_lev], true, assigned, below,
                                      [&](int i, int det_idx) {
                                          if (cosv) sim += cosv[(long long)det_idx * n_gt + i];
                                      });
    unsigned long long *cnt = counts + ((long long)g * AP_SAMPLE_PTS + lane) * 3;
    if (c.tp) atomicAdd(cnt + 0, (unsigned long long)c.tp);
    if (c.fp) atomicAdd(cnt + 1, (unsigned long long)c.fp);
    if (c.fn) atomicAdd(cnt + 2, (unsigned long long)c.fn);
    if (sim_out) *sim_out = (c.tp > 0 || c.fp > 0) ? sim : -1.0;
}

// pr (G, 41, 4) f64 = [tp, fp, fn, similarity]: the integer sums widened, the per-image similarities added in image order
__global__ __launch_bounds__(64) void ap_finish_kernel(int n_img, int G, const unsigned long long *__restrict__ counts,
                                                       const double *__restrict__ sim_img, double *__restrict__ pr)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= G * AP_SAMPLE_PTS) return;
    double s = 0.0;
    if (sim_img)
        for (int m = 0; m < n_img; ++m) {
            const double x = sim_img[(long long)m * G * AP_SAMPLE_PTS + e];
            if (x != -1) s += x;
        }
    pr[4 * e + 0] = (double)(long long)counts[3 * e + 0];
    pr[4 * e + 1] = (double)(long long)counts[3 * e + 1];
    pr[4 * e + 2] = (double)(long long)counts[3 * e + 2];
    pr[4 * e + 3] = s;
}

// HOST words -> ApSplit; false when a count is negative or a column that has rows is missing
static bool load_split(const long long *w, ApSplit *sp)
{
    if (!w) return false;
    auto at = [&](int k) { return (const void *)(uintptr_t)w[k]; };
    sp->n_img = (int)w[PRCNN_AP_N_IMG]; sp->max_dt = (int)w[PRCNN_AP_MAX_DT];
    sp->n_gt = w[PRCNN_AP_N_GT]; sp->n_dt = w[PRCNN_AP_N_DT]; sp->n_dc = w[PRCNN_AP_N_DC]; sp->n_pair = w[PRCNN_AP_N_PAIR];
    sp->gt_off = (const long long *)at(PRCNN_AP_GT_OFF); sp->dt_off = (const long long *)at(PRCNN_AP_DT_OFF);
    sp->dc_off = (const long long *)at(PRCNN_AP_DC_OFF); sp->pair_off = (const long long *)at(PRCNN_AP_PAIR_OFF);
    sp->ws_slot = (const int *)at(PRCNN_AP_WS_SLOT);
    sp->gt_code = (const signed char *)at(PRCNN_AP_GT_CODE); sp->dt_code = (const signed char *)at(PRCNN_AP_DT_CODE);
    sp->gt_occluded = (const double *)at(PRCNN_AP_GT_OCCLUDED); sp->gt_truncated = (const double *)at(PRCNN_AP_GT_TRUNCATED);
    sp->gt_bbox = (const double *)at(PRCNN_AP_GT_BBOX); sp->gt_depth = (const double *)at(PRCNN_AP_GT_DEPTH);
    sp->gt_box3d = (const double *)at(PRCNN_AP_GT_BOX3D);
    sp->dt_bbox = (const double *)at(PRCNN_AP_DT_BBOX); sp->dt_depth = (const double *)at(PRCNN_AP_DT_DEPTH);
    sp->dt_score = (const double *)at(PRCNN_AP_DT_SCORE); sp->dt_box3d = (const double *)at(PRCNN_AP_DT_BOX3D);
    sp->dc_bbox = (const double *)at(PRCNN_AP_DC_BBOX);
    sp->gt_bev = (const float *)at(PRCNN_AP_GT_BEV); sp->dt_bev = (const float *)at(PRCNN_AP_DT_BEV);
    if (w[PRCNN_AP_N_IMG] < 0 || w[PRCNN_AP_N_IMG] > 0x7fffffff || w[PRCNN_AP_MAX_DT] < 0 || w[PRCNN_AP_MAX_DT] > 0x7fffffff) return false;
    if (sp->n_gt < 0 || sp->n_dt < 0 || sp->n_dc < 0 || sp->n_pair < 0) return false;
    if (sp->n_img > 0 && !(sp->gt_off && sp->dt_off && sp->dc_off && sp->pair_off && sp->ws_slot)) return false;
    if (sp->n_gt > 0 && !(sp->gt_code && sp->gt_occluded && sp->gt_truncated && sp->gt_bbox && sp->gt_depth)) return false;
    if (sp->n_dt > 0 && !(sp->dt_code && sp->dt_bbox && sp->dt_depth && sp->dt_score)) return false;
    return sp->n_dc == 0 || sp->dc_bbox;
}

// words of workspace one scan flag set needs (0: every image fits the registers)
static long long scan_words(const ApSplit *sp) { return sp->max_dt > AP_REG_DETS ? (sp->max_dt + 63) / 64 : 0; }

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_ap_flags(const long long *split_words, int cls, int sibling, int metric_old, int n_diff, const double *caps,
                              char *ignored_gt, char *ignored_dt, int *num_valid_gt, void *stream)
{
    ApSplit table, *split = &table;
    PRCNN_REQUIRE(load_split(split_words, split), "ap_flags: bad split table");
    PRCNN_REQUIRE(n_diff >= 1 && n_diff <= AP_MAX_DIFF && caps && num_valid_gt, "ap_flags: %d difficulties not in 1..%d, or null", n_diff, AP_MAX_DIFF);
    PRCNN_REQUIRE((split->n_gt == 0 || ignored_gt) && (split->n_dt == 0 || ignored_dt), "ap_flags: null output");
    FlagCaps c;
    for (int d = 0; d < n_diff; ++d) {
        c.max_occ[d] = caps[5 * d + 0]; c.max_trunc[d] = caps[5 * d + 1]; c.lo[d] = caps[5 * d + 2]; c.hi[d] = caps[5 * d + 3];
        c.min_height[d] = caps[5 * d + 4];
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(num_valid_gt, 0, sizeof(int) * n_diff, st) != hipSuccess) {
        set_error("ap_flags: clearing the counters failed");
        return PRCNN_EINVAL;
    }
    const long long rows = split->n_gt + split->n_dt;
    if (rows == 0) return PRCNN_OK;
    PRCNN_REQUIRE(rows <= 0x7fffffffLL * 256, "ap_flags: %lld rows exceed the launch grid", rows);
    hipLaunchKernelGGL(ap_flags_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *split, cls, sibling, metric_old,
                       n_diff, c, (signed char *)ignored_gt, (signed char *)ignored_dt, num_valid_gt);
    return check_launch("ap_flags");
}

extern "C" int prcnn_ap_overlaps(const long long *split_words, int kind, const float *rinc, double *out, void *stream)
{
    ApSplit table, *split = &table;
    PRCNN_REQUIRE(load_split(split_words, split), "ap_overlaps: bad split table");
    PRCNN_REQUIRE(kind == 0 || kind == 2, "ap_overlaps: kind %d is neither 0 (image box) nor 2 (3D)", kind);
    if (split->n_pair == 0) return PRCNN_OK;
    PRCNN_REQUIRE(out && (kind == 0 || (rinc && split->gt_box3d && split->dt_box3d)), "ap_overlaps: null pointer");
    PRCNN_REQUIRE(split->n_pair <= 0x7fffffffLL * 256, "ap_overlaps: %lld pairs exceed the launch grid", split->n_pair);
    hipLaunchKernelGGL(ap_overlaps_kernel, dim3((unsigned)((split->n_pair + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *split,
                       kind, rinc, out);
    return check_launch("ap_overlaps");
}

extern "C" int prcnn_ap_scores(const long long *split_words, const char *ignored_gt, const char *ignored_dt, int n_diff, int n_lev,
                               const double *min_overlaps, const double *overlaps, int kind, double *scores, char *valid,
                               unsigned long long *workspace, long long workspace_words, void *stream)
{
    ApSplit table, *split = &table;
    PRCNN_REQUIRE(load_split(split_words, split), "ap_scores: bad split table");
    PRCNN_REQUIRE(n_diff >= 1 && n_lev >= 1 && (long long)n_diff * n_lev <= 0x7fffffff / AP_SAMPLE_PTS / 4 && min_overlaps, "ap_scores: bad groups");
    PRCNN_REQUIRE(kind >= 0 && kind <= 2, "ap_scores: kind %d not in 0..2", kind);
    const long long G = (long long)n_diff * n_lev, threads = split->n_img * G;
    if (threads == 0 || split->n_gt == 0) return PRCNN_OK;
    PRCNN_REQUIRE(ignored_gt && scores && valid && (split->n_dt == 0 || ignored_dt) && (split->n_pair == 0 || overlaps), "ap_scores: null pointer");
    PRCNN_REQUIRE(scan_words(split) == 0 || (workspace && workspace_words >= scan_words(split)),
                  "ap_scores: an image has %d detections (> %d): the workspace needs %lld words per (large image, group)", split->max_dt,
                  AP_REG_DETS, scan_words(split));
    PRCNN_REQUIRE(threads <= 0x7fffffffLL * 256, "ap_scores: %lld scans exceed the launch grid", threads);
    hipLaunchKernelGGL(ap_scores_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *split,
                       (const signed char *)ignored_gt, (const signed char *)ignored_dt, n_diff, n_lev, min_overlaps, overlaps, kind,
                       scores, (signed char *)valid, workspace, workspace_words);
    return check_launch("ap_scores");
}

extern "C" int prcnn_ap_thresholds(int n_groups, int n_lev, long long n_gt_total, const double *sorted_scores, const int *count,
                                   const int *num_valid_gt, double *thresholds, int *n_thr, void *stream)
{
    PRCNN_REQUIRE(n_groups >= 0 && n_lev >= 1 && n_gt_total >= 0, "ap_thresholds: bad sizes");
    if (n_groups == 0) return PRCNN_OK;
    PRCNN_REQUIRE(count && num_valid_gt && thresholds && n_thr && (n_gt_total == 0 || sorted_scores), "ap_thresholds: null pointer");
    hipLaunchKernelGGL(ap_thresholds_kernel, dim3((unsigned)((n_groups + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n_groups, n_lev,
                       n_gt_total, sorted_scores, count, num_valid_gt, thresholds, n_thr);
    return check_launch("ap_thresholds");
}

extern "C" int prcnn_ap_pr(const long long *split_words, const char *ignored_gt, const char *ignored_dt, int n_diff, int n_lev,
                           const double *min_overlaps, const double *overlaps, int kind, const double *thresholds, const int *n_thr,
                           const double *pair_cos, unsigned long long *counts, double *sim_img, double *pr,
                           unsigned long long *workspace, long long workspace_words, void *stream)
{
    ApSplit table, *split = &table;
    PRCNN_REQUIRE(load_split(split_words, split), "ap_pr: bad split table");
    PRCNN_REQUIRE(n_diff >= 1 && n_lev >= 1 && (long long)n_diff * n_lev <= 0x7fffffff / AP_SAMPLE_PTS / 4 && min_overlaps, "ap_pr: bad groups");
    PRCNN_REQUIRE(kind >= 0 && kind <= 2, "ap_pr: kind %d not in 0..2", kind);
    PRCNN_REQUIRE(thresholds && n_thr && counts && pr, "ap_pr: null pointer");
    PRCNN_REQUIRE((pair_cos == nullptr) == (sim_img == nullptr) || split->n_pair == 0, "ap_pr: pair_cos and sim_img go together");
    const int G = n_diff * n_lev;
    const long long waves = (long long)split->n_img * G;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 3 * AP_SAMPLE_PTS * G, st) != hipSuccess) {
        set_error("ap_pr: clearing the counters failed");
        return PRCNN_EINVAL;
    }
    if (waves > 0) {
        PRCNN_REQUIRE((split->n_gt == 0 || ignored_gt) && (split->n_dt == 0 || ignored_dt) && (split->n_pair == 0 || overlaps), "ap_pr: null pointer");
        PRCNN_REQUIRE(scan_words(split) == 0 || (workspace && workspace_words >= scan_words(split)),
                      "ap_pr: an image has %d detections (> %d): the workspace needs 2 x 64 x %lld words per (large image, group)",
                      split->max_dt, AP_REG_DETS, scan_words(split));
        PRCNN_REQUIRE(waves <= 0x7fffffffLL * 4, "ap_pr: %lld scans exceed the launch grid", waves);
        hipLaunchKernelGGL(ap_pr_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, *split, (const signed char *)ignored_gt,
                           (const signed char *)ignored_dt, n_diff, n_lev, min_overlaps, overlaps, kind, thresholds, n_thr,
                           sim_img ? pair_cos : nullptr, counts, sim_img, workspace, workspace_words);
        const int rc = check_launch("ap_pr");
        if (rc != PRCNN_OK) return rc;
    }
    hipLaunchKernelGGL(ap_finish_kernel, dim3((unsigned)((G * AP_SAMPLE_PTS + 63) / 64)), dim3(64), 0, st, split->n_img, G, counts,
                       sim_img, pr);
    return check_launch("ap_finish");
}
