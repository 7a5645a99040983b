// kitti_stats.hip -- host side of the KITTI AP evaluator: the per-image greedy matching and the
// precision/recall accumulation (evaluate/eval2.py:170-349; numba CPU jit in the reference), plus the
// segmented launch of the rotated-IoU kernel that replaces the reference's 50 "parts".
//
// Host code only (no device kernels here): the matching is a short sequential scan per image with
// data-dependent control flow -- it stays on the CPU in the reference too -- but it is called
// images x difficulties x overlap levels x 42 times per metric, so it lives in the library instead of
// a Python loop.  All arithmetic is f64, as numba types it from the f64 label arrays.  The scan itself is
// kitti_match.hpp, shared with the device form of these statistics (kitti_ap.hip), whose definition this file is.
#include "common.hpp"
#include "kitti_match.hpp"
#include <math.h>
#include <vector>

namespace prcnn {

// one true positive's orientation term; prcnn_kitti_pair_cos fills the device path's table with this same call
static double pair_cos_term(double delta) { return (1.0 + cos(delta)) / 2.0; }


struct ImageStats {
    long long tp, fp, fn;
    double similarity;
    int n_thresholds;
};

// one image's columns as the host entries take them
struct HostView {
    const double *overlaps, *dt_datas, *dc_bboxes;
    const long long *ig, *id;
    int n_gt;
    int ignored_gt(int i) const { return (int)ig[i]; }
    int ignored_det(int j) const { return (int)id[j]; }
    double score(int j) const { return dt_datas[6 * j + 5]; }
    double overlap(int j, int i) const { return overlaps[(size_t)j * n_gt + i]; }
    const double *det_box(int j) const { return dt_datas + 6 * j; }
    const double *dc_box(int i) const { return dc_bboxes + 4 * i; }
};

struct HostBits {
    std::vector<char> &b;
    bool get(int j) const { return b[j] != 0; }
    void set(int j) { b[j] = 1; }
};

// compute_statistics_jit (eval2.py:170-289) around the shared scan (kitti_match.hpp).  overlaps is (n_dt, n_gt) row-major;
// gt_datas (n_gt,5) = [bbox x4, alpha]; dt_datas (n_dt,6) = [bbox x4, alpha, score]; thresholds_out has room for n_gt values.
static ImageStats image_stats(int n_gt, int n_dt, int n_dc, const double *overlaps, const double *gt_datas,
                              const double *dt_datas, const long long *ignored_gt, const long long *ignored_det,
                              const double *dc_bboxes, int metric, double min_overlap, double thresh, bool compute_fp,
                              bool compute_aos, double *thresholds_out, std::vector<char> &assigned,
                              std::vector<char> &below, std::vector<double> &delta)
{
    assigned.assign((size_t)n_dt, 0);
    below.assign((size_t)n_dt, 0);
    delta.clear();
    if (compute_fp)
        for (int j = 0; j < n_dt; ++j) below[j] = dt_datas[6 * j + 5] < thresh;
    const HostView view = {overlaps, dt_datas, dc_bboxes, ignored_gt, ignored_det, n_gt};
    HostBits abits = {assigned};
    const HostBits bbits = {below};
    ImageStats st = {0, 0, 0, 0.0, 0};
    const MatchCounts c = match_image(view, n_gt, n_dt, n_dc, metric, min_overlap, compute_fp, abits, bbits, [&](int i, int det_idx) {
        if (thresholds_out) thresholds_out[st.n_thresholds] = dt_datas[6 * det_idx + 5];
        st.n_thresholds += 1;
        if (compute_aos) delta.push_back(gt_datas[5 * i + 4] - dt_datas[6 * det_idx + 4]);
    });
    st.tp = c.tp; st.fp = c.fp; st.fn = c.fn;
    if (compute_fp && compute_aos) {
        if (st.tp > 0 || st.fp > 0) {
            double s = 0.0;   // fp zeros first, then (1 + cos(delta)) / 2 per true positive, summed in that order
            for (double d : delta) s += pair_cos_term(d);
            st.similarity = s;
        } else {
            st.similarity = -1;
        }
    }
    return st;
}

}  // namespace prcnn

using namespace prcnn;

extern "C" int prcnn_kitti_image_stats(int n_gt, int n_dt, int n_dc, const double *overlaps, const double *gt_datas,
                                       const double *dt_datas, const long long *ignored_gt, const long long *ignored_det,
                                       const double *dc_bboxes, int metric, double min_overlap, double thresh,
                                       int compute_fp, int compute_aos, long long *tp_fp_fn, double *similarity,
                                       double *thresholds, int *n_thresholds)
{
    PRCNN_REQUIRE(n_gt >= 0 && n_dt >= 0 && n_dc >= 0, "kitti_image_stats: bad sizes");
    PRCNN_REQUIRE(tp_fp_fn && similarity && n_thresholds, "kitti_image_stats: null output");
    PRCNN_REQUIRE((n_gt == 0 || (gt_datas && ignored_gt && thresholds)) && (n_dt == 0 || (dt_datas && ignored_det)) &&
                      (n_gt == 0 || n_dt == 0 || overlaps) && (n_dc == 0 || dc_bboxes),
                  "kitti_image_stats: null input");
    std::vector<char> assigned, below;
    std::vector<double> delta;
    const ImageStats st = image_stats(n_gt, n_dt, n_dc, overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes,
                                      metric, min_overlap, thresh, compute_fp != 0, compute_aos != 0, thresholds, assigned,
                                      below, delta);
    tp_fp_fn[0] = st.tp; tp_fp_fn[1] = st.fp; tp_fp_fn[2] = st.fn;
    *similarity = st.similarity;
    *n_thresholds = st.n_thresholds;
    return PRCNN_OK;
}

// First pass of eval_class (eval2.py:512-527): scores of the matched detections of every image
// (compute_fp = False, thresh = 0), concatenated into scores_out (room for sum(gt_nums)); *n_scores = count.
extern "C" int prcnn_kitti_collect_scores(int n_img, const long long *gt_nums, const long long *dt_nums,
                                          const double *overlaps_flat, const double *gt_datas, const double *dt_datas,
                                          const long long *ignored_gts, const long long *ignored_dets, int metric,
                                          double min_overlap, double *scores_out, long long *n_scores)
{
    PRCNN_REQUIRE(n_img >= 0 && n_scores, "kitti_collect_scores: bad arguments");
    std::vector<char> assigned, below;
    std::vector<double> delta;
    size_t gt0 = 0, dt0 = 0, ov0 = 0;
    long long total = 0;
    for (int i = 0; i < n_img; ++i) {
        const int ng = (int)gt_nums[i], nd = (int)dt_nums[i];
        const ImageStats st = image_stats(ng, nd, 0, overlaps_flat + ov0, gt_datas + 5 * gt0, dt_datas + 6 * dt0,
                                          ignored_gts + gt0, ignored_dets + dt0, nullptr, metric, min_overlap, 0.0, false,
                                          false, scores_out + total, assigned, below, delta);
        total += st.n_thresholds;
        gt0 += ng; dt0 += nd; ov0 += (size_t)ng * nd;
    }
    *n_scores = total;
    return PRCNN_OK;
}

// fused_compute_statistics (eval2.py:300-349) over all images: pr (n_thresh, 4) += [tp, fp, fn, similarity].
extern "C" int prcnn_kitti_accumulate_pr(int n_img, const long long *gt_nums, const long long *dt_nums,
                                         const long long *dc_nums, const double *overlaps_flat, const double *gt_datas,
                                         const double *dt_datas, const double *dontcares, const long long *ignored_gts,
                                         const long long *ignored_dets, int metric, double min_overlap,
                                         const double *thresholds, int n_thresh, int compute_aos, double *pr)
{
    PRCNN_REQUIRE(n_img >= 0 && n_thresh >= 0 && (n_thresh == 0 || (thresholds && pr)), "kitti_accumulate_pr: bad arguments");
    std::vector<char> assigned, below;
    std::vector<double> delta, scratch;
    size_t gt0 = 0, dt0 = 0, dc0 = 0, ov0 = 0;
    for (int i = 0; i < n_img; ++i) {
        const int ng = (int)gt_nums[i], nd = (int)dt_nums[i], nc = (int)dc_nums[i];
        scratch.resize((size_t)ng + 1);
        for (int t = 0; t < n_thresh; ++t) {
            const ImageStats st = image_stats(ng, nd, nc, overlaps_flat + ov0, gt_datas + 5 * gt0, dt_datas + 6 * dt0,
                                              ignored_gts + gt0, ignored_dets + dt0, dontcares + 4 * dc0, metric, min_overlap,
                                              thresholds[t], true, compute_aos != 0, scratch.data(), assigned, below, delta);
            pr[4 * t + 0] += (double)st.tp;
            pr[4 * t + 1] += (double)st.fp;
            pr[4 * t + 2] += (double)st.fn;
            if (st.similarity != -1) pr[4 * t + 3] += st.similarity;
        }
        gt0 += ng; dt0 += nd; dc0 += nc; ov0 += (size_t)ng * nd;
    }
    return PRCNN_OK;
}

// (1 + cos(gt alpha - dt alpha)) / 2 of every (detection, ground-truth) pair of every image, in the overlap blocks' layout
// (pair_off[img] + j * n_gt + i).  HOST pointers.  The device pass adds these terms and never calls a cosine of its own.
extern "C" int prcnn_kitti_pair_cos(int n_img, const long long *gt_off, const long long *dt_off, const long long *pair_off,
                                    const double *gt_alpha, const double *dt_alpha, double *out)
{
    PRCNN_REQUIRE(n_img >= 0 && (n_img == 0 || (gt_off && dt_off && pair_off)), "kitti_pair_cos: bad arguments");
    for (int m = 0; m < n_img; ++m) {
        const long long ng = gt_off[m + 1] - gt_off[m], nd = dt_off[m + 1] - dt_off[m];
        PRCNN_REQUIRE(ng >= 0 && nd >= 0 && pair_off[m + 1] - pair_off[m] == ng * nd, "kitti_pair_cos: offsets of image %d disagree", m);
        PRCNN_REQUIRE(ng * nd == 0 || (gt_alpha && dt_alpha && out), "kitti_pair_cos: null pointer");
        for (long long j = 0; j < nd; ++j)
            for (long long i = 0; i < ng; ++i)
                out[pair_off[m] + j * ng + i] = pair_cos_term(gt_alpha[gt_off[m] + i] - dt_alpha[dt_off[m] + j]);
    }
    return PRCNN_OK;
}
