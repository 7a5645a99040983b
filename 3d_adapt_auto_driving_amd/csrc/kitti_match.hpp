// kitti_match.hpp -- the greedy matching of one image of the KITTI AP evaluator (compute_statistics_jit,
// evaluate/eval2.py:170-289), written once for the host entries (kitti_stats.hip) and the device kernels (kitti_ap.hip).
//
// The scan is data dependent and sequential per image; what differs between its two users is where an image's columns live
// (the host entries' (n,5) / (n,6) f64 rows with i64 flags, the device path's split table with i8 flags) and where the two
// per-detection flags of the scan are kept.  Both are template parameters:
//   View  : ignored_gt(i), ignored_det(j) in {-1, 0, 1}; score(j); overlap(j, i); det_box(j), dc_box(i) -> const double[4]
//   Bits  : get(j) / set(j); the caller clears them (host: a vector of words; device: register words + a workspace)
//   on_tp : called with (gt index, detection index) for every true positive, in ground-truth order
// All arithmetic is f64 comparisons; nothing here rounds.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PRCNN_HD __host__ __device__ inline
#else
#define PRCNN_HD inline
#endif

namespace prcnn {

// image_box_overlap(boxes, query, criterion = 0) of one pair (eval2.py:102-128): intersection / area(box)
PRCNN_HD double overlap_over_box_area(const double *box, const double *q)
{
    const double iw = fmin(box[2], q[2]) - fmax(box[0], q[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = fmin(box[3], q[3]) - fmax(box[1], q[1]);
    if (!(ih > 0)) return 0.0;
    const double ua = (box[2] - box[0]) * (box[3] - box[1]);
    return iw * ih / ua;
}

struct MatchCounts {
    long long tp, fp, fn;
};

// `below` is read only with compute_fp (the caller has set bit j where score(j) < thresh); `assigned` must be clear.
template <class View, class Bits, class OnTp>
PRCNN_HD MatchCounts match_image(const View &v, int n_gt, int n_dt, int n_dc, int metric, double min_overlap, bool compute_fp,
                                 Bits &assigned, const Bits &below, OnTp &&on_tp)
{
    const double NO_DETECTION = -10000000.0;
    MatchCounts st = {0, 0, 0};
    for (int i = 0; i < n_gt; ++i) {
        const int ig = v.ignored_gt(i);
        if (ig == -1) continue;
        int det_idx = -1;
        double valid_detection = NO_DETECTION, max_overlap = 0.0;
        bool assigned_ignored_det = false;
        for (int j = 0; j < n_dt; ++j) {
            const int id = v.ignored_det(j);
            if (id == -1 || assigned.get(j) || (compute_fp && below.get(j))) continue;
            const double overlap = v.overlap(j, i);
            const double score = v.score(j);
            if (!compute_fp && overlap > min_overlap && score > valid_detection) {
                det_idx = j;
                valid_detection = score;
            } else if (compute_fp && overlap > min_overlap && (overlap > max_overlap || assigned_ignored_det) && id == 0) {
                max_overlap = overlap;
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = false;
            } else if (compute_fp && overlap > min_overlap && valid_detection == NO_DETECTION && id == 1) {
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = true;
            }
        }
        if (valid_detection == NO_DETECTION && ig == 0) {
            st.fn += 1;
        } else if (valid_detection != NO_DETECTION && (ig == 1 || v.ignored_det(det_idx) == 1)) {
            assigned.set(det_idx);
        } else if (valid_detection != NO_DETECTION) {
            st.tp += 1;
            on_tp(i, det_idx);
            assigned.set(det_idx);
        }
    }
    if (compute_fp) {
        for (int j = 0; j < n_dt; ++j) {
            const int id = v.ignored_det(j);
            if (!(assigned.get(j) || id == -1 || id == 1 || below.get(j))) st.fp += 1;
        }
        long long nstuff = 0;
        if (metric == 0) {
            for (int i = 0; i < n_dc; ++i)
                for (int j = 0; j < n_dt; ++j) {
                    const int id = v.ignored_det(j);
                    if (assigned.get(j) || id == -1 || id == 1 || below.get(j)) continue;
                    if (overlap_over_box_area(v.det_box(j), v.dc_box(i)) > min_overlap) {
                        assigned.set(j);
                        nstuff += 1;
                    }
                }
        }
        st.fp -= nstuff;
    }
    return st;
}

}  // namespace prcnn
