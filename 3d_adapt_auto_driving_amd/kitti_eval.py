"""Offline KITTI AP evaluator around the rotated-IoU HIP kernel (counterpart of evaluate/eval2.py:8-690,
evaluate/eval_old.py, evaluate/kitti_common.py:293-360 and the ``evaluate()`` driver evaluate/evaluate.py:84-296 with its output
transformations: grounding, re-scaling, size / front alignment against the best-overlapping ground truth, statistical mapping of
the ground truth, per-box overlap columns, and the command line).

Protocol of the reference fork (``metric="new"``): 41 recall sample points, 11-point mAP (every 4th), six DISTANCE
based "difficulties" instead of KITTI's easy/moderate/hard (eval2.py:48-52):

    level        0        1        2        3        4        5
    depth (m)  (0,30)   (0,70)   (0,70)   (0,30)  (30,50)  (50,70)
    occlusion   <=0      <=1      <=2      <=2      <=2      <=2
    truncation <=.15     <=.3     <=.5     <=.5     <=.5     <=.5

What is different in shape, not in result: the reference cuts the split into ~50 parts, computes a dense
rotated-IoU matrix per part on the GPU (cross-image pairs are discarded) and runs the greedy matching as
numba-jitted Python.  Here every image is one segment of a single block-diagonal launch
(``prcnn_rotate_iou_eval_segmented``), and the matching / PR accumulation are host functions of the same
library (csrc/kitti_stats.hip) fed with the whole split at once.

``metric="old"`` is evaluate/eval_old.py: KITTI's three difficulties with the image-height rule, the 40 / 25 / 25 px caps scaled by the
dataset's focal length (FOCAL); no distance band.

The transformations need, beyond host bookkeeping, one thing: every detection's best-overlapping ground-truth box of its image and
that BEV overlap, and the same for every ground-truth box.  ``best_match(device="cuda")`` gets both from one fused launch
(``prcnn_bev_best_match``, csrc/eval_match.hip) that never writes the pair matrix; ``device="cpu"`` is numpy's max / argmax over
``calculate_iou(..., 1)``.  align_size / align_front then run on the device too (``prcnn_eval_align``).

``stats_device="cuda"`` (off by default) moves the statistics themselves to the device: one table of the split's columns (SplitTable),
then flags, overlaps, both matching passes, thresholds and PR sums as kernels of csrc/kitti_ap.hip (DeviceStats) with one read at
the end.  The host path is its definition and its checker; both give the same bits.

Command line:  python -m 3d_adapt_auto_driving_amd.kitti_eval --result_path ... --dataset_path ... [--metric old] [--align_size] [--stats_device cuda] ...
"""
import ctypes
import io
import json
import os
import pathlib
import pickle
import re

import numpy as np

from . import _lib

CLASS_NAMES = ["car", "pedestrian", "cyclist"]
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting"}
DIST_BOUNDARY = np.array([[0, 0, 0, 0, 30, 50], [30, 70, 70, 30, 50, 70]], dtype=np.float64)
MAX_OCCLUSION = [0, 1, 2, 2, 2, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5, 0.5, 0.5, 0.5]
N_SAMPLE_PTS = 41
# metric="old" (eval_old.py:28-39): bbox-height caps of KITTI's easy / moderate / hard, scaled from KITTI's focal length to the dataset's
FOCAL = {"kitti": 707.05, "argo": 1870.57, "nusc": 1266.42, "lyft": 811.16, "waymo": 2069.82}
OLD_MAX_OCCLUSION = [0, 1, 2]
OLD_MAX_TRUNCATION = [0.15, 0.3, 0.5]
ALIGN_MIN_OVERLAP = 0.2          # evaluate.py:196,209: a detection is aligned when its best BEV overlap exceeds this


def min_height(dataset):
    return (np.array([40, 25, 25]) / FOCAL["kitti"] * FOCAL[dataset]).tolist()


def _difficulties(metric):
    if metric not in ("new", "old"):
        raise ValueError("metric %r is neither 'new' (distance) nor 'old' (bbox height)" % (metric,))
    return [0, 1, 2, 3, 4, 5] if metric == "new" else [0, 1, 2]


# ---------------------------------------------------------------------------------------------------
# label files (kitti_common.py:307-360)
# ---------------------------------------------------------------------------------------------------
def _anno_from_rows(rows):
    """rows: list of token lists (15 or 16 tokens).  dimensions are stored l, h, w (file order h, w, l)."""
    n = len(rows)
    anno = {
        "name": np.array([r[0] for r in rows]),
        "truncated": np.array([float(r[1]) for r in rows]),
        "occluded": np.array([int(r[2]) for r in rows]),
        "alpha": np.array([float(r[3]) for r in rows]),
        "bbox": np.array([[float(v) for v in r[4:8]] for r in rows], dtype=np.float64).reshape(-1, 4),
        "dimensions": np.array([[float(v) for v in r[8:11]] for r in rows], dtype=np.float64).reshape(-1, 3)[:, [2, 0, 1]],
        "location": np.array([[float(v) for v in r[11:14]] for r in rows], dtype=np.float64).reshape(-1, 3),
        "rotation_y": np.array([float(r[14]) for r in rows]).reshape(-1),
    }
    if n != 0 and len(rows[0]) == 16:
        anno["score"] = np.array([float(r[15]) for r in rows])
    else:
        anno["score"] = np.zeros([n])
    return anno


def get_label_anno(label_path):
    with open(label_path, "r") as f:
        rows = [line.strip().split(" ") for line in f.readlines()]
    return _anno_from_rows(rows)


def get_label_annos(label_folder, image_ids=None):
    folder = pathlib.Path(label_folder)
    if image_ids is None:
        pat = re.compile(r"^\d{6}.txt$")
        image_ids = sorted(int(p.stem) for p in folder.glob("*.txt") if pat.match(p.name))
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    return [get_label_anno(folder / ("%06d.txt" % i)) for i in image_ids]


def filter_annos_low_score(annos, thresh):
    out = []
    for a in annos:
        keep = [i for i, s in enumerate(a["score"]) if s >= thresh]
        out.append({k: v[keep] for k, v in a.items()})
    return out


def annos_from_lines(lines):
    """KITTI label lines (strings, as eval_rcnn.save_kitti_format writes them) -> annotation dict."""
    return _anno_from_rows([l.strip().split(" ") for l in lines if l.strip()])


# ---------------------------------------------------------------------------------------------------
# overlaps
# ---------------------------------------------------------------------------------------------------
def image_box_overlap(boxes, query_boxes, criterion=-1):
    """(N,4) x (K,4) [x1,y1,x2,y2] -> (N,K) in boxes.dtype (eval2.py:102-128): no +1 on the extents."""
    boxes = np.asarray(boxes)
    query_boxes = np.asarray(query_boxes)
    n, k = boxes.shape[0], query_boxes.shape[0]
    out = np.zeros((n, k), dtype=boxes.dtype)
    if n == 0 or k == 0:
        return out
    iw = np.minimum(boxes[:, None, 2], query_boxes[None, :, 2]) - np.maximum(boxes[:, None, 0], query_boxes[None, :, 0])
    ih = np.minimum(boxes[:, None, 3], query_boxes[None, :, 3]) - np.maximum(boxes[:, None, 1], query_boxes[None, :, 1])
    barea = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[:, None]
    qarea = ((query_boxes[:, 2] - query_boxes[:, 0]) * (query_boxes[:, 3] - query_boxes[:, 1]))[None, :]
    inter = iw * ih
    if criterion == -1:
        ua = barea + qarea - inter
    elif criterion == 0:
        ua = np.broadcast_to(barea, inter.shape)
    elif criterion == 1:
        ua = np.broadcast_to(qarea, inter.shape)
    else:
        ua = np.ones_like(inter)
    hit = (iw > 0) & (ih > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[hit] = (inter / ua)[hit]
    return out


def rotate_iou_segmented(boxes_list, query_list, criterion=-1, device_id=0):
    """Per-image rotated IoU in one launch.  boxes_list[i] (n_i,5), query_list[i] (k_i,5)
    [cx, cy, w, h, angle] -> list of (n_i,k_i) f32 arrays and the flat concatenation."""
    import torch
    nseg = len(boxes_list)
    n = np.array([len(b) for b in boxes_list], dtype=np.int64)
    k = np.array([len(q) for q in query_list], dtype=np.int64)
    box_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    q_off = np.concatenate([[0], np.cumsum(k)]).astype(np.int32)
    out_off = np.concatenate([[0], np.cumsum(n * k)]).astype(np.int64)
    total = int(out_off[-1])
    flat = np.zeros((total,), dtype=np.float32)
    if total > 0:
        dev = torch.device("cuda", device_id)
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1, 5) for x in xs], 0))
        b = torch.from_numpy(cat(boxes_list)).to(dev)
        q = torch.from_numpy(cat(query_list)).to(dev)
        oo, bo, qo = (torch.from_numpy(a).to(dev) for a in (out_off, box_off, q_off))
        out = torch.empty((total,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("prcnn_rotate_iou_eval_segmented", nseg, total, oo.data_ptr(), bo.data_ptr(), qo.data_ptr(),
                      b.data_ptr(), q.data_ptr(), out.data_ptr(), int(criterion), _lib.current_stream(out))
        flat = out.cpu().numpy()
    blocks = [flat[out_off[i]:out_off[i + 1]].reshape(int(n[i]), int(k[i])) for i in range(nseg)]
    return blocks, flat


def _bev_boxes(anno):
    return np.concatenate([anno["location"][:, [0, 2]], anno["dimensions"][:, [0, 2]], anno["rotation_y"][..., np.newaxis]], axis=1)


def _d3_boxes(anno):
    return np.concatenate([anno["location"], anno["dimensions"], anno["rotation_y"][..., np.newaxis]], axis=1)


def calculate_iou(dt_annos, gt_annos, metric, device_id=0):
    """Per-image overlap blocks (n_dt_i, n_gt_i) f64 for metric 0 image box / 1 BEV / 2 3D
    (eval2.py:352-427 called with (dt, gt) as at :492)."""
    assert len(gt_annos) == len(dt_annos)
    if metric == 0:
        return [image_box_overlap(d["bbox"], g["bbox"]) for d, g in zip(dt_annos, gt_annos)]
    if metric == 1:
        blocks, _ = rotate_iou_segmented([_bev_boxes(d) for d in dt_annos], [_bev_boxes(g) for g in gt_annos], -1, device_id)
        return [b.astype(np.float64) for b in blocks]
    if metric == 2:
        db, gb = [_d3_boxes(d) for d in dt_annos], [_d3_boxes(g) for g in gt_annos]
        blocks, _ = rotate_iou_segmented([b[:, [0, 2, 3, 5, 6]] for b in db], [b[:, [0, 2, 3, 5, 6]] for b in gb], 2, device_id)
        out = []
        for rinc, boxes, qboxes in zip(blocks, db, gb):
            # height overlap x BEV intersection / union volume, in f64 (d3_box_overlap_kernel, eval2.py:136-161);
            # y is the box bottom in the camera frame, the box extends to y - h
            rinc = rinc.astype(np.float64)
            iw = (np.minimum(boxes[:, None, 1], qboxes[None, :, 1]) -
                  np.maximum(boxes[:, None, 1] - boxes[:, None, 4], qboxes[None, :, 1] - qboxes[None, :, 4]))
            area1 = (boxes[:, 3] * boxes[:, 4] * boxes[:, 5])[:, None]
            area2 = (qboxes[:, 3] * qboxes[:, 4] * qboxes[:, 5])[None, :]
            inc = iw * rinc
            with np.errstate(divide="ignore", invalid="ignore"):
                val = inc / (area1 + area2 - inc)
            out.append(np.where(rinc > 0, np.where(iw > 0, val, 0.0), rinc))
        return out
    raise ValueError("unknown metric")


# ---------------------------------------------------------------------------------------------------
# per-image bookkeeping
# ---------------------------------------------------------------------------------------------------
def clean_data(gt_anno, dt_anno, current_class, dataset, difficulty, metric="new"):
    """-> num_valid_gt, ignored_gt (n_gt) i64: 0 care / 1 ignore / -1 other class, ignored_dt (n_dt) i64, dc_bboxes (k, 4)
    (the per-image bookkeeping of evaluate/eval2.py:28-98, whole-array): a ground-truth box is CARED FOR when it carries the evaluated
    class name and passes the difficulty level's caps -- occlusion, truncation, and the distance band the reference uses instead of
    the official image-height rule; it is IGNORED (matches cost nothing) when it fails a cap or carries the neighbouring class
    (Van for Car, Person_sitting for Pedestrian); everything else is another class.  A detection outside the distance band is
    ignored, one of another class does not take part.  DontCare boxes are handed back for the false-positive exemption.
    metric="old" (eval_old.py:28-91): three levels; instead of the distance band a ground-truth box is ignored when its bbox height
    is <= min_height(dataset)[difficulty] and a detection when |height| is below it -- the only place ``dataset`` matters."""
    cls = CLASS_NAMES[current_class]
    _difficulties(metric)
    raw = np.asarray(gt_anno["name"], dtype=str).reshape(-1)
    names = np.char.lower(raw) if raw.size else raw
    gt_bbox = np.asarray(gt_anno["bbox"], dtype=np.float64).reshape(-1, 4)
    det = np.asarray(dt_anno["name"], dtype=str).reshape(-1)
    if metric == "old":
        cap = min_height(dataset)[difficulty]
        capped = ((np.asarray(gt_anno["occluded"]).reshape(-1) > OLD_MAX_OCCLUSION[difficulty]) |
                  (np.asarray(gt_anno["truncated"]).reshape(-1) > OLD_MAX_TRUNCATION[difficulty]) |
                  (gt_bbox[:, 3] - gt_bbox[:, 1] <= cap))
        dt_bbox = np.asarray(dt_anno["bbox"], dtype=np.float64).reshape(-1, 4)
        in_band = ~(np.abs(dt_bbox[:, 3] - dt_bbox[:, 1]) < cap)
    else:
        near, far = DIST_BOUNDARY[0, difficulty], DIST_BOUNDARY[1, difficulty]
        depth = np.asarray(gt_anno["location"], dtype=np.float64).reshape(-1, 3)[:, 2]
        capped = ((np.asarray(gt_anno["occluded"]).reshape(-1) > MAX_OCCLUSION[difficulty]) |
                  (np.asarray(gt_anno["truncated"]).reshape(-1) > MAX_TRUNCATION[difficulty]) | ~((near < depth) & (depth < far)))
        det_depth = np.asarray(dt_anno["location"], dtype=np.float64).reshape(-1, 3)[:, 2]
        in_band = (near < det_depth) & (det_depth < far)
    own = names == cls
    sibling = names == {"pedestrian": "person_sitting", "car": "van"}.get(cls, "\0")
    ignored_gt = np.full(names.shape, -1, dtype=np.int64)
    ignored_gt[sibling | (own & capped)] = 1
    ignored_gt[own & ~capped] = 0
    dc_bboxes = gt_bbox[raw == "DontCare"]
    det_own = (np.char.lower(det) if det.size else det) == cls
    ignored_dt = np.where(in_band, np.where(det_own, 0, -1), 1).astype(np.int64)
    return int(np.count_nonzero(ignored_gt == 0)), ignored_gt, ignored_dt, dc_bboxes


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """Score thresholds at (about) equally spaced recall positions -- the selection rule of evaluate/eval2.py:8-25 in closed form.
    With the true-positive scores in descending order, score i spans the recall interval [(i + 1) / num_gt, (i + 2) / num_gt] and
    the targets are c_t = t / (num_sample_pts - 1), accumulated by repeated addition as the reference does.  Target t may take score
    i unless the interval's far end is closer to the target than its near end (then a later score serves it better); the last score
    serves any target.  So a_t = the first score target t may take, and since every score is offered to one target only, the score
    taken for target t is i_t = max(a_t, i_(t-1) + 1), i.e. t + running max of (a_s - s): one comparison matrix, no loop."""
    s = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    n = len(s)
    if n == 0:
        return []
    step = 1 / (num_sample_pts - 1.0)
    n_targets = min(n, int(np.ceil((n + 2) / (num_gt * step))) + 2)                 # targets beyond recall n / num_gt all take the last score
    targets = np.concatenate([[0.0], np.cumsum(np.full(max(n_targets - 1, 0), step))])     # 0, step, step + step, ...: the reference's sums
    pos = np.arange(n)
    near_end, far_end = (pos + 1) / num_gt, np.where(pos < n - 1, (pos + 2) / num_gt, (pos + 1) / num_gt)
    later_is_better = (far_end[None, :] - targets[:, None]) < (targets[:, None] - near_end[None, :])
    later_is_better[:, n - 1] = False
    first_ok = np.argmin(later_is_better, axis=1)                                   # a_t (the last column is always admissible)
    t = np.arange(len(targets))
    taken = t + np.maximum.accumulate(first_ok - t)
    return list(s[taken[taken < n]])


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class _Split:
    """Concatenated per-image arrays of one (class, difficulty) in the layout csrc/kitti_stats.hip reads."""

    def __init__(self, gt_annos, dt_annos, current_class, dataset, difficulty, metric="new"):
        ig, idt, dcs, gts, dts = [], [], [], [], []
        self.num_valid_gt = 0
        for g, d in zip(gt_annos, dt_annos):
            nv, ignored_gt, ignored_dt, dc = clean_data(g, d, current_class, dataset, difficulty, metric)
            self.num_valid_gt += nv
            ig.append(ignored_gt)
            idt.append(ignored_dt)
            dcs.append(dc)
            gts.append(np.concatenate([g["bbox"], g["alpha"][..., np.newaxis]], 1).astype(np.float64).reshape(-1, 5))
            dts.append(np.concatenate([d["bbox"], d["alpha"][..., np.newaxis], d["score"][..., np.newaxis]], 1)
                       .astype(np.float64).reshape(-1, 6))
        cat = lambda xs, w, t: np.ascontiguousarray(np.concatenate(xs, 0) if xs else np.zeros((0, w) if w else (0,), t))
        self.gt_nums = np.array([len(x) for x in ig], dtype=np.int64)
        self.dt_nums = np.array([len(x) for x in idt], dtype=np.int64)
        self.dc_nums = np.array([len(x) for x in dcs], dtype=np.int64)
        self.ignored_gts, self.ignored_dets = cat(ig, 0, np.int64), cat(idt, 0, np.int64)
        self.dontcares, self.gt_datas, self.dt_datas = cat(dcs, 4, np.float64), cat(gts, 5, np.float64), cat(dts, 6, np.float64)


# ---------------------------------------------------------------------------------------------------
# the split as one table, and the statistics on the device (csrc/kitti_ap.hip)
# ---------------------------------------------------------------------------------------------------
class StatsDeviceError(RuntimeError):
    """stats_device="cuda" was asked for and no GPU is usable.  There is no fallback to the host path."""


def _check_stats_device(stats_device):
    if stats_device not in ("cpu", "cuda"):
        raise ValueError("stats_device %r is neither 'cpu' nor 'cuda'" % (stats_device,))


CLASS_CODE = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4}      # include/prcnn_hip.h: the split table
SIBLING_CODE = {0: 3, 1: 4}                                                                # Van for Car, Person_sitting for Pedestrian
REG_DETS = _lib.PRCNN_AP_REG_DETS                    # detections per image whose scan flags the kernels keep in registers


class SplitSide:
    """One side (labels or detections) of a split as concatenated columns: ``off`` (n_img + 1) i64, ``code`` i8 class codes of the
    lower-cased names (lower-casing runs over the UNIQUE names), ``is_dc`` (the name is exactly "DontCare"), and the numeric columns
    occluded, truncated, bbox, alpha, location, dimensions (l, h, w), rotation_y, score as f64."""

    def __init__(self, annos):
        self.n_img = len(annos)
        nums = np.array([len(a["name"]) for a in annos], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(nums)]).astype(np.int64)
        names = np.concatenate([np.asarray(a["name"], dtype=str).reshape(-1) for a in annos]) if self.n_img else np.zeros((0,), dtype=str)
        uniq, inv = np.unique(names, return_inverse=True) if names.size else (np.zeros((0,), dtype=str), np.zeros((0,), dtype=np.int64))
        self.code = np.array([CLASS_CODE.get(u.lower(), -1) for u in uniq], dtype=np.int8)[inv].reshape(-1)
        self.is_dc = np.array([u == "DontCare" for u in uniq], dtype=bool)[inv].reshape(-1)
        col = lambda key, w: _cat([a[key] for a in annos], w)
        self.occluded, self.truncated, self.alpha = col("occluded", 0), col("truncated", 0), col("alpha", 0)
        self.bbox, self.location, self.dimensions = col("bbox", 4), col("location", 3), col("dimensions", 3)
        self.rotation_y, self.score = col("rotation_y", 0), col("score", 0)

    def __len__(self):
        return int(self.off[-1])

    @property
    def box3d(self):                                 # _d3_boxes: x y z l h w ry
        return np.ascontiguousarray(np.concatenate([self.location, self.dimensions, self.rotation_y[:, None]], axis=1))

    @property
    def bev(self):                                   # _bev_boxes == _d3_boxes[:, [0, 2, 3, 5, 6]], narrowed as rotate_iou_segmented does
        return np.ascontiguousarray(self.box3d[:, [0, 2, 3, 5, 6]].astype(np.float32))


class PreparedGT:
    """The ground-truth half of a split, parsed and tabulated once: pass it wherever ``gt_annos`` goes (the device path takes its
    columns, the host path its annotation list) -- a sweep evaluates every checkpoint against the same one."""

    def __init__(self, gt_annos, ids=None):
        self.annos = list(gt_annos)
        self.ids = None if ids is None else list(ids)
        self.side = SplitSide(self.annos)

    def __len__(self):
        return len(self.annos)


def _plain_gt(gt_annos):
    return gt_annos.annos if isinstance(gt_annos, PreparedGT) else gt_annos


class SplitTable:
    """Both sides of a split and what pairs them: per-image offsets of ground truth, detections, DontCare rows and (n_dt x n_gt)
    pair blocks; ``dc_rows``: the ground-truth rows named DontCare, in order.  Built in whole-array numpy, once per evaluation;
    ``gt_annos`` may be a PreparedGT."""

    def __init__(self, gt_annos, dt_annos):
        self.gt = gt_annos.side if isinstance(gt_annos, PreparedGT) else SplitSide(gt_annos)
        self.dt = SplitSide(dt_annos)
        if self.gt.n_img != self.dt.n_img:
            raise ValueError("SplitTable: %d label images but %d detection images" % (self.gt.n_img, self.dt.n_img))
        self.n_img = self.gt.n_img
        self.gt_off, self.dt_off = self.gt.off, self.dt.off
        self.gt_nums, self.dt_nums = np.diff(self.gt_off), np.diff(self.dt_off)
        self.pair_off = np.concatenate([[0], np.cumsum(self.gt_nums * self.dt_nums)]).astype(np.int64)
        self.dc_rows = np.flatnonzero(self.gt.is_dc)
        self.dc_off = np.searchsorted(self.dc_rows, self.gt_off).astype(np.int64)
        self.dc_bbox = np.ascontiguousarray(self.gt.bbox[self.dc_rows])
        self.max_dt = int(self.dt_nums.max()) if self.n_img else 0
        big = self.dt_nums > REG_DETS
        self.ws_slot = np.where(big, np.cumsum(big) - 1, -1).astype(np.int32)
        self.n_big = int(big.sum())


def difficulty_caps(dataset, difficultys, metric):
    """(n_diff, 5) f64 rows [max occlusion, max truncation, band near, band far, min bbox height] of clean_data's comparisons"""
    _difficulties(metric)
    rows = []
    for d in difficultys:
        if metric == "old":
            rows.append([OLD_MAX_OCCLUSION[d], OLD_MAX_TRUNCATION[d], 0.0, 0.0, min_height(dataset)[d]])
        else:
            rows.append([MAX_OCCLUSION[d], MAX_TRUNCATION[d], DIST_BOUNDARY[0, d], DIST_BOUNDARY[1, d], 0.0])
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 5))


def split_flags(table, current_class, dataset, difficulty, metric="new"):
    """clean_data for every image of the split at once -> ignored_gt (n_gt) i64, ignored_dt (n_dt) i64, num_valid_gt, dc_bboxes
    (n_dc, 4): the concatenation of what clean_data gives image by image, and the definition of prcnn_ap_flags."""
    CLASS_NAMES[current_class]
    max_occ, max_trunc, near, far, cap = difficulty_caps(dataset, [difficulty], metric)[0]
    gt, dt = table.gt, table.dt
    if metric == "old":
        capped = (gt.occluded > max_occ) | (gt.truncated > max_trunc) | (gt.bbox[:, 3] - gt.bbox[:, 1] <= cap)
        in_band = ~(np.abs(dt.bbox[:, 3] - dt.bbox[:, 1]) < cap)
    else:
        capped = (gt.occluded > max_occ) | (gt.truncated > max_trunc) | ~((near < gt.location[:, 2]) & (gt.location[:, 2] < far))
        in_band = (near < dt.location[:, 2]) & (dt.location[:, 2] < far)
    own, sibling = gt.code == current_class, gt.code == SIBLING_CODE.get(current_class, -2)
    ignored_gt = np.full(len(gt), -1, dtype=np.int64)
    ignored_gt[sibling | (own & capped)] = 1
    ignored_gt[own & ~capped] = 0
    ignored_dt = np.where(in_band, np.where(dt.code == current_class, 0, -1), 1).astype(np.int64)
    return ignored_gt, ignored_dt, int(np.count_nonzero(ignored_gt == 0)), table.dc_bbox


def thresholds_loop(sorted_scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """The reference's loop as written (evaluate/eval2.py:8-25) over scores already in descending order: the definition of
    prcnn_ap_thresholds (get_thresholds is its closed form)."""
    current_recall = 0
    thresholds = []
    n = len(sorted_scores)
    for i, score in enumerate(sorted_scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def pair_cos(table):
    """(n_pair) f64: (1 + cos(gt alpha - dt alpha)) / 2 per pair in the overlap blocks' layout, by the library's host entry"""
    out = np.zeros((int(table.pair_off[-1]),), dtype=np.float64)
    _lib.call("prcnn_kitti_pair_cos", table.n_img, _ptr(table.gt_off), _ptr(table.dt_off), _ptr(table.pair_off),
              _ptr(table.gt.alpha), _ptr(table.dt.alpha), _ptr(out))
    return out


class DeviceStats:
    """A SplitTable on the device and the stages of csrc/kitti_ap.hip over it.  Every stage returns DEVICE tensors and reads nothing
    back; eval_class chains them and reads once.  All launches go to torch's current stream of the device."""
    CHUNK_BYTES = 256 << 20                          # bound on the per-image similarity buffer and the score rows of one chunk of levels

    def __init__(self, table, device_id=0):
        import torch
        if not torch.cuda.is_available():
            raise StatsDeviceError("stats_device='cuda': torch sees no usable GPU (torch.cuda.is_available() is False); "
                                   "there is no fallback -- pass stats_device='cpu' for the host path")
        self.torch, self.table = torch, table
        self.dev = torch.device("cuda", device_id)
        up = self._up
        gt, dt = table.gt, table.dt
        self.t = {"gt_off": up(table.gt_off), "dt_off": up(table.dt_off), "dc_off": up(table.dc_off), "pair_off": up(table.pair_off),
                  "ws_slot": up(table.ws_slot), "gt_code": up(gt.code), "dt_code": up(dt.code), "gt_occluded": up(gt.occluded),
                  "gt_truncated": up(gt.truncated), "gt_bbox": up(gt.bbox), "gt_depth": up(gt.location[:, 2]), "gt_box3d": up(gt.box3d),
                  "dt_bbox": up(dt.bbox), "dt_depth": up(dt.location[:, 2]), "dt_score": up(dt.score), "dt_box3d": up(dt.box3d),
                  "dc_bbox": up(table.dc_bbox), "gt_bev": up(gt.bev), "dt_bev": up(dt.bev)}
        self.n_gt, self.n_dt, self.n_pair = len(gt), len(dt), int(table.pair_off[-1])
        # the table as the entries take it: a host array of i64 words, counts then device pointers (include/prcnn_hip.h PRCNN_AP_*)
        self.words = np.zeros((_lib.PRCNN_AP_SPLIT_WORDS,), dtype=np.int64)
        for key, value in (("n_img", table.n_img), ("max_dt", table.max_dt), ("n_gt", self.n_gt), ("n_dt", self.n_dt),
                           ("n_dc", len(table.dc_rows)), ("n_pair", self.n_pair)) + tuple((k, v.data_ptr()) for k, v in self.t.items()):
            self.words[getattr(_lib, "PRCNN_AP_" + key.upper())] = value
        self._flags, self._overlaps, self._cos = {}, {}, None

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.dev)

    def _call(self, name, *args):
        with self.torch.cuda.device(self.dev):
            _lib.call(name, *args, _lib.current_stream(self.t["gt_off"]))

    def flags(self, current_class, dataset, difficultys, metric="new"):
        """-> ignored_gt (n_diff, n_gt) i8, ignored_dt (n_diff, n_dt) i8, num_valid_gt (n_diff) i32; one launch, kept per key"""
        key = (current_class, dataset if metric == "old" else None, tuple(difficultys), metric)
        if key not in self._flags:
            CLASS_NAMES[current_class]
            T, n_diff = self.torch, len(difficultys)
            caps = difficulty_caps(dataset, difficultys, metric)
            ig, idt, nv = self._empty((n_diff, self.n_gt), T.int8), self._empty((n_diff, self.n_dt), T.int8), self._empty((n_diff,), T.int32)
            self._call("prcnn_ap_flags", _ptr(self.words), int(current_class), SIBLING_CODE.get(current_class, -2),
                       int(metric == "old"), n_diff, _ptr(caps), _lib.ptr(ig), _lib.ptr(idt), _lib.ptr(nv))
            self._flags[key] = (ig, idt, nv)
        return self._flags[key]

    def overlaps(self, kind):
        """-> (n_pair) f64, the flat concatenation of calculate_iou(dt, gt, kind)'s blocks; kept per kind"""
        if kind not in self._overlaps:
            T = self.torch
            if kind == 0:
                out = self._empty((self.n_pair,), T.float64)
                self._call("prcnn_ap_overlaps", _ptr(self.words), 0, None, _lib.ptr(out))
            elif kind in (1, 2):
                raw = self._empty((self.n_pair,), T.float32)
                off32 = lambda a: self._up(a.astype(np.int32))
                if not hasattr(self, "_off32"):
                    self._off32 = (off32(self.table.dt_off), off32(self.table.gt_off))
                self._call("prcnn_rotate_iou_eval_segmented", self.table.n_img, self.n_pair, _lib.ptr(self.t["pair_off"]),
                           _lib.ptr(self._off32[0]), _lib.ptr(self._off32[1]), _lib.ptr(self.t["dt_bev"]), _lib.ptr(self.t["gt_bev"]),
                           _lib.ptr(raw), -1 if kind == 1 else 2)
                if kind == 1:
                    out = raw.double()
                else:
                    out = self._empty((self.n_pair,), T.float64)
                    self._call("prcnn_ap_overlaps", _ptr(self.words), 2, _lib.ptr(raw), _lib.ptr(out))
            else:
                raise ValueError("unknown metric")
            self._overlaps[kind] = out
        return self._overlaps[kind]

    def upload_overlaps(self, blocks):
        """A caller's per-image (n_dt, n_gt) blocks, as they are"""
        flat = np.concatenate([np.asarray(o, dtype=np.float64).reshape(-1) for o in blocks]) if len(blocks) else np.zeros((0,))
        if flat.shape[0] != self.n_pair:
            raise ValueError("overlaps hold %d pairs, the split has %d" % (flat.shape[0], self.n_pair))
        return self._up(flat.astype(np.float64))

    def pair_cos(self):
        if self._cos is None:
            self._cos = self._up(pair_cos(self.table))
        return self._cos

    def _workspace(self, n_groups, lanes):
        words = (self.table.max_dt + 63) // 64 if self.table.n_big else 0
        ws = self._empty((max(1, self.table.n_big * n_groups * lanes * words),), self.torch.int64)
        return ws, words

    def scores(self, flags, overlaps, kind, min_overlaps):
        """Pass 1.  min_overlaps (n_lev) f64 device -> scores (n_groups, n_gt) f64 (-inf where unmatched), valid (n_groups, n_gt) i8"""
        T, (ig, idt, nv) = self.torch, flags
        n_diff, n_lev = ig.shape[0], min_overlaps.shape[0]
        scores, valid = self._empty((n_diff * n_lev, self.n_gt), T.float64), self._empty((n_diff * n_lev, self.n_gt), T.int8)
        ws, words = self._workspace(n_diff * n_lev, 1)
        self._call("prcnn_ap_scores", _ptr(self.words), _lib.ptr(ig), _lib.ptr(idt), n_diff, n_lev, _lib.ptr(min_overlaps),
                   _lib.ptr(overlaps), int(kind), _lib.ptr(scores), _lib.ptr(valid), _lib.ptr(ws), words)
        return scores, valid

    def thresholds(self, scores, valid, num_valid_gt):
        """One batched descending sort, the per-group count, then the reference's loop per group
        -> sorted (n_groups, n_gt), count (n_groups) i32, thresholds (n_groups, 41) f64, n_thr (n_groups) i32"""
        T, n_groups = self.torch, scores.shape[0]
        ordered = T.sort(scores, dim=1, descending=True).values.contiguous()
        count = valid.sum(dim=1, dtype=T.int32)
        thr, n_thr = self._empty((n_groups, N_SAMPLE_PTS), T.float64), self._empty((n_groups,), T.int32)
        self._call("prcnn_ap_thresholds", n_groups, n_groups // num_valid_gt.shape[0], self.n_gt, _lib.ptr(ordered), _lib.ptr(count),
                   _lib.ptr(num_valid_gt), _lib.ptr(thr), _lib.ptr(n_thr))
        return ordered, count, thr, n_thr

    def pr(self, flags, overlaps, kind, min_overlaps, thr, n_thr, compute_aos):
        """Pass 2 and the sums -> pr (n_groups, 41, 4) f64 = [tp, fp, fn, similarity]"""
        T, (ig, idt, nv) = self.torch, flags
        n_diff, n_lev = ig.shape[0], min_overlaps.shape[0]
        n_groups = n_diff * n_lev
        counts, pr = self._empty((n_groups, N_SAMPLE_PTS, 3), T.int64), self._empty((n_groups, N_SAMPLE_PTS, 4), T.float64)
        sim = self._empty((self.table.n_img, n_groups, N_SAMPLE_PTS), T.float64) if compute_aos else None
        cos = self.pair_cos() if compute_aos else None
        ws, words = self._workspace(n_groups, 2 * 64)
        self._call("prcnn_ap_pr", _ptr(self.words), _lib.ptr(ig), _lib.ptr(idt), n_diff, n_lev, _lib.ptr(min_overlaps),
                   _lib.ptr(overlaps), int(kind), _lib.ptr(thr), _lib.ptr(n_thr), _lib.ptr(cos), _lib.ptr(counts), _lib.ptr(sim),
                   _lib.ptr(pr), _lib.ptr(ws), words)
        return pr

    def level_chunk(self, n_diff, n_lev):
        per_level = 8 * n_diff * max(self.table.n_img * N_SAMPLE_PTS, 3 * self.n_gt, 1)
        return max(1, min(n_lev, self.CHUNK_BYTES // per_level))

    def eval_class(self, current_classes, dataset, difficultys, kind, min_overlaps, compute_aos=False, overlaps=None,
                   difficulty_metric="new"):
        """-> pr (n_class, n_diff, n_lev, 41, 4) f64 and n_thr (n_class, n_diff, n_lev) int, numpy, from ONE device-to-host read"""
        T = self.torch
        with T.cuda.device(self.dev):
            ov = self.overlaps(kind) if overlaps is None else self.upload_overlaps(overlaps)
            n_cls, n_diff, n_lev, width = len(current_classes), len(difficultys), len(min_overlaps), 4 * N_SAMPLE_PTS
            out = T.zeros((n_cls, n_diff, n_lev, width + 1), dtype=T.float64, device=self.dev)
            step = self.level_chunk(n_diff, n_lev)
            for m, current_class in enumerate(current_classes):
                flags = self.flags(current_class, dataset, difficultys, difficulty_metric)
                levels = self._up(np.asarray(min_overlaps[:, kind, m], dtype=np.float64))
                for k0 in range(0, n_lev, step):
                    lev = levels[k0:k0 + step]
                    scores, valid = self.scores(flags, ov, kind, lev)
                    _, _, thr, n_thr = self.thresholds(scores, valid, flags[2])
                    pr = self.pr(flags, ov, kind, lev, thr, n_thr, compute_aos)
                    out[m, :, k0:k0 + step, :width] = pr.view(n_diff, lev.shape[0], width)
                    out[m, :, k0:k0 + step, width] = n_thr.view(n_diff, lev.shape[0]).double()
            host = out.cpu().numpy()                                                     # the read
        n_thr = host[..., width].astype(np.int64)
        if n_thr.size and n_thr.max() > N_SAMPLE_PTS:
            raise _lib.PrcnnError("a group took %d recall thresholds (> %d)" % (n_thr.max(), N_SAMPLE_PTS))
        return host[..., :width].reshape(n_cls, n_diff, n_lev, N_SAMPLE_PTS, 4), n_thr


def _fill_curves(precision, recall, aos, pr, compute_aos):
    """pr (n_thresholds, 4) = [tp, fp, fn, similarity] -> one group's 41-sample rows, in place (eval2.py:545-560)."""
    n = len(pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            recall[i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
            precision[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                aos[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
    for i in range(n):      # monotone envelope, right to left
        precision[i] = np.max(precision[i:], axis=-1)
        recall[i] = np.max(recall[i:], axis=-1)
        if compute_aos:
            aos[i] = np.max(aos[i:], axis=-1)


def eval_class(gt_annos, dt_annos, current_classes, dataset, difficultys, metric, min_overlaps, compute_aos=False,
               device_id=0, overlaps=None, difficulty_metric="new", stats_device="cpu", split=None):
    """-> dict(recall, precision, orientation), each [num_class, num_difficulty, num_minoverlap, 41]
    (eval2.py:460-569).  min_overlaps: [num_minoverlap, metric, num_class].  ``metric`` is the overlap kind (0 image box / 1 BEV /
    2 3D) as in the reference; the difficulty rule ("new" | "old", the ``metric`` keyword everywhere else) is ``difficulty_metric``.
    stats_device "cpu": the host entries of csrc/kitti_stats.hip; "cuda": flags, overlaps, both passes, thresholds and sums on the
    device (csrc/kitti_ap.hip) with one read at the end -- the same bits.  ``split``: a DeviceStats of these annotations to reuse."""
    _check_stats_device(stats_device)
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    precision, recall, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    if stats_device == "cuda":
        if split is None:
            split = DeviceStats(SplitTable(gt_annos, dt_annos), device_id)
        pr, n_thr = split.eval_class(current_classes, dataset, difficultys, metric, min_overlaps, compute_aos, overlaps, difficulty_metric)
        for m in range(shape[0]):
            for l in range(shape[1]):
                for k in range(shape[2]):
                    _fill_curves(precision[m, l, k], recall[m, l, k], aos[m, l, k], pr[m, l, k, :n_thr[m, l, k]], compute_aos)
        return {"recall": recall, "precision": precision, "orientation": aos}
    gt_annos = _plain_gt(gt_annos)
    assert len(gt_annos) == len(dt_annos)
    n_img = len(gt_annos)
    if overlaps is None:
        overlaps = calculate_iou(dt_annos, gt_annos, metric, device_id)
    flat = np.ascontiguousarray(np.concatenate([o.reshape(-1) for o in overlaps]) if n_img else np.zeros((0,)), dtype=np.float64)
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            sp = _Split(gt_annos, dt_annos, current_class, dataset, difficulty, difficulty_metric)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                scores = np.zeros((max(1, int(sp.gt_nums.sum())),), dtype=np.float64)
                n_scores = ctypes.c_longlong(0)
                _lib.call("prcnn_kitti_collect_scores", n_img, _ptr(sp.gt_nums), _ptr(sp.dt_nums), _ptr(flat),
                          _ptr(sp.gt_datas), _ptr(sp.dt_datas), _ptr(sp.ignored_gts), _ptr(sp.ignored_dets), int(metric),
                          float(min_overlap), _ptr(scores), ctypes.cast(ctypes.pointer(n_scores), ctypes.c_void_p))
                thresholds = np.array(get_thresholds(scores[:n_scores.value], sp.num_valid_gt), dtype=np.float64)
                pr = np.zeros([len(thresholds), 4])
                if len(thresholds):
                    _lib.call("prcnn_kitti_accumulate_pr", n_img, _ptr(sp.gt_nums), _ptr(sp.dt_nums), _ptr(sp.dc_nums),
                              _ptr(flat), _ptr(sp.gt_datas), _ptr(sp.dt_datas), _ptr(sp.dontcares), _ptr(sp.ignored_gts),
                              _ptr(sp.ignored_dets), int(metric), float(min_overlap), _ptr(thresholds), len(thresholds),
                              int(bool(compute_aos)), _ptr(pr))
                _fill_curves(precision[m, l, k], recall[m, l, k], aos[m, l, k], pr, compute_aos)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    """11-point interpolated AP in percent from the 41-sample precision curve: the samples at recall 0, 0.1, ..., 1 (every 4th one),
    added left to right (a cumulative sum: the reference's order of additions, evaluate/eval2.py:572-576), over 11."""
    return np.cumsum(prec[..., ::4], axis=-1)[..., -1] / 11 * 100


def do_eval(gt_annos, dt_annos, current_classes, dataset, min_overlaps, compute_aos=False, device_id=0, metric="new", stats_device="cpu"):
    difficultys = _difficulties(metric)
    _check_stats_device(stats_device)
    # the device path builds the split table and its uploads once; the three overlap kinds share them and the flags
    split = DeviceStats(SplitTable(gt_annos, dt_annos), device_id) if stats_device == "cuda" else None
    more = {"device_id": device_id, "difficulty_metric": metric, "stats_device": stats_device, "split": split}
    ret = eval_class(gt_annos, dt_annos, current_classes, dataset, difficultys, 0, min_overlaps, compute_aos, **more)
    mAP_bbox = get_mAP(ret["precision"])
    mAP_aos = get_mAP(ret["orientation"]) if compute_aos else None
    mAP_bev = get_mAP(eval_class(gt_annos, dt_annos, current_classes, dataset, difficultys, 1, min_overlaps, **more)["precision"])
    mAP_3d = get_mAP(eval_class(gt_annos, dt_annos, current_classes, dataset, difficultys, 2, min_overlaps, **more)["precision"])
    return mAP_bbox, mAP_bev, mAP_3d, mAP_aos


def _line(value):
    s = io.StringIO()
    print(value, file=s)
    return s.getvalue()


def _class_ids(current_classes):
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [name_to_class[c] if isinstance(c, str) else c for c in current_classes]


def _alpha_is_valid(dt_annos):
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(anno["alpha"][0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, dataset="kitti", dense_sample=False, device_id=0, metric="new",
                             stats_device="cpu"):
    """-> (result text, dict) in the reference's format (eval2.py:629-722; metric="old": eval_old.py:619-695, three numbers per
    line and no dense sampling)."""
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5], [0.7, 0.5, 0.5, 0.7, 0.5]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    extra = []
    if dense_sample and metric == "new":
        for i in range(101):
            tmp = np.zeros((3, 5))
            tmp[:, 0] = i / 100.0
            extra.append(tmp)
    min_overlaps = np.stack([overlap_0_7, overlap_0_5] + extra, axis=0)
    current_classes = _class_ids(current_classes)
    min_overlaps = min_overlaps[:, :, current_classes]
    compute_aos = _alpha_is_valid(dt_annos)
    mAPbbox, mAPbev, mAP3d, mAPaos = do_eval(gt_annos, dt_annos, current_classes, dataset, min_overlaps, compute_aos, device_id,
                                             metric, stats_device)
    levels = range(len(_difficulties(metric)))
    result = ""
    res = {}
    for j, curcls in enumerate(current_classes):
        res[curcls] = {}
        for i in range(min_overlaps.shape[0]):
            head = "%s AP@%.2f, %.2f, %.2f" % ((CLASS_TO_NAME[curcls],) + tuple(min_overlaps[i, :, j]))
            res[curcls][head] = {"mAPbbox": mAPbbox[j, :, i], "mAPbev": mAPbev[j, :, i], "mAP3d": mAP3d[j, :, i]}
            result += _line(head + ":")
            for tag, arr in (("bbox AP:", mAPbbox), ("bev  AP:", mAPbev), ("3d   AP:", mAP3d)):
                result += _line(tag + "".join("%.4f, " % arr[j, d, i] for d in levels))
            if compute_aos:                           # the old metric's line keeps its trailing separator (eval_old.py:681-683)
                result += _line("aos  AP:" + ", ".join("%.2f" % mAPaos[j, d, i] for d in levels) + (", " if metric == "old" else ""))
    ret = {"result": res}
    for tag, arr in (("3d", mAP3d), ("bev", mAPbev), ("image", mAPbbox)):
        for d, name in enumerate(("easy", "moderate", "hard")):
            ret["Car_%s_%s" % (tag, name)] = arr[0, d, 0]
    return result, ret


COCO_RANGE = {0: [0.5, 0.95, 10], 1: [0.25, 0.7, 10], 2: [0.25, 0.7, 10], 3: [0.5, 0.95, 10], 4: [0.25, 0.7, 10]}


def do_coco_style_eval(gt_annos, dt_annos, current_classes, overlap_ranges, compute_aos, dataset="kitti", device_id=0, metric="new",
                       stats_device="cpu"):
    """mAP averaged over ten overlap thresholds (eval2.py:611-626).  overlap_ranges: [lo / hi / count, overlap kind, num_class].
    The reference's call of do_eval is one argument short since ``dataset`` joined its signature; this passes it."""
    min_overlaps = np.zeros([10, *overlap_ranges.shape[1:]])
    for i in range(overlap_ranges.shape[1]):
        for j in range(overlap_ranges.shape[2]):
            lo, hi, num = overlap_ranges[:, i, j]
            min_overlaps[:, i, j] = np.linspace(lo, hi, int(num))
    mAP_bbox, mAP_bev, mAP_3d, mAP_aos = do_eval(gt_annos, dt_annos, current_classes, dataset, min_overlaps, compute_aos, device_id,
                                                 metric, stats_device)
    return mAP_bbox.mean(-1), mAP_bev.mean(-1), mAP_3d.mean(-1), None if mAP_aos is None else mAP_aos.mean(-1)


def get_coco_eval_result(gt_annos, dt_annos, current_classes, dataset="kitti", device_id=0, metric="new", stats_device="cpu"):
    """-> result text (eval2.py:725-784): three numbers per line for either metric."""
    current_classes = _class_ids(current_classes)
    overlap_ranges = np.zeros([3, 3, len(current_classes)])
    for i, curcls in enumerate(current_classes):
        overlap_ranges[:, :, i] = np.array(COCO_RANGE[curcls])[:, np.newaxis]
    compute_aos = _alpha_is_valid(dt_annos)
    mAPs = do_coco_style_eval(gt_annos, dt_annos, current_classes, overlap_ranges, compute_aos, dataset, device_id, metric, stats_device)
    result = ""
    for j, curcls in enumerate(current_classes):
        lo, hi, num = COCO_RANGE[curcls]
        result += _line("%s coco AP@%.2f:%.2f:%.2f:" % (CLASS_TO_NAME[curcls], lo, (hi - lo) / (num - 1), hi))
        for tag, arr in zip(("bbox AP:", "bev  AP:", "3d   AP:", "aos  AP:"), mAPs):
            if arr is not None:
                result += _line(tag + ", ".join("%.2f" % arr[j, d] for d in range(3)))
    return result


# ---------------------------------------------------------------------------------------------------
# best match and the output transformations (evaluate.py:17-81, 114-275)
# ---------------------------------------------------------------------------------------------------
def _segments(dt_annos, gt_annos):
    assert len(dt_annos) == len(gt_annos)
    n = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
    k = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
    return (np.concatenate([[0], np.cumsum(n)]).astype(np.int32), np.concatenate([[0], np.cumsum(k)]).astype(np.int32))


def _cat(arrays, width, dtype=np.float64):
    parts = [np.asarray(a, dtype=dtype).reshape((-1, width) if width else (-1,)) for a in arrays]
    return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, width) if width else (0,), dtype))


def _best_match_device(dt_annos, gt_annos, device_id=0, columns=True):
    """One prcnn_bev_best_match launch over all images.  -> dict of DEVICE tensors row_val / row_idx (/ col_val / col_idx),
    box_off / q_off, and the host offsets."""
    import torch
    box_off, q_off = _segments(dt_annos, gt_annos)
    n, k = int(box_off[-1]), int(q_off[-1])
    dev = torch.device("cuda", device_id)
    boxes = torch.from_numpy(_cat([_bev_boxes(a) for a in dt_annos], 5, np.float32)).to(dev)
    query = torch.from_numpy(_cat([_bev_boxes(a) for a in gt_annos], 5, np.float32)).to(dev)
    m = {"box_off_host": box_off, "q_off_host": q_off, "box_off": torch.from_numpy(box_off).to(dev), "q_off": torch.from_numpy(q_off).to(dev),
         "row_val": torch.empty((n,), dtype=torch.float32, device=dev), "row_idx": torch.empty((n,), dtype=torch.int32, device=dev),
         "col_val": torch.empty((k,), dtype=torch.float32, device=dev) if columns else None,
         "col_idx": torch.empty((k,), dtype=torch.int32, device=dev) if columns else None}
    with torch.cuda.device(dev):
        _lib.call("prcnn_bev_best_match", len(dt_annos), n, k, m["box_off"].data_ptr(), m["q_off"].data_ptr(), boxes.data_ptr(),
                  query.data_ptr(), -1, m["row_val"].data_ptr(), m["row_idx"].data_ptr(), _lib.ptr(m["col_val"]), _lib.ptr(m["col_idx"]),
                  _lib.current_stream(boxes))
    return m


def best_match(dt_annos, gt_annos, device="cuda", device_id=0):
    """-> (dt_matches, gt_matches): per image (val f64, idx i64) -- for every detection the largest BEV overlap with a ground-truth box
    of its image and that box's index (np.max / np.argmax: ties to the lowest index), and the same for every ground-truth box over the
    detections (evaluate.py:135-207).  An image with an empty side gives val 0, idx -1.
    device "cuda": the fused launch (no pair matrix); "cpu": numpy over calculate_iou(..., 1)."""
    if device == "cuda":
        m = _best_match_device(dt_annos, gt_annos, device_id)
        host = {key: m[key].cpu().numpy() for key in ("row_val", "row_idx", "col_val", "col_idx")}
        out = []
        for off, val, idx in ((m["box_off_host"], host["row_val"], host["row_idx"]), (m["q_off_host"], host["col_val"], host["col_idx"])):
            out.append([(val[off[i]:off[i + 1]].astype(np.float64), idx[off[i]:off[i + 1]].astype(np.int64)) for i in range(len(dt_annos))])
        return out[0], out[1]
    if device != "cpu":
        raise ValueError("device %r is neither 'cuda' nor 'cpu'" % (device,))
    dt_matches, gt_matches = [], []
    for o in calculate_iou(dt_annos, gt_annos, 1, device_id):
        for axis, other, into in ((1, 0, dt_matches), (0, 1, gt_matches)):
            if o.shape[0] > 0 and o.shape[1] > 0:
                into.append((np.max(o, axis=axis), np.argmax(o, axis=axis).astype(np.int64)))
            else:
                into.append((np.zeros(o.shape[other]), np.full(o.shape[other], -1, dtype=np.int64)))
    return dt_matches, gt_matches


def read_plane(fname):
    with open(fname) as f:
        return np.array([float(v) for v in f.readlines()[-1].split(" ")])


def annos_to_ground(annos, planes_dir, ids):
    """Drop every box onto its image's ground plane a x + b y + c z + d = 0: the last line of <planes_dir>/<id>.txt (evaluate.py:17-35)."""
    for anno, i in zip(annos, ids):
        plane = read_plane(os.path.join(planes_dir, "%06d.txt" % i))
        anno["location"][:, 1] -= (-plane[3] - plane[0] * anno["location"][:, 0] - plane[2] * anno["location"][:, 2]) / plane[1]
    return annos


def rescale_pred(annos, ratio):
    for anno in annos:
        anno["dimensions"] *= ratio
    return annos


def _align(dt_annos, gt_annos, mode, device, device_id):
    """align_size (mode 0) / align_front (mode 1), in place.  -> per image branch codes (-1 untouched; bits as prcnn_eval_align)."""
    if device == "cuda":
        import torch
        m = _best_match_device(dt_annos, gt_annos, device_id, columns=False)
        dev = m["row_val"].device
        up = lambda annos, key, w: torch.from_numpy(_cat([a[key] for a in annos], w)).to(dev)
        loc, dim = up(dt_annos, "location", 3), up(dt_annos, "dimensions", 3)
        alpha, ry, gdim = up(dt_annos, "alpha", 0), up(dt_annos, "rotation_y", 0), up(gt_annos, "dimensions", 3)
        branch = torch.empty((loc.shape[0],), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("prcnn_eval_align", len(dt_annos), loc.shape[0], m["box_off"].data_ptr(), m["q_off"].data_ptr(), loc.data_ptr(),
                      dim.data_ptr(), alpha.data_ptr(), ry.data_ptr(), gdim.data_ptr(), m["row_val"].data_ptr(), m["row_idx"].data_ptr(),
                      int(mode), branch.data_ptr(), _lib.current_stream(loc))
        loc, dim, branch, off = loc.cpu().numpy(), dim.cpu().numpy(), branch.cpu().numpy().astype(np.int64), m["box_off_host"]
        for i, anno in enumerate(dt_annos):
            anno["location"][...] = loc[off[i]:off[i + 1]]
            anno["dimensions"][...] = dim[off[i]:off[i + 1]]
        return [branch[off[i]:off[i + 1]] for i in range(len(dt_annos))]
    branches = []
    for dt, gt, (val, idx) in zip(dt_annos, gt_annos, best_match(dt_annos, gt_annos, device, device_id)[0]):
        code = np.full(len(val), -1, dtype=np.int64)
        for j in range(len(val)):
            if val[j] > ALIGN_MIN_OVERLAP:
                code[j] = 0
                if mode == 1:                          # evaluate.py:210-228
                    dist = np.linalg.norm(dt["location"][j, :])
                    alpha = dt["alpha"][j]
                    alpha = np.arctan2(np.sin(alpha), np.cos(alpha))
                    if np.abs(np.sin(alpha)) * dist > dt["dimensions"][j, 2] / 2.0:
                        shift = (dt["dimensions"][j, 2] - gt["dimensions"][idx[j], 2]) / 2.0
                        angle = -dt["rotation_y"][j] if 0 < alpha else -dt["rotation_y"][j] + np.pi
                        code[j] |= 1 | (2 if 0 < alpha else 0)
                        dt["location"][j, 0] += shift * np.cos(angle)
                        dt["location"][j, 2] += shift * np.sin(angle)
                    if np.abs(np.cos(alpha)) * dist > dt["dimensions"][j, 1] / 2.0:
                        shift = (dt["dimensions"][j, 1] - gt["dimensions"][idx[j], 1]) / 2.0
                        inner = -np.pi / 2.0 < alpha < np.pi / 2.0
                        angle = -dt["rotation_y"][j] - np.pi / 2.0 if inner else -dt["rotation_y"][j] + np.pi / 2.0
                        code[j] |= 4 | (8 if inner else 0)
                        dt["location"][j, 0] += shift * np.cos(angle)
                        dt["location"][j, 2] += shift * np.sin(angle)
                dt["dimensions"][j, :] = gt["dimensions"][idx[j], :]
        branches.append(code)
    return branches


def align_size(dt_annos, gt_annos, device="cuda", device_id=0):
    """Every detection whose best BEV overlap exceeds 0.2 takes the size of that ground-truth box (evaluate.py:187-197)."""
    _align(dt_annos, gt_annos, 0, device, device_id)
    return dt_annos


def align_front(dt_annos, gt_annos, device="cuda", device_id=0):
    """... and is first moved so that its faces towards the camera stay where they were (evaluate.py:200-229)."""
    _align(dt_annos, gt_annos, 1, device, device_id)
    return dt_annos


def get_scale_map(src, dst, form="regular"):
    """Map (n,3) dimensions (l, h, w) from the source statistics to the destination's (evaluate.py:58-81).  src / dst: the
    ``label_stats_<split>.json`` dicts of ``stat_norm stats`` (length / height / width -> mean, std)."""
    keys = ("length", "height", "width")
    if form == "regular":
        f = lambda x, s, d: x - s["mean"] + d["mean"]
    elif form == "gaussian":
        f = lambda x, s, d: (x - s["mean"]) / s["std"] * d["std"] + d["mean"]
    elif form == "log":
        f = lambda x, s, d: x / s["mean"] * d["mean"]
    else:
        raise ValueError("scale_map %r is none of regular, gaussian, log" % (form,))
    return lambda x: np.stack([f(x[:, c], src[key], dst[key]) for c, key in enumerate(keys)], axis=1)


def _stats(s):
    if isinstance(s, dict):
        return s
    with open(s) as f:
        return json.load(f)


def reverse_align(gt_annos, src_stats, dst_stats, scale_map="regular"):
    """Statistical normalization applied to the ground-truth sizes (evaluate.py:232-249); statistics as dicts or file names."""
    mapping = get_scale_map(_stats(src_stats), _stats(dst_stats), scale_map)
    for anno in gt_annos:
        if len(anno["name"]) > 0:
            anno["dimensions"] = mapping(anno["dimensions"])
    return gt_annos


def to_kitti_format(anno, extra=None):
    """Annotation -> the reference's 16-column %.2f text (kitti_common.py:293-304); ``extra``: a 17th column."""
    rows = []
    for i in range(len(anno["name"])):
        row = "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            anno["name"][i], anno["truncated"][i], anno["occluded"][i], anno["alpha"][i],
            anno["bbox"][i, 0], anno["bbox"][i, 1], anno["bbox"][i, 2], anno["bbox"][i, 3],
            anno["dimensions"][i, 1], anno["dimensions"][i, 2], anno["dimensions"][i, 0],
            anno["location"][i, 0], anno["location"][i, 1], anno["location"][i, 2], anno["rotation_y"][i], anno["score"][i])
        rows.append(row if extra is None else row + " %.2f" % extra[i])
    return "\n".join(rows)


def save_labels(annos, folder, ids, extras=None):
    assert len(annos) == len(ids)
    os.makedirs(folder, exist_ok=True)
    for n, (anno, i) in enumerate(zip(annos, ids)):
        with open(os.path.join(folder, "%06d.txt" % i), "w") as f:
            f.write(to_kitti_format(anno, None if extras is None else extras[n]))


def write_with_iou(dt_annos, gt_annos, parent, ids, device="cuda", device_id=0):
    """<parent>/with_iou: the detections with their best BEV overlap as a 17th column; <parent>/with_iou_gt: the ground truth
    with theirs (evaluate.py:130-185)."""
    dt_matches, gt_matches = best_match(dt_annos, gt_annos, device, device_id)
    save_labels(dt_annos, os.path.join(parent, "with_iou"), ids, [v for v, _ in dt_matches])
    save_labels(gt_annos, os.path.join(parent, "with_iou_gt"), ids, [v for v, _ in gt_matches])


def direct_save(result_path, text, result, toground=False, align_size=False, reverse_align=False, adapted=False):
    """Result text and per-class dict beside the run folder: <run>_val20[_ground][_align_size][_reverse_align][_adapted].txt / .pkl
    in the folder that holds <run>/<result folder> (evaluate.py:258-274).  -> the path without extension."""
    run = os.path.dirname(result_path)
    fname = os.path.basename(run) + "_val20"
    for on, tag in ((toground, "_ground"), (align_size, "_align_size"), (reverse_align, "_reverse_align"), (adapted, "_adapted")):
        if on:
            fname += tag
    base = os.path.join(os.path.dirname(run), fname)
    with open(base + ".pkl", "wb") as f:
        pickle.dump(result, f)
    with open(base + ".txt", "w") as f:
        f.write(text)
    return base


# evaluate() takes the reference's keyword names, which are these functions' names
_TRANSFORMS = {"rescale_pred": rescale_pred, "align_size": align_size, "align_front": align_front, "reverse_align": reverse_align,
               "direct_save": direct_save}


def evaluate(result_path, label_path, image_ids, current_class=0, dataset="kitti", score_thresh=-1, device_id=0, metric="new",
             coco=False, toground=False, rescale_pred=None, align_size=False, align_front=False, reverse_align=False,
             dense_sample=False, direct_save=False, output_iou=False, adapted=False, planes_path=None, src_stats=None,
             dst_stats=None, scale_map="regular", device="cuda", stats_device="cpu"):
    """Result folder + label folder + id list -> (result text, dict); the text alone with ``coco``; None with ``output_iou``
    (evaluate.py:84-275, the switches in the reference's order of application).  The transformed labels go where the reference
    puts them: grounded/, align_size/, align_front/, reverse_align/, with_iou/, with_iou_gt/ beside the result folder.
    planes_path defaults to <label folder>/../planes; reverse_align reads its two statistics from src_stats / dst_stats.
    ``device`` selects how best matches and alignment are computed ("cuda": csrc/eval_match.hip, "cpu": numpy); ``stats_device`` where
    the AP statistics run ("cpu": csrc/kitti_stats.hip's host entries, "cuda": csrc/kitti_ap.hip)."""
    _check_stats_device(stats_device)
    g = _TRANSFORMS
    image_ids = list(image_ids)
    parent = os.path.dirname(result_path)
    dt_annos = get_label_annos(result_path, image_ids)
    if score_thresh > 0:
        dt_annos = filter_annos_low_score(dt_annos, score_thresh)
    if toground:
        dt_annos = annos_to_ground(dt_annos, planes_path or os.path.join(os.path.dirname(label_path), "planes"), image_ids)
        save_labels(dt_annos, os.path.join(parent, "grounded"), image_ids)
    if rescale_pred is not None:
        dt_annos = g["rescale_pred"](dt_annos, rescale_pred)
    gt_annos = get_label_annos(label_path, image_ids)
    if output_iou:
        write_with_iou(dt_annos, gt_annos, parent, image_ids, device, device_id)
    if align_size:
        dt_annos = g["align_size"](dt_annos, gt_annos, device, device_id)
        save_labels(dt_annos, os.path.join(parent, "align_size"), image_ids)
    if align_front:
        dt_annos = g["align_front"](dt_annos, gt_annos, device, device_id)
        save_labels(dt_annos, os.path.join(parent, "align_front"), image_ids)
    if reverse_align:
        if src_stats is None or dst_stats is None:
            raise ValueError("reverse_align needs src_stats and dst_stats (label_stats_<split>.json of `stat_norm stats`)")
        gt_annos = g["reverse_align"](gt_annos, src_stats, dst_stats, scale_map)
        save_labels(gt_annos, os.path.join(parent, "reverse_align"), image_ids)
    if output_iou:
        return None
    if coco:
        return get_coco_eval_result(gt_annos, dt_annos, current_class, dataset, device_id, metric, stats_device)
    text, ret = get_official_eval_result(gt_annos, dt_annos, current_class, dataset, dense_sample, device_id, metric, stats_device)
    if direct_save:
        g["direct_save"](result_path, text, ret["result"], toground, align_size, reverse_align, adapted)
    return text, ret


def read_imageset_file(path):
    with open(path) as f:
        return [int(line) for line in f.readlines()]


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.kitti_eval", description=__doc__.split("\n")[0])
    ap.add_argument("--result_path", type=str, required=True, help="predictions to be evaluated")
    ap.add_argument("--dataset_path", type=str, default=None, help="KITTI format dataset path")
    ap.add_argument("--label_split_file", type=str, default=None, help="split file containing data ids to be evaluated")
    ap.add_argument("--label_path", type=str, default=None, help="ground truth label files")
    ap.add_argument("--metric", type=str, default="new", choices=["new", "old"], help="difficulty by [old: bbox height, new: distance]")
    ap.add_argument("--current_class", type=int, default=0, choices=range(5), help="0: Car, 1: Pedestrian, 2: Cyclist, 3: Van, 4: Person_sitting")
    ap.add_argument("--toground", action="store_true", help="move predictions to ground plane")
    ap.add_argument("--rescale_pred", type=int, default=None, help="scale all prediction boxes with this ratio")
    ap.add_argument("--align_size", action="store_true", help="set prediction box size same as ground truth")
    ap.add_argument("--align_front", action="store_true", help="align bbox's face facing camera with ground truth")
    ap.add_argument("--reverse_align", action="store_true", help="apply statistical normalization to ground truth (needs --src_stats, --dst_stats)")
    ap.add_argument("--dataset", type=str, default="kitti", choices=sorted(FOCAL), help="focal length of the old metric's height caps")
    ap.add_argument("--coco", action="store_true", help="COCO-style result (mean over ten overlap thresholds)")
    ap.add_argument("--score_thresh", type=float, default=-1)
    ap.add_argument("--dense_sample", action="store_true", help="also AP at overlap 0.00, 0.01, ..., 1.00 (new metric)")
    ap.add_argument("--direct_save", action="store_true", help="write <run>_val20[...].txt / .pkl beside the run folder")
    ap.add_argument("--output_iou", action="store_true", help="write with_iou/ and with_iou_gt/ and stop")
    ap.add_argument("--adapted", action="store_true", help="tag for the --direct_save file name")
    ap.add_argument("--src_stats", type=str, default=None, help="label_stats_<split>.json of the labels' dataset")
    ap.add_argument("--dst_stats", type=str, default=None, help="label_stats_<split>.json of the model's dataset")
    ap.add_argument("--scale_map", type=str, default="regular", choices=["regular", "gaussian", "log"])
    ap.add_argument("--device", type=str, default="cuda", choices=["cuda", "cpu"], help="best match / alignment: fused HIP launch or numpy")
    ap.add_argument("--stats_device", type=str, default="cpu", choices=["cpu", "cuda"],
                    help="AP statistics (flags, matching, PR sums): host entries or the device kernels; the same numbers")
    args = vars(ap.parse_args(argv))
    dataset_path = args.pop("dataset_path")
    split_file, label_path = args.pop("label_split_file"), args.pop("label_path")
    if dataset_path is None and (split_file is None or label_path is None):
        ap.error("give --dataset_path, or both --label_split_file and --label_path")
    split_file = split_file or os.path.join(dataset_path, "val.txt")
    label_path = label_path or os.path.join(dataset_path, "training", "label_2")
    out = evaluate(args.pop("result_path"), label_path, read_imageset_file(split_file), **args)
    if out is not None:
        print(out if isinstance(out, str) else out[0])
    return out


if __name__ == "__main__":
    main()
