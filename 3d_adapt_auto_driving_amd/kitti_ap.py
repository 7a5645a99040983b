"""The AP statistics of the offline evaluator (evaluate/eval2.py:8-98, 460-544; evaluate/eval_old.py:28-91): the protocol's
constants, the per-image bookkeeping (clean_data) and the recall thresholds, the split as one table of columns (SplitTable) with
clean_data over all of it at once (split_flags), and the statistics over that table as stages -- flags, overlaps, scores,
thresholds, pr, eval_class -- on two backends with the same stage names:

  HostStats    the host entries of csrc/kitti_stats.hip (pass 1 ``prcnn_kitti_collect_scores``, pass 2
               ``prcnn_kitti_accumulate_pr``) and the closed-form threshold rule; numpy in, numpy out.
  DeviceStats  the kernels of csrc/kitti_ap.hip; device tensors between the stages and one read at the end.

Both give the same bits.  kitti_ap_result.py turns their sums into curves, mAPs and the result texts."""
import ctypes

import numpy as np

from . import _lib
from .kitti_annos import PreparedGT, SplitSide
from .kitti_overlaps import calculate_iou

CLASS_NAMES = ["car", "pedestrian", "cyclist"]
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting"}
SIBLING_CODE = {0: 3, 1: 4}                                                                # Van for Car, Person_sitting for Pedestrian
DIST_BOUNDARY = np.array([[0, 0, 0, 0, 30, 50], [30, 70, 70, 30, 50, 70]], dtype=np.float64)
MAX_OCCLUSION = [0, 1, 2, 2, 2, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5, 0.5, 0.5, 0.5]
N_SAMPLE_PTS = 41
# metric="old" (eval_old.py:28-39): bbox-height caps of KITTI's easy / moderate / hard, scaled from KITTI's focal length to the dataset's
FOCAL = {"kitti": 707.05, "argo": 1870.57, "nusc": 1266.42, "lyft": 811.16, "waymo": 2069.82}
OLD_MAX_OCCLUSION = [0, 1, 2]
OLD_MAX_TRUNCATION = [0.15, 0.3, 0.5]
REG_DETS = _lib.PRCNN_AP_REG_DETS                    # detections per image whose scan flags the kernels keep in registers


def min_height(dataset):
    return (np.array([40, 25, 25]) / FOCAL["kitti"] * FOCAL[dataset]).tolist()


def _difficulties(metric):
    if metric not in ("new", "old"):
        raise ValueError("metric %r is neither 'new' (distance) nor 'old' (bbox height)" % (metric,))
    return [0, 1, 2, 3, 4, 5] if metric == "new" else [0, 1, 2]


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


def thresholds_loop(sorted_scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """The reference's loop as written (evaluate/eval2.py:8-25) over scores already in descending order: the definition of
    prcnn_ap_thresholds (get_thresholds is its closed form)."""
    current_recall, thresholds, n = 0, [], len(sorted_scores)
    for i, score in enumerate(sorted_scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


class SplitTable:
    """Both sides of a split and what pairs them: per-image offsets of ground truth, detections, DontCare rows and (n_dt x n_gt)
    pair blocks; ``dc_rows``: the ground-truth rows named DontCare, in order.  Built in whole-array numpy, once per evaluation,
    for either backend; ``gt_annos`` may be a PreparedGT, and either side a SplitSide (kitti_annos.parse_texts makes one)."""

    def __init__(self, gt_annos, dt_annos):
        self.gt = gt_annos.side if isinstance(gt_annos, PreparedGT) else gt_annos if isinstance(gt_annos, SplitSide) else SplitSide(gt_annos)
        self.dt = dt_annos if isinstance(dt_annos, SplitSide) else SplitSide(dt_annos)
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
    rows = [[OLD_MAX_OCCLUSION[d], OLD_MAX_TRUNCATION[d], 0.0, 0.0, min_height(dataset)[d]] if metric == "old" else
            [MAX_OCCLUSION[d], MAX_TRUNCATION[d], DIST_BOUNDARY[0, d], DIST_BOUNDARY[1, d], 0.0] for d in difficultys]
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(-1, 5))


def split_flags(table, current_class, dataset, difficulty, metric="new"):
    """clean_data for every image of the split at once -> ignored_gt (n_gt) i64, ignored_dt (n_dt) i64, num_valid_gt, dc_bboxes
    (n_dc, 4): the concatenation of what clean_data gives image by image; the host path's flags and the definition of
    prcnn_ap_flags."""
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


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pair_cos(table):
    """(n_pair) f64: (1 + cos(gt alpha - dt alpha)) / 2 per pair in the overlap blocks' layout, by the library's host entry"""
    out = np.zeros((int(table.pair_off[-1]),), dtype=np.float64)
    _lib.call("prcnn_kitti_pair_cos", table.n_img, _ptr(table.gt_off), _ptr(table.dt_off), _ptr(table.pair_off),
              _ptr(table.gt.alpha), _ptr(table.dt.alpha), _ptr(out))
    return out


def _flat_overlaps(blocks, n_pair):
    """A caller's per-image (n_dt, n_gt) blocks, as they are -> (n_pair) f64"""
    flat = np.concatenate([np.asarray(o, dtype=np.float64).reshape(-1) for o in blocks]) if len(blocks) else np.zeros((0,))
    if flat.shape[0] != n_pair:
        raise ValueError("overlaps hold %d pairs, the split has %d" % (flat.shape[0], n_pair))
    return np.ascontiguousarray(flat, dtype=np.float64)


class HostStats:
    """A SplitTable in the layout the host entries of csrc/kitti_stats.hip read, and DeviceStats's stages over it in numpy.  What
    no class or difficulty changes -- gt_datas = [bbox | alpha], dt_datas = [bbox | alpha | score], the DontCare boxes, the three
    count vectors -- is built once, here.  A group is one (difficulty, level) pair, difficulty-major, as on the device."""

    def __init__(self, table, device_id=0):
        self.table, self.device_id = table, device_id
        self._flags, self._overlaps = {}, {}
        gt, dt = table.gt, table.dt
        self.gt_datas = np.ascontiguousarray(np.concatenate([gt.bbox, gt.alpha[:, None]], 1))
        self.dt_datas = np.ascontiguousarray(np.concatenate([dt.bbox, dt.alpha[:, None], dt.score[:, None]], 1))
        self.gt_nums, self.dt_nums, self.dc_nums = table.gt_nums, table.dt_nums, np.diff(table.dc_off)
        self.dontcares = table.dc_bbox

    def flags(self, current_class, dataset, difficultys, metric="new"):
        """-> ignored_gt (n_diff, n_gt) i64, ignored_dt (n_diff, n_dt) i64, num_valid_gt (n_diff) i64: split_flags, kept per key"""
        key = (current_class, dataset if metric == "old" else None, tuple(difficultys), metric)
        if key not in self._flags:
            rows = [split_flags(self.table, current_class, dataset, d, metric) for d in difficultys]
            self._flags[key] = tuple(np.ascontiguousarray(np.stack([r[c] for r in rows]), dtype=np.int64) for c in (0, 1, 2))
        return self._flags[key]

    def overlaps(self, kind):
        """-> (n_pair) f64, the flat concatenation of calculate_iou(dt, gt, kind)'s blocks; kept per kind"""
        if kind not in self._overlaps:
            blocks = calculate_iou(self.table.dt.annos, self.table.gt.annos, kind, self.device_id)
            self._overlaps[kind] = _flat_overlaps(blocks, int(self.table.pair_off[-1]))
        return self._overlaps[kind]

    def scores(self, flags, overlaps, kind, min_overlaps):
        """Pass 1 -> per group the scores of the matched valid ground-truth boxes, in image order"""
        out = []
        for ig, idt in zip(flags[0], flags[1]):
            for level in min_overlaps:
                scores, n = np.zeros((max(1, len(self.table.gt)),), dtype=np.float64), ctypes.c_longlong(0)
                _lib.call("prcnn_kitti_collect_scores", self.table.n_img, _ptr(self.gt_nums), _ptr(self.dt_nums), _ptr(overlaps),
                          _ptr(self.gt_datas), _ptr(self.dt_datas), _ptr(ig), _ptr(idt), int(kind), float(level), _ptr(scores),
                          ctypes.cast(ctypes.pointer(n), ctypes.c_void_p))
                out.append(scores[:n.value].copy())
        return out

    def thresholds(self, scores, num_valid_gt):
        """get_thresholds per group -> list of (n_thr) f64"""
        per = len(scores) // max(1, len(num_valid_gt))
        return [np.array(get_thresholds(s, int(num_valid_gt[g // per])), dtype=np.float64) for g, s in enumerate(scores)]

    def pr(self, flags, overlaps, kind, min_overlaps, thr, compute_aos):
        """Pass 2 and the sums -> per group (n_thr, 4) f64 = [tp, fp, fn, similarity]"""
        out = [np.zeros([len(t), 4]) for t in thr]
        for l, (ig, idt) in enumerate(zip(flags[0], flags[1])):
            for k, level in enumerate(min_overlaps):
                g = l * len(min_overlaps) + k
                if len(thr[g]):
                    _lib.call("prcnn_kitti_accumulate_pr", self.table.n_img, _ptr(self.gt_nums), _ptr(self.dt_nums), _ptr(self.dc_nums),
                              _ptr(overlaps), _ptr(self.gt_datas), _ptr(self.dt_datas), _ptr(self.dontcares), _ptr(ig), _ptr(idt),
                              int(kind), float(level), _ptr(thr[g]), len(thr[g]), int(bool(compute_aos)), _ptr(out[g]))
        return out

    def eval_class(self, current_classes, dataset, difficultys, kind, min_overlaps, compute_aos=False, overlaps=None,
                   difficulty_metric="new"):
        """-> pr (n_class, n_diff, n_lev, 41, 4) f64 and n_thr (n_class, n_diff, n_lev) int, as DeviceStats.eval_class"""
        ov = self.overlaps(kind) if overlaps is None else _flat_overlaps(overlaps, int(self.table.pair_off[-1]))
        n_cls, n_diff, n_lev = len(current_classes), len(difficultys), len(min_overlaps)
        pr, n_thr = np.zeros((n_cls, n_diff * n_lev, N_SAMPLE_PTS, 4)), np.zeros((n_cls, n_diff * n_lev), dtype=np.int64)
        for m, current_class in enumerate(current_classes):
            flags = self.flags(current_class, dataset, difficultys, difficulty_metric)
            levels = np.asarray(min_overlaps[:, kind, m], dtype=np.float64)
            thr = self.thresholds(self.scores(flags, ov, kind, levels), flags[2])
            for g, rows in enumerate(self.pr(flags, ov, kind, levels, thr, compute_aos)):
                pr[m, g, :len(rows)], n_thr[m, g] = rows, len(rows)
        return pr.reshape(n_cls, n_diff, n_lev, N_SAMPLE_PTS, 4), n_thr.reshape(n_cls, n_diff, n_lev)


class StatsDeviceError(RuntimeError):
    """stats_device="cuda" was asked for and no GPU is usable.  There is no fallback to the host path."""


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
        self.seg_off = (up(dt.off32), up(gt.off32))                                  # what the segmented rotated-IoU launch takes
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
                self._call("prcnn_rotate_iou_eval_segmented", self.table.n_img, self.n_pair, _lib.ptr(self.t["pair_off"]),
                           _lib.ptr(self.seg_off[0]), _lib.ptr(self.seg_off[1]), _lib.ptr(self.t["dt_bev"]), _lib.ptr(self.t["gt_bev"]),
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
            ov = self.overlaps(kind) if overlaps is None else self._up(_flat_overlaps(overlaps, self.n_pair))
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
