"""From the AP statistics to the results (evaluate/eval2.py:545-784, evaluate/eval_old.py:619-695): the 41-sample curves of every
(class, difficulty, level) group, the 11-point mAP, the three overlap kinds over one split table (do_eval), and the official and
COCO-style result texts.  Where the statistics run is ``stats_device``: kitti_ap.HostStats or kitti_ap.DeviceStats."""
import io

import numpy as np

from .kitti_annos import SplitSide, _check_parse_device, parse_texts
from .kitti_ap import CLASS_TO_NAME, DeviceStats, HostStats, SplitTable, _difficulties


def _check_stats_device(stats_device):
    if stats_device not in ("cpu", "cuda"):
        raise ValueError("stats_device %r is neither 'cpu' nor 'cuda'" % (stats_device,))


def _sides(gt_annos, dt_annos, parse_device, device_id):
    """``parse_device`` of the entry points below: a side given as TEXTS (one str / bytes per image, a file's content each) is parsed
    by kitti_annos.parse_texts on that device -> its SplitSide; annotation dicts, a SplitSide or a PreparedGT pass as they are"""
    _check_parse_device(parse_device)
    texts = lambda side: isinstance(side, (list, tuple)) and len(side) > 0 and all(isinstance(t, (str, bytes)) for t in side)
    if parse_device is None:
        return gt_annos, dt_annos
    return tuple(parse_texts(side, parse_device, device_id=device_id) if texts(side) else side for side in (gt_annos, dt_annos))


def _backend(gt_annos, dt_annos, stats_device, device_id, parse_device=None):
    _check_stats_device(stats_device)
    gt_annos, dt_annos = _sides(gt_annos, dt_annos, parse_device, device_id)
    return (DeviceStats if stats_device == "cuda" else HostStats)(SplitTable(gt_annos, dt_annos), device_id)


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
               device_id=0, overlaps=None, difficulty_metric="new", stats_device="cpu", split=None, parse_device=None):
    """-> dict(recall, precision, orientation), each [num_class, num_difficulty, num_minoverlap, 41]
    (eval2.py:460-569).  min_overlaps: [num_minoverlap, metric, num_class].  ``metric`` is the overlap kind (0 image box / 1 BEV /
    2 3D) as in the reference; the difficulty rule ("new" | "old", the ``metric`` keyword everywhere else) is ``difficulty_metric``.
    stats_device "cpu": the host entries of csrc/kitti_stats.hip; "cuda": flags, overlaps, both passes, thresholds and sums on the
    device (csrc/kitti_ap.hip) with one read at the end -- the same bits.  ``split``: a HostStats / DeviceStats of these
    annotations to reuse; when given, IT is the backend and stats_device / device_id are not looked at.  ``parse_device``: _sides."""
    if split is None:
        split = _backend(gt_annos, dt_annos, stats_device, device_id, parse_device)
    pr, n_thr = split.eval_class(current_classes, dataset, difficultys, metric, min_overlaps, compute_aos, overlaps, difficulty_metric)
    precision, recall, aos = np.zeros(pr.shape[:4]), np.zeros(pr.shape[:4]), np.zeros(pr.shape[:4])
    for m, l, k in np.ndindex(*n_thr.shape):
        _fill_curves(precision[m, l, k], recall[m, l, k], aos[m, l, k], pr[m, l, k, :n_thr[m, l, k]], compute_aos)
    return {"recall": recall, "precision": precision, "orientation": aos}


def get_mAP(prec):
    """11-point interpolated AP in percent from the 41-sample precision curve: the samples at recall 0, 0.1, ..., 1 (every 4th one),
    added left to right (a cumulative sum: the reference's order of additions, evaluate/eval2.py:572-576), over 11."""
    return np.cumsum(prec[..., ::4], axis=-1)[..., -1] / 11 * 100


def do_eval(gt_annos, dt_annos, current_classes, dataset, min_overlaps, compute_aos=False, device_id=0, metric="new", stats_device="cpu",
            parse_device=None):
    difficultys = _difficulties(metric)
    # either path builds the split table (and its uploads) once; the three overlap kinds share it and the flags
    more = {"difficulty_metric": metric, "split": _backend(gt_annos, dt_annos, stats_device, device_id, parse_device)}
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
    if isinstance(dt_annos, SplitSide):                # the first row of the first image that has one
        return bool(len(dt_annos) and dt_annos.alpha[0] != -10)
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(anno["alpha"][0] != -10)
    return False


def get_official_eval_result(gt_annos, dt_annos, current_classes, dataset="kitti", dense_sample=False, device_id=0, metric="new",
                             stats_device="cpu", parse_device=None):
    """-> (result text, dict) in the reference's format (eval2.py:629-722; metric="old": eval_old.py:619-695, three numbers per
    line and no dense sampling).  ``parse_device``: _sides."""
    gt_annos, dt_annos = _sides(gt_annos, dt_annos, parse_device, device_id)
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
    result, res = "", {}
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
                       stats_device="cpu", parse_device=None):
    """mAP averaged over ten overlap thresholds (eval2.py:611-626).  overlap_ranges: [lo / hi / count, overlap kind, num_class].
    The reference's call of do_eval is one argument short since ``dataset`` joined its signature; this passes it."""
    min_overlaps = np.zeros([10, *overlap_ranges.shape[1:]])
    for i in range(overlap_ranges.shape[1]):
        for j in range(overlap_ranges.shape[2]):
            lo, hi, num = overlap_ranges[:, i, j]
            min_overlaps[:, i, j] = np.linspace(lo, hi, int(num))
    mAP_bbox, mAP_bev, mAP_3d, mAP_aos = do_eval(gt_annos, dt_annos, current_classes, dataset, min_overlaps, compute_aos, device_id,
                                                 metric, stats_device, parse_device)
    return mAP_bbox.mean(-1), mAP_bev.mean(-1), mAP_3d.mean(-1), None if mAP_aos is None else mAP_aos.mean(-1)


def get_coco_eval_result(gt_annos, dt_annos, current_classes, dataset="kitti", device_id=0, metric="new", stats_device="cpu",
                         parse_device=None):
    """-> result text (eval2.py:725-784): three numbers per line for either metric.  ``parse_device``: _sides."""
    gt_annos, dt_annos = _sides(gt_annos, dt_annos, parse_device, device_id)
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
