"""KITTI result text and files, AP of gathered detections, recall statistics, and the writer processes' jobs."""
import os

import numpy as np
import torch

from . import kitti_utils
from . import iou3d_utils


_RESULT_ROW = " -1 -1" + " %.4f" * 13 + "\n"


def kitti_result_text(calib, bbox3d, scores, img_shape, cls_name="Car"):
    """The result file of one scene as ONE string (tools/eval_rcnn.py:76-101 ``save_kitti_format``; pinned to the text the
    reference writes by tests/golden g11): per surviving box ``<class> -1 -1 alpha x1 y1 x2 y2 h w l x y z ry score``, %.4f.
    Whole-array form: the image boxes of all corners in one projection, clipped to the image; boxes that project wider or
    taller than 80 % of it are dropped; the observation angle alpha = ry + beta - sign(beta) * pi / 2 with beta = atan2(z, x) in the
    boxes' own precision; the 13 numeric columns of all rows go through a single format call."""
    n = int(bbox3d.shape[0])
    if n == 0:
        return ""
    bbox3d = np.asarray(bbox3d)
    img_boxes = calib.corners3d_to_img_boxes(kitti_utils.boxes3d_to_corners3d(bbox3d))[0]
    h, w = img_shape[0], img_shape[1]
    img_boxes = np.clip(img_boxes, 0, np.array([w - 1, h - 1, w - 1, h - 1]))
    ok = ((img_boxes[:, 2] - img_boxes[:, 0]) < w * 0.8) & ((img_boxes[:, 3] - img_boxes[:, 1]) < h * 0.8)
    beta = np.arctan2(bbox3d[:, 2], bbox3d[:, 0])
    alpha = -np.sign(beta) * np.pi / 2 + beta + bbox3d[:, 6]
    table = np.empty((n, 13), dtype=np.float64)
    table[:, 0] = alpha
    table[:, 1:5] = img_boxes
    table[:, 5:8] = bbox3d[:, 3:6]
    table[:, 8:11] = bbox3d[:, 0:3]
    table[:, 11] = bbox3d[:, 6]
    table[:, 12] = np.asarray(scores)
    table = table[ok]
    return ((cls_name + _RESULT_ROW) * len(table)) % tuple(table.reshape(-1).tolist())


def kitti_result_lines(calib, bbox3d, scores, img_shape, cls_name="Car"):
    """The same as a list of lines (for the in-memory AP evaluation)."""
    return kitti_result_text(calib, bbox3d, scores, img_shape, cls_name).split("\n")[:-1]


def save_kitti_format(sample_id, calib, bbox3d, kitti_output_dir, scores, img_shape, cls_name="Car"):
    """One result file per scene (empty when nothing survives); returns the number of lines."""
    text = kitti_result_text(calib, bbox3d, scores, img_shape, cls_name)
    with open(os.path.join(kitti_output_dir, "%06d.txt" % sample_id), "w") as f:
        f.write(text)
    return text.count("\n")


def detections_to_annos(table, counts, source, cls_name="Car", parse_device=None, device_id=0):
    """Gathered detection table [S, M, 9] (+ counts) -> (scene ids, KITTI annotation dicts), through the same
    %.4f text form the result files carry, so the in-memory AP equals the AP of the written files.  With ``parse_device`` the scenes'
    texts are parsed in ONE call of kitti_annos.parse_texts and the second item is its SplitSide (``.annos``: the same dicts)."""
    from . import kitti_eval
    kitti_eval._check_parse_device(parse_device)
    ids, annos = [], []
    tb, ct = table.numpy(), counts.numpy()
    for s in np.argsort(tb[:, 0, 8], kind="stable"):
        sid, n = int(tb[s, 0, 8]), int(ct[s])
        calib, shape = source.calib_and_shape(sid)
        ids.append(sid)
        if parse_device is None:
            annos.append(kitti_eval.annos_from_lines(kitti_result_lines(calib, tb[s, :n, 0:7], tb[s, :n, 7], shape, cls_name)))
        else:
            annos.append(kitti_result_text(calib, tb[s, :n, 0:7], tb[s, :n, 7], shape, cls_name))
    if parse_device is not None:
        return ids, kitti_eval.parse_texts(annos, parse_device, skip_blank=True, device_id=device_id)
    return ids, annos


def _gt_annos(source, ids, parse_device, device_id):
    """The labels of scenes ``ids``: annotation dicts by the host parser, or with ``parse_device`` and a source over label FILES
    (``label_file(id)``) their parsed SplitSide; a source that makes its label lines keeps the host parser."""
    from . import kitti_eval
    kitti_eval._check_parse_device(parse_device)
    label_file = getattr(source, "label_file", None)
    if parse_device is None or label_file is None:
        return [kitti_eval.annos_from_lines(source.label_lines(i)) for i in ids]
    def read(i):
        with open(label_file(i), "rb") as f:
            return f.read()
    return kitti_eval.parse_texts([read(i) for i in ids], parse_device, skip_blank=True, device_id=device_id)


def prepare_gt(source, ids, parse_device=None, device_id=0):
    """The labels of scenes ``ids`` (in that order) parsed and tabulated once, for evaluate_detections(prepared_gt=...)."""
    from . import kitti_eval
    return kitti_eval.PreparedGT(_gt_annos(source, ids, parse_device, device_id), ids)


def evaluate_detections(table, counts, source, current_class=0, dataset="kitti", device_id=0, metric="new", stats_device="cpu",
                        prepared_gt=None, parse_device=None):
    """Rank-0 tail of the sharded evaluation: AP of the gathered detections against the source's labels
    (tools/eval_rcnn.py:706-713 -> evaluate/evaluate.py).  Returns (result text, dict).  stats_device: where the AP statistics run
    (kitti_eval.eval_class); prepared_gt: prepare_gt(source, ids) of the same scenes, instead of parsing the labels again;
    parse_device: None for the host parser, "cuda" / "cpu" for kitti_annos.parse_texts over the scenes' result texts in one call."""
    from . import kitti_eval
    ids, dt_annos = detections_to_annos(table, counts, source, parse_device=parse_device, device_id=device_id)
    if prepared_gt is None:
        gt_annos = _gt_annos(source, ids, parse_device, device_id)
    elif prepared_gt.ids != ids:
        raise ValueError("evaluate_detections: prepared_gt was made for other scenes than the gathered table holds")
    else:
        gt_annos = prepared_gt
    return kitti_eval.get_official_eval_result(gt_annos, dt_annos, current_class, dataset, device_id=device_id, metric=metric,
                                               stats_device=stats_device)


class RecallStats:
    """Recall of the RoIs and of the refined boxes against the ground truth (eval_rcnn.py:539-570, :669-679): per scene the
    3-D IoU matrix boxes x gt through the extension's BEV overlap kernel (iou3d_utils.boxes_iou3d_gpu -> K10), a gt box
    counts as recalled at threshold t when some box overlaps it with IoU > t.  Counters stay on the device until
    ``result()``; ALL M decoded boxes of a scene enter (before score threshold and NMS), as in the reference."""
    THRESH = (0.1, 0.3, 0.5, 0.7, 0.9)

    def __init__(self, device):
        self.device = torch.device(device)
        self.rcnn = torch.zeros(len(self.THRESH), dtype=torch.int64, device=self.device)
        self.roi = torch.zeros(len(self.THRESH), dtype=torch.int64, device=self.device)
        self.total_gt = 0
        self._th = torch.tensor(self.THRESH, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def update(self, pred_boxes3d, roi_boxes3d, gt_list):
        """pred_boxes3d / roi_boxes3d (B,M,7) device; gt_list: B arrays (n_k,7) [x,y,z,h,w,l,ry] (all-zero rows = padding)"""
        for k, gt in enumerate(gt_list):
            gt = np.asarray(gt, dtype=np.float32).reshape(-1, 7)
            n = gt.shape[0]
            while n > 0 and gt[n - 1].sum() == 0:           # trailing zero padding of the collated batch (:549-552)
                n -= 1
            if n == 0:
                continue
            g = torch.from_numpy(gt[:n]).to(self.device, non_blocking=True)
            for boxes, acc in ((pred_boxes3d[k], self.rcnn), (roi_boxes3d[k], self.roi)):
                iou = iou3d_utils.boxes_iou3d_gpu(boxes.contiguous(), g)
                best = iou.max(dim=0).values
                acc += (best.unsqueeze(0) > self._th.unsqueeze(1)).sum(dim=1)
            self.total_gt += n

    def result(self):
        rcnn, roi = self.rcnn.cpu().tolist(), self.roi.cpu().tolist()
        out = {"total_gt_bbox": self.total_gt}
        for i, t in enumerate(self.THRESH):
            out["rpn_recall(thresh=%.2f)" % t] = roi[i] / max(self.total_gt, 1.0)
            out["rcnn_recall(thresh=%.2f)" % t] = rcnn[i] / max(self.total_gt, 1.0)
            out["rpn_recalled(thresh=%.2f)" % t] = roi[i]
            out["rcnn_recalled(thresh=%.2f)" % t] = rcnn[i]
        return out


def _calib_row(calib):
    """P2 | R0 | V2C of a calibration object as 33 floats (what a loader process sends back instead of the object)"""
    row = np.zeros(33, dtype=np.float32)
    row[0:12] = np.asarray(calib.P2, np.float32).reshape(-1)
    r0, v2c = getattr(calib, "R0", None), getattr(calib, "V2C", None)
    row[12:21] = (np.eye(3, dtype=np.float32) if r0 is None else np.asarray(r0, np.float32)).reshape(-1)
    row[21:33] = (np.eye(3, 4, dtype=np.float32) if v2c is None else np.asarray(v2c, np.float32)).reshape(-1)
    return row


class _RowCalib:
    """the parent's side of _calib_row: projection for the result writer + the arrays DeviceInputStage.pack_calib reads"""

    def __init__(self, row):
        self.P2, self.R0, self.V2C = row[0:12].reshape(3, 4), row[12:21].reshape(3, 3), row[21:33].reshape(3, 4)

    def corners3d_to_img_boxes(self, corners3d):
        n = corners3d.shape[0]
        hom = np.concatenate((corners3d, np.ones((n, 8, 1))), axis=2)
        img = np.matmul(hom, self.P2.T)
        x, y = img[:, :, 0] / img[:, :, 2], img[:, :, 1] / img[:, :, 2]
        boxes = np.stack((np.min(x, axis=1), np.min(y, axis=1), np.max(x, axis=1), np.max(y, axis=1)), axis=1)
        return boxes, np.stack((x, y), axis=2)


def _write_batch(ids, calibs, shapes, boxes, scores, output_dir, cls_name):
    """one writer job: the KITTI result files of one batch (runs in a writer process)"""
    return sum(save_kitti_format(sid, c, b, output_dir, s, sh, cls_name) for sid, c, sh, b, s in zip(ids, calibs, shapes, boxes, scores))


def _write_rpn_batch(ids, calibs, shapes, rois, scores, seg, feats, output_dir, cls_name):
    """one writer job of --eval_mode rpn (eval_rcnn.py:212-229): detections/data/%06d.txt (every RoI, save_kitti_format),
    seg_result/%06d.npy and, with ``feats``, the features/ files of save_rpn_features (:104-117)"""
    det_dir, seg_dir = os.path.join(output_dir, "detections", "data"), os.path.join(output_dir, "seg_result")
    for k, sid in enumerate(ids):
        save_kitti_format(sid, calibs[k], rois[k], det_dir, scores[k], shapes[k], cls_name)
        np.save(os.path.join(seg_dir, "%06d.npy" % sid), seg[k].astype(np.float16))
        if feats is not None:
            fdir = os.path.join(output_dir, "features")
            for suffix, arr in feats[k].items():
                np.save(os.path.join(fdir, "%06d%s.npy" % (sid, suffix)), arr)
    return len(ids)
