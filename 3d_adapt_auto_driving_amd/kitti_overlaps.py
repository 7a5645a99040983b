"""The evaluator's three overlap kinds (image box / BEV / 3D; evaluate/eval2.py:102-161, 352-427) and the best match of every box
with the other side of its image (evaluate/evaluate.py:135-207).  The rotated kinds are one block-diagonal launch over the split
(``prcnn_rotate_iou_eval_segmented``); ``best_match(device="cuda")`` is one fused launch that never writes the pair matrix
(``prcnn_bev_best_match``, csrc/eval_match.hip).  A stand-in for the rotated IoU (oracle.ext_cpu.patch_package) is installed
under its public name, ``kitti_eval.rotate_iou_segmented``: see ``_rotated``."""
import sys

import numpy as np

from . import _lib
from .kitti_annos import SplitSide, _bev_boxes, _cat, _d3_boxes


def image_box_overlap(boxes, query_boxes, criterion=-1):
    """(N,4) x (K,4) [x1,y1,x2,y2] -> (N,K) in boxes.dtype (eval2.py:102-128): no +1 on the extents."""
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
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
        b = torch.from_numpy(_cat(boxes_list, 5, np.float32)).to(dev)
        q = torch.from_numpy(_cat(query_list, 5, np.float32)).to(dev)
        oo, bo, qo = (torch.from_numpy(a).to(dev) for a in (out_off, box_off, q_off))
        out = torch.empty((total,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("prcnn_rotate_iou_eval_segmented", nseg, total, oo.data_ptr(), bo.data_ptr(), qo.data_ptr(),
                      b.data_ptr(), q.data_ptr(), out.data_ptr(), int(criterion), _lib.current_stream(out))
        flat = out.cpu().numpy()
    blocks = [flat[out_off[i]:out_off[i + 1]].reshape(int(n[i]), int(k[i])) for i in range(nseg)]
    return blocks, flat


def _rotated():
    """rotate_iou_segmented, or what a caller has put under that public name in kitti_eval (nothing is imported here)"""
    return getattr(sys.modules.get(__package__ + ".kitti_eval"), "rotate_iou_segmented", rotate_iou_segmented)


def calculate_iou(dt_annos, gt_annos, metric, device_id=0):
    """Per-image overlap blocks (n_dt_i, n_gt_i) f64 for metric 0 image box / 1 BEV / 2 3D
    (eval2.py:352-427 called with (dt, gt) as at :492)."""
    assert len(gt_annos) == len(dt_annos)
    if metric == 0:
        return [image_box_overlap(d["bbox"], g["bbox"]) for d, g in zip(dt_annos, gt_annos)]
    if metric == 1:
        blocks, _ = _rotated()([_bev_boxes(d) for d in dt_annos], [_bev_boxes(g) for g in gt_annos], -1, device_id)
        return [b.astype(np.float64) for b in blocks]
    if metric == 2:
        db, gb = [_d3_boxes(d) for d in dt_annos], [_d3_boxes(g) for g in gt_annos]
        blocks, _ = _rotated()([b[:, [0, 2, 3, 5, 6]] for b in db], [b[:, [0, 2, 3, 5, 6]] for b in gb], 2, device_id)
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


def _best_match_device(dt, gt, device_id=0, columns=True):
    """One prcnn_bev_best_match launch over all images of the two SplitSides.  -> dict of DEVICE tensors row_val / row_idx
    (/ col_val / col_idx) and the i32 offsets box_off / q_off."""
    import torch
    assert dt.n_img == gt.n_img
    n, k = len(dt), len(gt)
    dev = torch.device("cuda", device_id)
    boxes, query = torch.from_numpy(dt.bev).to(dev), torch.from_numpy(gt.bev).to(dev)
    m = {"box_off": torch.from_numpy(dt.off32).to(dev), "q_off": torch.from_numpy(gt.off32).to(dev),
         "row_val": torch.empty((n,), dtype=torch.float32, device=dev), "row_idx": torch.empty((n,), dtype=torch.int32, device=dev),
         "col_val": torch.empty((k,), dtype=torch.float32, device=dev) if columns else None,
         "col_idx": torch.empty((k,), dtype=torch.int32, device=dev) if columns else None}
    with torch.cuda.device(dev):
        _lib.call("prcnn_bev_best_match", dt.n_img, n, k, m["box_off"].data_ptr(), m["q_off"].data_ptr(), boxes.data_ptr(),
                  query.data_ptr(), -1, m["row_val"].data_ptr(), m["row_idx"].data_ptr(), _lib.ptr(m["col_val"]), _lib.ptr(m["col_idx"]),
                  _lib.current_stream(boxes))
    return m


def best_match(dt_annos, gt_annos, device="cuda", device_id=0):
    """-> (dt_matches, gt_matches): per image (val f64, idx i64) -- for every detection the largest BEV overlap with a ground-truth box
    of its image and that box's index (np.max / np.argmax: ties to the lowest index), and the same for every ground-truth box over the
    detections (evaluate.py:135-207).  An image with an empty side gives val 0, idx -1.
    device "cuda": the fused launch (no pair matrix); "cpu": numpy over calculate_iou(..., 1)."""
    if device == "cuda":
        dt, gt = SplitSide(dt_annos, SplitSide.BOX_KEYS), SplitSide(gt_annos, SplitSide.BOX_KEYS)
        m = _best_match_device(dt, gt, device_id)
        host = {key: m[key].cpu().numpy() for key in ("row_val", "row_idx", "col_val", "col_idx")}
        cut = lambda off, val, idx: [(val[off[i]:off[i + 1]].astype(np.float64), idx[off[i]:off[i + 1]].astype(np.int64)) for i in range(dt.n_img)]
        return cut(dt.off, host["row_val"], host["row_idx"]), cut(gt.off, host["col_val"], host["col_idx"])
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
