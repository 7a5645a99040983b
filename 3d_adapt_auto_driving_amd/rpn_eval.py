"""RPN evaluation (tools/eval_rcnn.py:120-260 eval_one_epoch_rpn): per-point RPN labels and the mode's statistics.

  rpn_labels(pts, gt, counts, device)   generate_rpn_training_labels (kitti_rcnn_dataset.py:385-414) for a batch of ragged scenes;
                                        device="cuda" runs csrc/rpn_labels.hip, device="cpu" is the numpy restatement (the checker)
  pack_gt(gt_list)                      per-scene (g_k, 7) boxes -> (B, G, 7) f32, counts, numpy's f32 (cos, sin) of ry
  RpnStats                              segmentation IoU and proposal recall, counters on the device until result()

Labels: boxes are visited in order and a later box overrides an earlier one.  A point inside box k gets 1 and the regression target
(center - pt with the center lifted by h / 2, then h, w, l, ry); a point inside exactly one of box k and its enlarged box
(enlarge_box3d(0.2)) gets -1.  "Inside" is the reference's kitti_utils.in_hull -- Delaunay(corners).find_simplex(p) >= 0 -- restated
without scipy: the convex hull of the 8 f32 corners as 12 facet triangles in f64, a point within 100 eps of a facet (relative to the
hull's extent normal to it) counts as inside, a hull without volume (QhullError) is empty.  Corners: numpy's f32 cos / sin of ry, then
np.matmul's order (a product per term, one add), pinned by tests/golden g16.  Every operation of the numpy path has the kernel's order.

Recall quirk, reproduced on purpose: the reference trims a scene's zero padding with ``while k > 0 and ...`` (eval_rcnn.py:190-192).
A scene without GT keeps one all-zero row -- one unrecalled GT -- whenever another scene of its collated batch has GT; a batch in
which no scene has GT counts none.  The counts therefore depend on the batching: they equal the reference's at the same batch size
and one rank.
"""
import ctypes as C

import numpy as np

THRESH = (0.1, 0.3, 0.5, 0.7, 0.9)
_EPS100 = 100.0 * 2.220446049250313e-16
_FACES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7))
_SX = np.array([1, 1, -1, -1, 1, 1, -1, -1], dtype=np.float32)
_SZ = np.array([1, -1, -1, 1, 1, -1, -1, 1], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ packing
def pack_gt(gt_list, G=None):
    """gt_list: B arrays (g_k, 7) [x, y, z, h, w, l, ry] -> gt (B, G, 7) f32 (zero rows past each count), counts (B,) i32,
    trig (B, G, 2) f32 = numpy's np.cos / np.sin of the f32 angle (the reference's boxes3d_to_corners3d calls them)."""
    arrs = [np.asarray(g, dtype=np.float32).reshape(-1, 7) for g in gt_list]
    counts = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    G = int(max(counts.max(initial=0), G or 0))
    gt = np.zeros((len(arrs), G, 7), dtype=np.float32)
    for i, a in enumerate(arrs):
        gt[i, :a.shape[0]] = a
    ry = gt[:, :, 6]
    trig = np.stack([np.cos(ry), np.sin(ry)], axis=2).astype(np.float32)
    return gt, counts, trig


# ------------------------------------------------------------------------------------------------------------ numpy restatement
def box_corners(boxes, cos, sin):
    """(K, 7) f32 boxes, (K,) f32 cos / sin -> (K, 8, 3) f32: kitti_utils.boxes3d_to_corners3d(rotate=True) in its f32 order"""
    f32 = np.float32
    x, y, z, h, w, l = (boxes[:, j:j + 1] for j in range(6))
    c, s = cos.reshape(-1, 1).astype(f32), sin.reshape(-1, 1).astype(f32)
    xc = (l / f32(2)) * _SX
    zc = (w / f32(2)) * _SZ
    xr = xc * c + zc * s
    zr = xc * (-s) + zc * c
    yc = np.repeat(y, 8, axis=1)
    yc[:, 4:] = y + (-h)
    return np.stack([x + xr, yc, z + zr], axis=2).astype(f32)


def _facet(P, ia, ib, ic):
    """P (K, 8, 3) f64 -> planes (K, 7) [n, a, tol] oriented outward and supporting (K,) bool; csrc/rpn_labels.hip facet()"""
    a = P[:, ia]
    e1, e2 = P[:, ib] - a, P[:, ic] - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    d = P - a[:, None, :]
    v = (n[:, None, 0] * d[:, :, 0] + n[:, None, 1] * d[:, :, 1]) + n[:, None, 2] * d[:, :, 2]
    smin = np.minimum(v.min(axis=1), 0.0)
    smax = np.maximum(v.max(axis=1), 0.0)
    flip = ~(smax <= 0.0) & (smin >= 0.0)
    H = np.where(smax <= 0.0, -smin, np.where(smin >= 0.0, smax, -1.0))
    n = np.where(flip[:, None], -n, n)
    tol = _EPS100 * np.where(H > 0.0, H, 0.0)
    return np.concatenate([n, a, tol[:, None]], axis=1), H >= 0.0


def hull_planes(corners):
    """(K, 8, 3) f32 corners -> planes (K, 12, 7) f64, valid (K,) bool (the hull has volume)"""
    P = corners.astype(np.float64)
    out, valid = [], np.ones(P.shape[0], dtype=bool)
    for q0, q1, q2, q3 in _FACES:
        p0, s0 = _facet(P, q0, q1, q2)
        p1, s1 = _facet(P, q0, q2, q3)
        b0, _ = _facet(P, q0, q1, q3)
        b1, _ = _facet(P, q1, q2, q3)
        use_a = (s0 & s1)[:, None]
        p0, p1 = np.where(use_a, p0, b0), np.where(use_a, p1, b1)
        valid &= (p0[:, 6] > 0.0) & (p1[:, 6] > 0.0)
        out += [p0, p1]
    return np.stack(out, axis=1), valid


def in_hull(pts, planes, valid):
    """pts (N, 3) f32, planes (12, 7) f64 of ONE hull -> (N,) bool"""
    if not valid:
        return np.zeros(pts.shape[0], dtype=bool)
    p = pts.astype(np.float64)
    inside = np.ones(p.shape[0], dtype=bool)
    for pl in planes:
        v = (pl[0] * (p[:, 0] - pl[3]) + pl[1] * (p[:, 1] - pl[4])) + pl[2] * (p[:, 2] - pl[5])
        inside &= v <= pl[6]
    return inside


def _labels_cpu(pts, gt, trig, want_reg):
    f32 = np.float32
    n = pts.shape[0]
    cls = np.zeros(n, dtype=np.int32)
    reg = np.zeros((n, 7), dtype=np.float32) if want_reg else None
    if gt.shape[0] == 0:
        return cls, reg
    big = gt.copy()
    big[:, 3:6] += f32(0.4)
    big[:, 1] += f32(0.2)
    pl0, v0 = hull_planes(box_corners(gt, trig[:, 0], trig[:, 1]))
    pl1, v1 = hull_planes(box_corners(big, trig[:, 0], trig[:, 1]))
    for k in range(gt.shape[0]):
        fg = in_hull(pts, pl0[k], v0[k])
        cls[fg] = 1
        cls[fg != in_hull(pts, pl1[k], v1[k])] = -1
        if want_reg:
            center = gt[k, 0:3].copy()
            center[1] -= gt[k, 3] / f32(2)
            reg[fg, 0:3] = center - pts[fg]
            reg[fg, 3:7] = gt[k, 3:7]
    return cls, reg


def seg_decision(scores_raw, thresh):
    """numpy: sigmoid(raw) > thresh with one f32 rounding per operation (the kernels' rpn_seg_fg)"""
    f32 = np.float32
    raw = np.asarray(scores_raw, dtype=f32)
    with np.errstate(over="ignore"):
        sg = f32(1) / (f32(1) + np.exp(-raw))
    return sg > f32(thresh)


def seg_counts(cls, pred):
    """(..., N) labels and predictions -> (..., 3) int64 (correct, fg, pred) (eval_rcnn.py:205-207)"""
    fg = cls > 0
    return np.stack([(pred & fg).sum(-1), fg.sum(-1), pred.sum(-1)], axis=-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- public
def rpn_labels(pts, gt, counts, device="cpu", want_reg=True, trig=None, scores_raw=None, thresh=None, stats=None):
    """RPN labels of a batch.  pts (B, N, 3) f32 rect points (numpy or torch); gt (B, G, 7) f32 packed with counts (B,);
    trig (B, G, 2) numpy's f32 (cos, sin) of ry (pack_gt; computed here from gt when None).
    -> cls (B, N) int32 and reg (B, N, 7) float32 (None with want_reg=False), numpy for device="cpu", torch tensors on the device
    otherwise.  With ``scores_raw`` (B, N) and ``thresh`` the per-scene counters (correct, fg, pred) are added into ``stats``
    (B, 3): a device int32 tensor for "cuda" (one atomic per wave and scene inside the kernel), a numpy int64 array for "cpu"."""
    dev = str(device)
    if dev != "cpu" and not dev.startswith("cuda"):
        raise ValueError("device must be 'cpu' or 'cuda[:i]'")
    gt_np = gt.detach().cpu().numpy() if hasattr(gt, "detach") else np.asarray(gt, dtype=np.float32)
    counts_np = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts, dtype=np.int32).reshape(-1)
    if trig is None:
        ry = gt_np[..., 6].astype(np.float32)
        trig = np.stack([np.cos(ry), np.sin(ry)], axis=-1).astype(np.float32)
    if dev == "cpu":
        P = pts.detach().cpu().numpy() if hasattr(pts, "detach") else np.asarray(pts, dtype=np.float32)
        B, N = P.shape[0], P.shape[1]
        cls = np.zeros((B, N), dtype=np.int32)
        reg = np.zeros((B, N, 7), dtype=np.float32) if want_reg else None
        for s in range(B):
            g = int(counts_np[s])
            c, r = _labels_cpu(np.ascontiguousarray(P[s, :, :3], dtype=np.float32), gt_np[s, :g], trig[s, :g], want_reg)
            cls[s] = c
            if want_reg:
                reg[s] = r
        if scores_raw is not None and stats is not None:
            sc = scores_raw.detach().cpu().numpy() if hasattr(scores_raw, "detach") else np.asarray(scores_raw)
            stats += seg_counts(cls, seg_decision(sc, thresh))
        return cls, reg
    return _labels_device(pts, gt_np, counts_np, np.asarray(trig, dtype=np.float32), want_reg, scores_raw, thresh, stats, device)


def _labels_device(pts, gt_np, counts_np, trig, want_reg, scores_raw, thresh, stats, device):
    import torch
    from . import _lib
    if not torch.is_tensor(pts):
        pts = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32))
    pts = pts.to(device)
    if pts.shape[-1] != 3 or not pts.is_contiguous():
        pts = pts[..., :3].contiguous()
    B, N = int(pts.shape[0]), int(pts.shape[1])
    G = int(gt_np.shape[1]) if gt_np.ndim == 3 else 0
    if counts_np.shape[0] != B or (counts_np > G).any() or (counts_np < 0).any():
        raise ValueError("rpn_labels: counts must be (B,) with 0 <= count <= G")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device, non_blocking=True)
    t_cnt = t(counts_np, np.int32)
    t_gt = t(gt_np, np.float32) if G else None
    t_trig = t(trig, np.float32) if G else None
    nbytes = C.c_longlong(0)
    _lib.call("prcnn_rpn_labels_workspace", B, G, C.byref(nbytes))
    work = torch.empty((max(1, nbytes.value // 8),), dtype=torch.float64, device=pts.device) if G else None
    cls = torch.empty((B, N), dtype=torch.int32, device=pts.device)
    reg = torch.empty((B, N, 7), dtype=torch.float32, device=pts.device) if want_reg else None
    sc = None
    if scores_raw is not None and stats is not None:
        sc = scores_raw.contiguous()
        if sc.dtype != torch.float32 or tuple(sc.shape) != (B, N) or stats.dtype != torch.int32 or tuple(stats.shape) != (B, 3):
            raise ValueError("rpn_labels: scores_raw must be (B, N) f32 and stats (B, 3) int32")
    _lib.call("prcnn_rpn_labels", B, N, G, pts.data_ptr(), _lib.ptr(t_gt), t_cnt.data_ptr(), _lib.ptr(t_trig), _lib.ptr(sc),
              float(thresh if thresh is not None else 0.0), cls.data_ptr(), _lib.ptr(reg), _lib.ptr(stats if sc is not None else None),
              _lib.ptr(work), C.c_void_p(_lib.current_stream(pts)))
    return cls, reg


def reference_trim(counts):
    """per-scene GT rows that eval_one_epoch_rpn's recall loop keeps for a collated batch with these GT counts (the quirk above)"""
    counts = [int(c) for c in counts]
    G = max(counts, default=0)
    if G == 0:
        return [0] * len(counts)
    return [c if c > 0 else 1 for c in counts]


class RpnStats:
    """eval_one_epoch_rpn's statistics: the per-scene segmentation IoU correct / max(fg + pred - correct, 1) averaged over the
    scenes, and the recall of the M proposals at IoU 0.1 ... 0.9 (iou3d_utils.boxes_iou3d_gpu, as RecallStats).  The counters
    stay on the device until result()."""
    THRESH = THRESH

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self.recalled = torch.zeros(len(THRESH), dtype=torch.int64, device=self.device)
        self._ious = []                       # per batch the scenes' f32 IoUs, on the device
        self.seg = torch.zeros(3, dtype=torch.int64, device=self.device)
        self.total_gt = 0
        self.scenes = 0
        self._th = torch.tensor(THRESH, dtype=torch.float32, device=self.device)

    def update_seg(self, counters):
        """counters (B, 3) (correct, fg, pred) of one batch, device int32 (the label kernel's) -> per-scene IoU, computed in f32
        like the reference's ``correct / clamp(union, 1)``; result() adds them as Python floats one scene at a time, in scene order,
        as the reference does."""
        import torch
        c = counters.to(torch.float32)
        self._ious.append(c[:, 0] / torch.clamp(c[:, 1] + c[:, 2] - c[:, 0], min=1.0))
        self.seg += counters.to(torch.int64).sum(0)
        self.scenes += int(counters.shape[0])

    def update_recall(self, rois, gt_list):
        """rois (B, M, 7) device; gt_list: the batch's per-scene (g_k, 7) boxes (no padding).  Trimmed as the reference does."""
        import torch
        from . import iou3d_utils
        keep = reference_trim([np.asarray(g).reshape(-1, 7).shape[0] for g in gt_list])
        for k, gt in enumerate(gt_list):
            n = keep[k]
            if n == 0:
                continue
            g = np.zeros((n, 7), dtype=np.float32)
            real = np.asarray(gt, dtype=np.float32).reshape(-1, 7)
            g[:real.shape[0]] = real
            gd = torch.from_numpy(g).to(self.device, non_blocking=True)
            best = iou3d_utils.boxes_iou3d_gpu(rois[k].contiguous(), gd).max(dim=0).values
            self.recalled += (best.unsqueeze(0) > self._th.unsqueeze(1)).sum(dim=1)
            self.total_gt += n

    def result(self):
        rec = self.recalled.cpu().tolist()
        seg = self.seg.cpu().tolist()
        iou_sum = 0.0
        if self._ious:
            import torch
            for v in torch.cat(self._ious).cpu().tolist():
                iou_sum += v
        out = {"max_obj_num": 0, "rpn_iou": iou_sum / max(self.scenes, 1), "total_gt_bbox": self.total_gt,
               "seg_correct": seg[0], "seg_fg": seg[1], "seg_pred": seg[2], "scenes": self.scenes}
        for i, t in enumerate(THRESH):
            out["rpn_recall(thresh=%.2f)" % t] = rec[i] / max(self.total_gt, 1.0)
            out["rpn_recalled(thresh=%.2f)" % t] = rec[i]
        return out

    def summary_lines(self, epoch_id="no_number", result_dir=""):
        """the reference's closing log lines (eval_rcnn.py:236-258)"""
        r = self.result()
        lines = ["-------------------performance of epoch %s---------------------" % epoch_id,
                 "max number of objects: %d" % r["max_obj_num"], "rpn iou avg: %f" % r["rpn_iou"]]
        for t in THRESH:
            lines.append("total bbox recall(thresh=%.3f): %d / %d = %f" % (t, r["rpn_recalled(thresh=%.2f)" % t], r["total_gt_bbox"],
                                                                          r["rpn_recall(thresh=%.2f)" % t]))
        lines.append("result is saved to: %s" % result_dir)
        return lines
