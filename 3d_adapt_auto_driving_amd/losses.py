"""The training losses of both stages with their gradients (reference: lib/net/train_functions.py get_rpn_loss / get_rcnn_loss / model_fn,
lib/utils/loss_utils.py DiceLoss / SigmoidFocalClassificationLoss / get_reg_loss).  No train loop, no optimizer, no scheduler: a caller
gets a scalar with a grad_fn and the reference's tb_dict.

  res = rpn_loss(cfg, rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label)     # rpn_cls (B, N, 1) | (B, N), rpn_reg (B, N, C), labels (B, N)
                                                                           # with -1 ignore / 0 background / > 0 foreground and (B, N, 7)
  res = rcnn_loss(cfg, ret_dict)                                           # what RCNNNet.forward returns in training mode
  res.loss.backward();  res.tb_dict()
  loss, tb_dict, disp_dict = model_fn(cfg, model, data)

CUDA tensors run csrc/losses.hip through one torch.autograd.Function per call: its forward produces the value, ``parts`` and the
gradients of both predictions (four launches, no host read); its backward scales them by the incoming scalar.  CPU tensors run a
plain-torch path differentiated by torch autograd: it is the checker, not a second product path, and neither path falls back to the other.

The definition both paths implement.  Every DECISION is taken in f32 by the reference's own operation sequence: the bin labels (clamp to
[0, 2 scope - 1e-3], divide, floor), the heading chain (``%`` with the f32-rounded 2 pi as Python's remainder, the opposite-flag fold,
the clamp to [1e-3, pi/2 - 1e-3]) and, for BinaryCrossEntropy, the f32 sigmoid with torch's log clamp at -100 and its backward's
denominator floor 1e-12 (a logit saturated in f32 has loss 100 and gradient 0).  The ARITHMETIC on top of the decisions and every sum
run in f64 and are rounded to f32 once.  Entries labelled -1 and regression rows outside the mask are never read: NaN or Inf there reaches
nothing.  With no foreground row the regression terms and their gradient are zero; that branch is taken on the device.

``parts`` (f32, PARTS entries, one device tensor; ``PART_NAMES`` names them):
  0 loss  1 cls  2 reg  3 loc  4 angle  5 size (x 3)  6 cls_pos  7 cls_neg  (the focal loss's split)
  8 x_bin  9 z_bin  10 x_res  11 z_res  12 y_bin  13 y_res  14 y_offset  15 ry_bin  16 ry_res  17 size before the x 3
  18 n_pos  19 n_neg  20 n_valid  21 n_reg_fg  22 Dice sum min(p, t) m  23 Dice sum max(p, t) m
``tb_dict()`` is the batch's one device-to-host read.
"""
import collections
import ctypes as C

import numpy as np

from . import _lib

P = {name[len("PRCNN_LP_"):].lower(): i for name, i in _lib.ENUMS.items() if name.startswith("PRCNN_LP_")}   # PRCNN_LP_X_BIN -> "x_bin": 8
PART_NAMES = tuple(sorted(P, key=P.get))
PARTS = _lib.PRCNN_LOSS_PARTS
CLS_KINDS = {"DiceLoss": _lib.PRCNN_LOSS_DICE, "SigmoidFocalLoss": _lib.PRCNN_LOSS_FOCAL, "BinaryCrossEntropy": _lib.PRCNN_LOSS_BCE}

ModelReturn = collections.namedtuple("ModelReturn", ["loss", "tb_dict", "disp_dict"])


_LossArgs = _lib.struct("prcnn_loss_args")


class Spec(collections.namedtuple("Spec", ["stage", "cls_kind", "alpha", "gamma", "fg_weight", "w_cls", "w_reg", "loc_scope", "loc_bin",
                                           "nbin_head", "xz_fine", "y_by_bin", "y_scope", "y_bin", "ry_fine", "anchor", "anchor_on_roi"])):
    """One stage's loss configuration, read from cfg once"""
    @property
    def nbin_loc(self):
        return int(self.loc_scope / self.loc_bin) * 2

    @property
    def nbin_y(self):
        return int(self.y_scope / self.y_bin) * 2

    @property
    def channels(self):
        return self.nbin_loc * (4 if self.xz_fine else 2) + (2 * self.nbin_y if self.y_by_bin else 1) + 2 * self.nbin_head + 3


def rpn_spec(cfg):
    R = cfg.RPN
    if R.LOSS_CLS not in CLS_KINDS:
        raise NotImplementedError("losses: RPN.LOSS_CLS %r" % (R.LOSS_CLS,))
    return Spec("rpn", R.LOSS_CLS, float(R.FOCAL_ALPHA[0]), float(R.FOCAL_GAMMA), float(R.FG_WEIGHT), float(R.LOSS_WEIGHT[0]),
                float(R.LOSS_WEIGHT[1]), float(R.LOC_SCOPE), float(R.LOC_BIN_SIZE), int(R.NUM_HEAD_BIN), bool(R.LOC_XZ_FINE), False, 0.5, 0.25,
                False, tuple(float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32)), False)


def rcnn_spec(cfg):
    R = cfg.RCNN
    if R.LOSS_CLS == "CrossEntropy":
        raise NotImplementedError("losses: the multi-class head (RCNN.LOSS_CLS 'CrossEntropy') is out of scope")
    if R.LOSS_CLS not in ("SigmoidFocalLoss", "BinaryCrossEntropy"):
        raise NotImplementedError("losses: RCNN.LOSS_CLS %r" % (R.LOSS_CLS,))
    # (get_rcnn_loss weights neither term and gives BinaryCrossEntropy no foreground weight)
    return Spec("rcnn", R.LOSS_CLS, float(R.FOCAL_ALPHA[0]), float(R.FOCAL_GAMMA), 1.0, 1.0, 1.0, float(R.LOC_SCOPE), float(R.LOC_BIN_SIZE),
                int(R.NUM_HEAD_BIN), True, bool(R.LOC_Y_BY_BIN), float(R.LOC_Y_SCOPE), float(R.LOC_Y_BIN_SIZE), True,
                tuple(float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], dtype=np.float32)), bool(R.SIZE_RES_ON_ROI))


class LossResult:
    """loss: 0-d tensor with a grad_fn; parts: (PARTS,) f32 on the loss's device (the layout of this module's docstring)"""

    def __init__(self, spec, loss, parts):
        self.spec, self.loss, self.parts = spec, loss, parts

    def tb_dict(self):
        """The reference's dictionary for this stage and configuration: ONE device-to-host read of ``parts``"""
        v = self.parts.detach().cpu().numpy().astype(np.float64)
        g = lambda name: float(v[P[name]])
        s, d = self.spec, {}
        if s.cls_kind == "SigmoidFocalLoss":                                 # (get_rcnn_loss files its split under the rpn_ names too)
            d["rpn_loss_cls_pos"], d["rpn_loss_cls_neg"] = g("cls_pos"), g("cls_neg")
        if s.stage == "rpn":
            d.update({"rpn_loss_cls": g("cls"), "rpn_loss_reg": g("reg"), "rpn_loss": g("loss"), "rpn_fg_sum": int(v[P["n_reg_fg"]]),
                      "rpn_loss_loc": g("loc"), "rpn_loss_angle": g("angle"), "rpn_loss_size": g("size")})
            return d
        if int(v[P["n_reg_fg"]]) != 0:                                       # reg_loss_dict exists only when get_reg_loss ran
            for name in ("x_bin", "z_bin", "x_res", "z_res") + (("y_bin", "y_res") if s.y_by_bin else ("y_offset",)) + ("ry_bin", "ry_res"):
                d["loss_" + name] = g(name)
            d["loss_loc"], d["loss_angle"], d["loss_size"] = g("loc"), g("angle"), g("size_raw")
        d.update({"rcnn_loss_cls": g("cls"), "rcnn_loss_reg": g("reg"), "rcnn_loss": g("loss"), "rcnn_loss_loc": g("loc"),
                  "rcnn_loss_angle": g("angle"), "rcnn_loss_size": g("size"), "rcnn_cls_fg": int(v[P["n_pos"]]),
                  "rcnn_cls_bg": int(v[P["n_neg"]]), "rcnn_reg_fg": int(v[P["n_reg_fg"]])})
        return d


# ------------------------------------------------------------------------------------------------------------------------- cpu path
def _stage_cpu(spec, cls, reg, label, reg_mask, reg_label, anchors):
    """-> (loss with a grad_fn, parts): decisions in f32, arithmetic in f64.  Plain torch operators on the tensors' own device (the tests
    also apply these formulas to device tensors); the count of foreground rows is read on the host, as the reference reads it."""
    import torch
    import torch.nn.functional as F
    dev = cls.device
    pos, neg, valid = label > 0, label == 0, label >= 0
    n_pos, n_neg, n_valid = (m.sum().double() for m in (pos, neg, valid))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    cls_pos = cls_neg = dice_min = dice_max = zero
    if spec.cls_kind == "DiceLoss":
        keep = label != -1
        p = torch.sigmoid(torch.where(keep, cls, torch.zeros_like(cls)).double())
        t, m = label.double(), keep.double()
        dice_min, dice_max = (torch.min(p, t) * m).sum(), (torch.max(p, t) * m).sum()
        loss_cls = 1.0 - dice_min / torch.clamp(dice_max, min=1.0)
    elif spec.cls_kind == "SigmoidFocalLoss":
        x = torch.where(valid, cls, torch.zeros_like(cls)).double()
        t = pos.double()
        ce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-torch.abs(x)))
        p = torch.sigmoid(x)
        one_minus_pt = 1.0 - (t * p + (1 - t) * (1 - p))
        mod = torch.pow(one_minus_pt, spec.gamma) if spec.gamma else 1.0
        terms = mod * (t * spec.alpha + (1 - t) * (1 - spec.alpha)) * ce * (valid.double() / torch.clamp(n_pos, min=1.0))
        cls_pos, cls_neg = (terms * pos.double()).sum(), (terms * neg.double()).sum()
        loss_cls = terms.sum()
    else:
        x = torch.where(valid, cls, torch.zeros_like(cls))
        weight = torch.where(pos, torch.full_like(x, spec.fg_weight), torch.ones_like(x))
        terms = F.binary_cross_entropy(torch.sigmoid(x), pos.float(), weight=weight, reduction="none")      # f32: saturation, clamps
        loss_cls = (terms.double() * valid.double()).sum() / torch.clamp(n_valid, min=1.0)

    fg = (reg_mask > 0) if reg_mask is not None else pos
    rows = torch.nonzero(fg).view(-1)
    n_fg = rows.numel()
    comp = {k: zero for k in ("x_bin", "z_bin", "x_res", "z_res", "y_bin", "y_res", "y_offset", "ry_bin", "ry_res", "size_raw")}
    if n_fg:
        pred, lab = reg[rows].double(), reg_label[rows]
        if pred.shape[1] != spec.channels:
            raise ValueError("losses: %d regression channels, the configuration needs %d" % (pred.shape[1], spec.channels))
        ce_of = lambda l, nb, b: F.cross_entropy(pred[:, l:l + nb], b, reduction="sum") / n_fg
        sl1_of = lambda got, want: F.smooth_l1_loss(got, want, reduction="sum") / n_fg
        pick = lambda l, b: pred[:, l:].gather(1, b.view(-1, 1)).view(-1)

        def loc_bins(off32, scope, size):
            shift32 = torch.clamp(off32 + scope, 0, scope * 2 - 1e-3)
            b = (shift32 / size).floor().long()
            shift64 = torch.clamp(off32.double() + scope, 0, scope * 2 - 1e-3)
            return b, (shift64 - (b.double() * size + size / 2)) / size
        nb = spec.nbin_loc
        xb, x_res = loc_bins(lab[:, 0], spec.loc_scope, spec.loc_bin)
        zb, z_res = loc_bins(lab[:, 2], spec.loc_scope, spec.loc_bin)
        comp["x_bin"], comp["z_bin"] = ce_of(0, nb, xb), ce_of(nb, nb, zb)
        at = 2 * nb
        if spec.xz_fine:
            comp["x_res"], comp["z_res"] = sl1_of(pick(2 * nb, xb), x_res), sl1_of(pick(3 * nb, zb), z_res)
            at = 4 * nb
        if spec.y_by_bin:
            yb, y_res = loc_bins(lab[:, 1], spec.y_scope, spec.y_bin)
            comp["y_bin"], comp["y_res"] = ce_of(at, spec.nbin_y, yb), sl1_of(pick(at + spec.nbin_y, yb), y_res)
            at += 2 * spec.nbin_y
        else:
            comp["y_offset"] = sl1_of(pred[:, at], lab[:, 1].double())
            at += 1
        two_pi, ry32 = 2 * np.pi, lab[:, 6]
        if spec.ry_fine:
            apc = (np.pi / 2) / spec.nbin_head
            h32, h64 = ry32 % two_pi, ry32.double() % two_pi
            opp = (h32 > np.pi * 0.5) & (h32 < np.pi * 1.5)
            h32 = torch.where(opp, (h32 + np.pi) % two_pi, h32)
            h64 = torch.where(opp, (h64 + np.pi) % two_pi, h64)
            shift32 = torch.clamp((h32 + np.pi * 0.5) % two_pi - np.pi * 0.25, min=1e-3, max=np.pi * 0.5 - 1e-3)
            shift64 = torch.clamp((h64 + np.pi * 0.5) % two_pi - np.pi * 0.25, min=1e-3, max=np.pi * 0.5 - 1e-3)
        else:
            apc = two_pi / spec.nbin_head
            shift32 = (ry32 % two_pi + apc / 2) % two_pi
            shift64 = (ry32.double() % two_pi + apc / 2) % two_pi
        shift64 = torch.where((shift64 - shift32.double()).abs() > 1e-4, shift32.double(), shift64)   # a wrap that fell differently in f64
        rb = (shift32 / apc).floor().long()
        ry_res = (shift64 - (rb.double() * apc + apc / 2)) / (apc / 2)
        comp["ry_bin"], comp["ry_res"] = ce_of(at, spec.nbin_head, rb), sl1_of(pick(at + spec.nbin_head, rb), ry_res)
        at += 2 * spec.nbin_head
        anc = anchors[rows][:, 3:6].double() if anchors is not None else torch.tensor(spec.anchor, dtype=torch.float32, device=dev).double()
        comp["size_raw"] = sl1_of(pred[:, at:at + 3], (lab[:, 3:6].double() - anc) / anc) / 3
    loc = comp["x_bin"] + comp["z_bin"] + comp["x_res"] + comp["z_res"] + comp["y_bin"] + comp["y_res"] + comp["y_offset"]
    angle, size = comp["ry_bin"] + comp["ry_res"], 3 * comp["size_raw"]
    loss_reg = loc + angle + size
    loss = loss_cls * spec.w_cls + loss_reg * spec.w_reg
    vals = {"loss": loss, "cls": loss_cls, "reg": loss_reg, "loc": loc, "angle": angle, "size": size, "cls_pos": cls_pos, "cls_neg": cls_neg,
            "n_pos": n_pos, "n_neg": n_neg, "n_valid": n_valid, "n_reg_fg": torch.tensor(float(n_fg), dtype=torch.float64, device=dev),
            "dice_min": dice_min, "dice_max": dice_max}
    vals.update(comp)
    parts = torch.stack([torch.as_tensor(vals[k], dtype=torch.float64, device=dev).detach().reshape(()) for k in PART_NAMES]).float()
    return loss.float(), parts


# ---------------------------------------------------------------------------------------------------------------------- device path
def _device_function():
    import torch

    class StageLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, cls, reg, spec, label, reg_mask, reg_label, anchors):
            n, c, dev = cls.numel(), reg.shape[-1], cls.device
            x, r = cls.detach().contiguous().view(-1), reg.detach().contiguous().view(n, c)
            grad_cls, grad_reg = torch.empty_like(x), torch.empty_like(r)
            parts = torch.empty((PARTS,), dtype=torch.float32, device=dev)
            work = torch.empty((_lib.call("prcnn_loss_workspace"),), dtype=torch.float64, device=dev)
            a = _LossArgs(n, c, CLS_KINDS[spec.cls_kind], int(spec.xz_fine), int(spec.y_by_bin), int(spec.ry_fine), spec.nbin_loc, spec.nbin_y,
                          spec.nbin_head, spec.loc_scope, spec.loc_bin, spec.y_scope, spec.y_bin, spec.alpha, spec.gamma, spec.fg_weight,
                          spec.w_cls, spec.w_reg, (C.c_float * 3)(*spec.anchor), x.data_ptr(), label.data_ptr(),
                          None if reg_mask is None else reg_mask.data_ptr(), r.data_ptr(), reg_label.data_ptr(),
                          None if anchors is None else anchors.data_ptr(), grad_cls.data_ptr(), grad_reg.data_ptr(), parts.data_ptr(),
                          work.data_ptr())
            stream = C.c_void_p(_lib.current_stream(x))
            _lib.call("prcnn_loss_stats", C.byref(a), stream)
            _lib.call("prcnn_cls_loss", C.byref(a), stream)
            _lib.call("prcnn_reg_loss", C.byref(a), stream)
            ctx.save_for_backward(grad_cls.view(cls.shape), grad_reg.view(reg.shape))
            ctx.mark_non_differentiable(parts)
            return parts[P["loss"]].clone(), parts

        @staticmethod
        def backward(ctx, g_loss, _g_parts):
            grad_cls, grad_reg = ctx.saved_tensors
            return g_loss * grad_cls, g_loss * grad_reg, None, None, None, None, None
    return StageLoss


_StageLoss = None


def _stage(spec, cls, reg, label, reg_mask, reg_label, anchors):
    """Shape and dtype checks (raised before any launch), then the path the tensors' device selects"""
    import torch
    global _StageLoss
    for name, v in (("cls", cls), ("reg", reg), ("reg_label", reg_label)) + ((("anchors", anchors),) if anchors is not None else ()):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
            raise ValueError("losses: %s must be a float32 tensor" % name)
    for name, v in (("label", label),) + ((("reg_mask", reg_mask),) if reg_mask is not None else ()):
        if not isinstance(v, torch.Tensor) or v.is_floating_point():
            raise ValueError("losses: %s must be an integer tensor" % name)
    n = label.numel()
    c = reg.shape[-1] if reg.dim() else 0
    if n == 0 or cls.numel() != n or reg.numel() != n * c or reg_label.numel() != n * 7 or (reg_mask is not None and reg_mask.numel() != n) or \
            (anchors is not None and anchors.numel() != n * 7):
        raise ValueError("losses: shapes cls %s reg %s label %s reg_label %s" % (tuple(cls.shape), tuple(reg.shape), tuple(label.shape),
                                                                                  tuple(reg_label.shape)))
    if c != spec.channels:
        raise ValueError("losses: %d regression channels, the configuration needs %d" % (c, spec.channels))
    tensors = [cls, reg, label, reg_label] + [v for v in (reg_mask, anchors) if v is not None]
    if len({v.device for v in tensors}) != 1:
        raise ValueError("losses: the tensors are on different devices")
    label = label.reshape(-1).long().contiguous()
    reg_mask = None if reg_mask is None else reg_mask.reshape(-1).long().contiguous()
    reg_label = reg_label.detach().reshape(n, 7).contiguous()
    anchors = None if anchors is None else anchors.detach().reshape(n, 7).contiguous()
    if cls.is_cuda:
        if _StageLoss is None:
            _StageLoss = _device_function()
        loss, parts = _StageLoss.apply(cls, reg, spec, label, reg_mask, reg_label, anchors)
    else:
        loss, parts = _stage_cpu(spec, cls.reshape(-1), reg.reshape(n, c), label, reg_mask, reg_label, anchors)
    return LossResult(spec, loss, parts)


def rpn_loss(cfg, rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label):
    """get_rpn_loss"""
    return _stage(rpn_spec(cfg), rpn_cls, rpn_reg, rpn_cls_label, None, rpn_reg_label, None)


def rcnn_loss(cfg, ret_dict):
    """get_rcnn_loss on RCNNNet.forward's training-mode dictionary"""
    spec = rcnn_spec(cfg)
    return _stage(spec, ret_dict["rcnn_cls"], ret_dict["rcnn_reg"], ret_dict["cls_label"], ret_dict["reg_valid_mask"], ret_dict["gt_of_rois"],
                  ret_dict["roi_boxes3d"] if spec.anchor_on_roi else None)


RPN_ROWS = ("rpn_cls", "rpn_reg", "rpn_cls_label", "rpn_reg_label")
RCNN_ROWS = ("rcnn_cls", "rcnn_reg", "cls_label", "reg_valid_mask", "gt_of_rois", "roi_boxes3d")


def forward_rows(cfg, model, data):
    """The forward half of model_fn -> the rows the loss reads (RPN_ROWS and / or RCNN_ROWS), every one a tensor on the model's device
    whose first dimension runs over the batch's rows.  ``data`` holds tensors or numpy arrays (pts_input, gt_boxes3d, rpn_cls_label,
    rpn_reg_label with the RPN enabled; the RCNN stage's inputs without it); they are moved to the model's device."""
    import torch
    dev = next(model.parameters()).device
    to = lambda v, dtype=torch.float32: torch.as_tensor(v).to(device=dev, dtype=dtype)
    train_rpn = cfg.RPN.ENABLED and not cfg.RPN.FIXED
    if cfg.RCNN.ENABLED and not cfg.RCNN.ROI_SAMPLE_JIT:
        raise NotImplementedError("losses.model_fn: offline RoI samples (RCNN.ROI_SAMPLE_JIT off) are out of scope")
    if not train_rpn and not cfg.RCNN.ENABLED:
        raise NotImplementedError("losses.model_fn: nothing to train (the RPN is fixed or off and the RCNN is off)")
    if cfg.RPN.ENABLED:
        input_data = {"pts_input": to(data["pts_input"]), "gt_boxes3d": to(data["gt_boxes3d"])}
    else:
        input_data = {k: to(v).contiguous() for k, v in data.items() if k != "sample_id"}
    ret = model(input_data)
    rows = {}
    if train_rpn:
        rows.update(rpn_cls=ret["rpn_cls"], rpn_reg=ret["rpn_reg"], rpn_cls_label=to(data["rpn_cls_label"], torch.int64),
                    rpn_reg_label=to(data["rpn_reg_label"]))
    if cfg.RCNN.ENABLED:
        rows.update({k: ret[k] for k in RCNN_ROWS})
    return rows


def loss_of_rows(cfg, rows):
    """The loss half of model_fn on forward_rows' dictionary -> ModelReturn.  Glue: the two tb_dict() calls are its only host reads."""
    tb_dict, disp_dict, loss = {}, {}, 0
    if "rpn_cls" in rows:
        res = rpn_loss(cfg, rows["rpn_cls"], rows["rpn_reg"], rows["rpn_cls_label"], rows["rpn_reg_label"])
        tb_dict.update(res.tb_dict())
        disp_dict["rpn_loss"] = tb_dict["rpn_loss"]
        loss = loss + res.loss
    if "rcnn_cls" in rows:
        res = rcnn_loss(cfg, rows)
        tb_dict.update(res.tb_dict())
        disp_dict["reg_fg_sum"] = tb_dict["rcnn_reg_fg"]
        loss = loss + res.loss
    disp_dict["loss"] = sum(tb_dict[k] for k in ("rpn_loss", "rcnn_loss") if k in tb_dict)
    return ModelReturn(loss, tb_dict, disp_dict)


def model_fn(cfg, model, data):
    """The reference's model_fn for what this project runs: the RPN enabled and not fixed and / or the RCNN enabled with ROI_SAMPLE_JIT;
    forward_rows then loss_of_rows (data-parallel training gathers the rows over the ranks between the two: dist_train.py)."""
    return loss_of_rows(cfg, forward_rows(cfg, model, data))
