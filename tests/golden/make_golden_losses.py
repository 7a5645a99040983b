"""Generates tests/golden/g23_losses_ref.npz: the REFERENCE's own get_rpn_loss / get_rcnn_loss (lib/net/train_functions.py) and
get_reg_loss (lib/utils/loss_utils.py) on the seeded batches of tests/losses_batch.py, with torch.autograd.grad with respect to the
predictions, once in f32 and once in f64.

RUN IN THE BUILD CONTAINER ONLY (imports the reference through ref_harness, read-only):
    python tests/golden/make_golden_losses.py

The f64 run feeds the same functions ``.double()`` predictions, regression labels and RoI boxes: the reference accepts them in every
case recorded here, no numpy evaluation is needed.  One shim, for both runs: this torch's F.binary_cross_entropy refuses a target
outside [0, 1] and a float target next to a double input, and get_rcnn_loss hands it the labels themselves, -1 included, and masks the
ignored entries afterwards; while the reference runs, F.binary_cross_entropy is wrapped to see those targets as 0 and in the input's
dtype.  Value and gradient of every entry the reference keeps are untouched.
The f64 run gives every output its own rounding scale e_ref = |ref32 - ref64| (for a gradient: the maximum over the tensor).

Per case (tests/losses_batch.py CASES; B = 2, N = 700 for the RPN, 2 x 64 rows for the RCNN):
  <case>_ref32 / _ref64   (PARTS) f64 in losses.PART_NAMES order (NaN where the reference has no such output)
  <case>_gcls32 (n) f32, <case>_gcls64 (n) f64          d loss / d cls in full
  <case>_rows (fg) i64, <case>_greg64 (fg, C) f64, <case>_greg_eref   the regression gradient's foreground rows (the others are asserted
                                                         to be zero) and max |g32 - g64|
  <case>_cls (n), <case>_label (n), <case>_reg_fg (fg, C), <case>_reg_label_fg (fg, 7) [, _reg_mask (n), _roi_fg (fg, 7)]   the inputs
  <case>_tb_keys  json list: the reference's tb_dict keys;  cases  json: what the batches contain
The generator asserts a margin of 1e-3 bin between every bin decision and its nearest edge (1e-3 rad around the heading's fold and wrap
points) and that the batches contain every case the fixture was built for; it fails with "change the batch or the seed" otherwise.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as H  # noqa: E402
import losses_batch as LB  # noqa: E402

MARGIN = 1e-3
FAIL = ": change the batch or the seed"
LIMIT = 425000


def closures(fn):
    return {n: c.cell_contents for n, c in zip(fn.__code__.co_freevars, fn.__closure__)}


def margins(spec, b, cases):
    """every bin decision of the foreground rows, in f64: at least MARGIN bins from an edge (an offset clamped to exactly 0 aside)"""
    fg = (b["reg_mask"] > 0) if "reg_mask" in b else (b["label"] > 0)
    lab = b["reg_label"][fg].astype(np.float64)

    def loc(v, scope, size, what):
        shift = np.clip(v + scope, 0, 2 * scope - 1e-3)
        q = shift / size
        frac = q - np.floor(q)
        ok = (shift == 0) | ((frac >= MARGIN) & (frac <= 1 - MARGIN))
        assert ok.all(), "a %s bin decision within 1e-3 bin of an edge" % what + FAIL
        cases["offset_clamped_low"] += int((v + scope < 0).sum())
        cases["offset_clamped_high"] += int((v + scope > 2 * scope - 1e-3).sum())
    loc(lab[:, 0], spec.loc_scope, spec.loc_bin, "x")
    loc(lab[:, 2], spec.loc_scope, spec.loc_bin, "z")
    if spec.y_by_bin:
        loc(lab[:, 1], spec.y_scope, spec.y_bin, "y")
    ry, two_pi = lab[:, 6], 2 * np.pi
    h = ry % two_pi
    cases["heading_zero"] += int((ry == 0).sum())
    cases["heading_negative"] += int((ry < 0).sum())
    cases["heading_above_2pi"] += int((ry > two_pi).sum())
    wrap = np.minimum(h, two_pi - h)
    assert ((ry == 0) | (wrap >= MARGIN)).all(), "a heading within 1e-3 of a multiple of 2 pi" + FAIL
    if spec.ry_fine:
        apc = (np.pi / 2) / spec.nbin_head
        assert (np.abs(h - np.pi / 2) >= MARGIN).all() and (np.abs(h - 3 * np.pi / 2) >= MARGIN).all(), "a heading within 1e-3 of the fold" + FAIL
        opp = (h > np.pi / 2) & (h < 3 * np.pi / 2)
        cases["heading_folded"] += int(opp.sum())
        h = np.where(opp, (h + np.pi) % two_pi, h)
        shift = np.clip((h + np.pi / 2) % two_pi - np.pi / 4, 1e-3, np.pi / 2 - 1e-3)
    else:
        apc = two_pi / spec.nbin_head
        pre = h + apc / 2
        assert (np.abs(pre - two_pi) >= MARGIN).all(), "a shifted heading within 1e-3 of 2 pi" + FAIL
        shift = pre % two_pi
    q = shift / apc
    frac = q - np.floor(q)
    assert ((frac >= MARGIN) & (frac <= 1 - MARGIN)).all(), "a heading bin decision within 1e-3 bin of an edge" + FAIL


def set_cfg(cfg, name):
    stage, _kind, over = LB.CASES[name]
    ours = LB.case_cfg(name)
    node, mine = cfg[stage.upper()], ours[stage.upper()]
    for k in ("LOSS_CLS", "FOCAL_ALPHA", "FOCAL_GAMMA", "LOC_SCOPE", "LOC_BIN_SIZE", "NUM_HEAD_BIN"):
        node[k] = mine[k]
    if stage == "rpn":
        for k in ("LOC_XZ_FINE", "FG_WEIGHT", "LOSS_WEIGHT"):
            node[k] = mine[k]
        cfg.RPN.ENABLED, cfg.RPN.FIXED, cfg.RCNN.ENABLED = True, False, False
    else:
        for k in ("LOC_Y_BY_BIN", "LOC_Y_SCOPE", "LOC_Y_BIN_SIZE", "SIZE_RES_ON_ROI"):
            node[k] = mine[k]
    cfg.CLS_MEAN_SIZE = np.asarray(ours.CLS_MEAN_SIZE, dtype=np.float32)


def reference_run(name, b, spec, double):
    """-> (values by part name, d loss / d cls, d loss / d reg, tb keys)"""
    import torch
    import torch.nn.functional as F
    from lib.config import cfg
    import lib.net.train_functions as TF
    import lib.utils.loss_utils as LU
    stage = LB.CASES[name][0]
    set_cfg(cfg, name)
    fns = closures(TF.model_joint_fn_decorator())
    fl = (lambda a: torch.from_numpy(a).double()) if double else torch.from_numpy
    n, c = b["label"].shape[0], b["reg"].shape[1]
    cls, reg = fl(b["cls"]).requires_grad_(True), fl(b["reg"]).requires_grad_(True)
    label, reg_label = torch.from_numpy(b["label"]), fl(b["reg_label"])
    tb = {}
    if stage == "rpn":
        node = cfg.RPN
        func = {"DiceLoss": LU.DiceLoss(ignore_target=-1), "BinaryCrossEntropy": F.binary_cross_entropy,
                "SigmoidFocalLoss": LU.SigmoidFocalClassificationLoss(alpha=node.FOCAL_ALPHA[0], gamma=node.FOCAL_GAMMA)}[node.LOSS_CLS]
        model = types.SimpleNamespace(rpn=types.SimpleNamespace(rpn_cls_loss_func=func))
        shape = LB.RPN_SHAPE
        fg = label > 0
        kw = dict(loc_scope=node.LOC_SCOPE, loc_bin_size=node.LOC_BIN_SIZE, num_head_bin=node.NUM_HEAD_BIN,
                  anchor_size=torch.from_numpy(cfg.CLS_MEAN_SIZE[0]), get_xz_fine=node.LOC_XZ_FINE, get_y_by_bin=False, get_ry_fine=False)
        call = lambda: fns["get_rpn_loss"](model, cls.view(shape + (1,)), reg.view(shape + (c,)), label.view(shape), reg_label.view(shape + (7,)), tb)
    else:
        node = cfg.RCNN
        func = F.binary_cross_entropy if node.LOSS_CLS == "BinaryCrossEntropy" else \
            LU.SigmoidFocalClassificationLoss(alpha=node.FOCAL_ALPHA[0], gamma=node.FOCAL_GAMMA)
        model = types.SimpleNamespace(rcnn_net=types.SimpleNamespace(cls_loss_func=func))
        mask, roi = torch.from_numpy(b["reg_mask"]), fl(b["roi"])
        fg = mask > 0
        ret = {"rcnn_cls": cls, "rcnn_reg": reg, "cls_label": label, "reg_valid_mask": mask, "roi_boxes3d": roi, "gt_of_rois": reg_label,
               "pts_input": torch.zeros((n, 1, 1))}
        kw = dict(loc_scope=node.LOC_SCOPE, loc_bin_size=node.LOC_BIN_SIZE, num_head_bin=node.NUM_HEAD_BIN,
                  anchor_size=roi[:, 3:6][fg] if node.SIZE_RES_ON_ROI else torch.from_numpy(cfg.CLS_MEAN_SIZE[0]), get_xz_fine=True,
                  get_y_by_bin=node.LOC_Y_BY_BIN, loc_y_scope=node.LOC_Y_SCOPE, loc_y_bin_size=node.LOC_Y_BIN_SIZE, get_ry_fine=True)
        call = lambda: fns["get_rcnn_loss"](model, ret, tb)
    n_fg = int(fg.sum())
    comp = {}
    if n_fg:                                                                  # the components: the reference's own get_reg_loss on the fg rows
        _loc, _angle, _size, d = LU.get_reg_loss(reg.detach()[fg], reg_label[fg], **kw)
        comp = {k[5:]: float(v) for k, v in d.items() if k not in ("loss_loc", "loss_angle", "loss_size")}
        comp["size_raw"] = float(d["loss_size"])
    real_bce = F.binary_cross_entropy
    # shim (see the header): ignored targets -1 -> 0 (masked out afterwards by the reference), the target in the input's dtype
    F.binary_cross_entropy = lambda inp, target, weight=None, **k: real_bce(inp, target.clamp(min=0).to(inp.dtype), weight=weight, **k)
    try:
        loss = call()
    finally:
        F.binary_cross_entropy = real_bce
    g = torch.autograd.grad(loss, [cls, reg], allow_unused=True)
    gcls = np.zeros(n) if g[0] is None else g[0].numpy().astype(np.float64)
    greg = np.zeros((n, c)) if g[1] is None else g[1].numpy().astype(np.float64)
    p = "rpn" if stage == "rpn" else "rcnn"
    vals = {"loss": tb[p + "_loss"], "cls": tb[p + "_loss_cls"], "reg": tb[p + "_loss_reg"], "loc": tb[p + "_loss_loc"],
            "angle": tb[p + "_loss_angle"], "size": tb[p + "_loss_size"], "n_pos": float((label > 0).sum()), "n_neg": float((label == 0).sum()),
            "n_valid": float((label >= 0).sum()), "n_reg_fg": float(n_fg)}
    if "rpn_loss_cls_pos" in tb:
        vals["cls_pos"], vals["cls_neg"] = tb["rpn_loss_cls_pos"], tb["rpn_loss_cls_neg"]
    assert int(tb["rpn_fg_sum"] if stage == "rpn" else tb["rcnn_reg_fg"]) == n_fg
    vals.update(comp)
    return {k: float(v) for k, v in vals.items()}, gcls, greg, sorted(tb)


def main():
    H.install()
    L = LB.L()
    out = {"seed": np.int64(LB.SEED)}
    cases = {k: 0 for k in ("offset_clamped_low", "offset_clamped_high", "heading_zero", "heading_negative", "heading_above_2pi", "heading_folded",
                            "sl1_below_1", "sl1_above_1", "logit_20", "logit_90", "no_positive", "dice_union_below_1", "no_fg_row", "all_fg_rows",
                            "ignored_labels", "c46", "c52", "c53", "c76", "size_on_roi", "size_on_mean")}
    for kind in ("DiceLoss", "SigmoidFocalLoss", "BinaryCrossEntropy"):
        cases["rpn_" + kind] = 0
    for kind in ("SigmoidFocalLoss", "BinaryCrossEntropy"):
        cases["rcnn_" + kind] = 0
    for name, (stage, kind, _over) in LB.CASES.items():
        spec, b = LB.case_spec(name), LB.case_batch(name)
        margins(spec, b, cases)
        v32, gc32, gr32, keys = reference_run(name, b, spec, double=False)
        v64, gc64, gr64, _keys = reference_run(name, b, spec, double=True)
        fg = (b["reg_mask"] > 0) if "reg_mask" in b else (b["label"] > 0)
        assert not gr32[~fg].any() and not gr64[~fg].any(), "a gradient row outside the mask is not zero"
        for tag, vals in (("ref32", v32), ("ref64", v64)):
            out["%s_%s" % (name, tag)] = np.array([vals.get(k, np.nan) for k in L.PART_NAMES], dtype=np.float64)
        out[name + "_gcls32"], out[name + "_gcls64"] = gc32.astype(np.float32), gc64
        out[name + "_rows"], out[name + "_greg64"] = np.nonzero(fg)[0].astype(np.int64), gr64[fg]
        out[name + "_greg_eref"] = np.float64(np.abs(gr32 - gr64).max(initial=0.0))
        out[name + "_cls"], out[name + "_label"] = b["cls"], b["label"].astype(np.int8)
        out[name + "_reg_fg"], out[name + "_reg_label_fg"] = b["reg"][fg], b["reg_label"][fg]
        if stage == "rcnn":
            out[name + "_reg_mask"], out[name + "_roi_fg"] = b["reg_mask"].astype(np.int8), b["roi"][fg]
        out[name + "_tb_keys"] = np.array(json.dumps(keys))
        # what the case contains
        cases["%s_%s" % (stage, spec.cls_kind)] += 1
        cases["c%d" % spec.channels] += 1
        cases["size_on_roi" if spec.anchor_on_roi else "size_on_mean"] += int(fg.any())
        live = b["label"] >= 0
        cases["logit_20"] += int((np.abs(b["cls"][live]) == 20).sum() >= 2 and (b["cls"][live] == 20).any() and (b["cls"][live] == -20).any())
        cases["logit_90"] += int((b["cls"][live] == -90).any() and ((b["cls"][live] == 90).any() or kind == "nopos"))
        cases["no_positive"] += int(not (b["label"] > 0).any())
        cases["dice_union_below_1"] += int(spec.cls_kind == "DiceLoss" and out[name + "_ref64"][L.P["cls"]] == 1.0 - 0.0 and not (b["label"] > 0).any())
        cases["no_fg_row"] += int(not fg.any())
        cases["all_fg_rows"] += int(fg.all())
        cases["ignored_labels"] += int((b["label"] == -1).any())
        if fg.any():                                                         # smooth-L1 arguments on both sides of 1: the size columns
            anc = b["roi"][fg][:, 3:6] if spec.anchor_on_roi else np.asarray(spec.anchor)
            d = np.abs(b["reg"][fg][:, -3:] - (b["reg_label"][fg][:, 3:6] - anc) / anc)
            cases["sl1_below_1"] += int((d < 1).sum())
            cases["sl1_above_1"] += int((d > 1).sum())
        print(name, "loss32 %.9g loss64 %.17g fg %d" % (v32["loss"], v64["loss"], int(fg.sum())))
    # the Dice union of the no-positive batch, from the inputs
    b = LB.case_batch("rpn_dice_nopos")
    keep = b["label"] != -1
    union = float((1.0 / (1.0 + np.exp(-b["cls"][keep].astype(np.float64)))).sum())
    assert union < 1.0, "the Dice union of the no-positive batch is %.3g" % union + FAIL
    cases["dice_union_below_1"] = 1
    for k, v in cases.items():
        assert v > 0, "the batches contain no case of: %s" % k + FAIL
    out["cases"] = np.array(json.dumps(cases))
    print(cases)
    path = os.path.join(HERE, "g23_losses_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < LIMIT, "the fixture is not below g22's size"


if __name__ == "__main__":
    main()
