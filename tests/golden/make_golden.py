"""Generates the committed golden fixtures under tests/golden/*.npz.

RUN IN THE BUILD CONTAINER ONLY (needs /root/reference, read-only):   python tests/golden/make_golden.py
The fixtures are DATA (inputs + expected outputs); no reference source is stored.  Sources of truth:

  g5_roipool_ref.npz   outputs of the REFERENCE's own compiled CPU code (oracle/_ref = roipool3d.cpp
                       built by oracle/Makefile): pts_in_boxes3d_cpu, roipool3d_cpu
  g7_glue_ref.npz      outputs of the reference's importable Python glue: decode_bbox_target (both
                       flag sets used on the path), boxes3d_to_bev_torch, enlarge_box3d,
                       rotate_pc_along_y_torch, boxes3d_to_corners3d, Calibration.corners3d_to_img_boxes
  g8i_e2e_tiny_intensity_ref.npz  the same with cfg.RPN.USE_INTENSITY = True and a 4-channel input
  g8_e2e_tiny_ref.npz  the reference PointRCNN (imported under tests/golden/ref_harness.py shims, oracle
                       operator backend) on a tiny config: weights, input, rois, rcnn_cls, rcnn_reg and the
                       final boxes produced with the reference's own decode + nms_gpu sequence
                       (eval_rcnn.py:516-530,611-629)
  g9_rotate_iou_ref.npz  the reference's OWN evaluate/rotate_iou.py (K18: host function + kernel + device functions) run by the
                       numba / numba.cuda interpreter of tests/golden/numba_shim.py (numba's float32 typing rules
                       reproduced) on 256 x 256 centre-format boxes: random, identical, touching, nested, thin,
                       axis-aligned and far-apart pairs, all four criteria, plus the mask of pairs that overrun
                       the reference's 8-point intersection buffer (undefined behaviour on CUDA)
  g9l_rotate_iou_sample_ref.npz  the same interpreter run on a second, independent random sample (70 x 20 boxes, criteria -1 / 1)
  g14_kitti_labels_ref.npz  the reference's KittiRCNNDataset.filtrate_objects + objs_to_boxes3d (EVAL and TRAIN mode) on a
                       seven-line label file (stored in the fixture)
  g10_ap_eval_ref.npz  the reference's AP evaluator (evaluate/eval2.py imported with ``numba.jit`` shimmed to the
                       identity, an empty ``skimage`` stand-in for kitti_common's unused import, and its ``rotate_iou`` dependency -- a numba.cuda module -- IMPORTED FROM THE
                       REFERENCE and run by the same interpreter; round 2 fed it the oracle's K18 restatement) on 60 synthetic label / result files (the reference needs >= 50 images: it cuts the split into 50 parts): label lines in, mAP arrays,
                       precision / recall curves and the result text out
  g_ops_oracle.npz     oracle outputs for ball query / FPS / three_nn / group / NMS / overlap / rotate_iou
                       on small seeded inputs with the edge cases of SURVEY.md section 8c (regression pins; the
                       tests also check them against independent numpy brute force)
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_harness as H  # noqa: E402
from oracle import oracle as O  # noqa: E402
import helpers  # noqa: E402

TINY = {  # G8 tiny configuration: same topology as default.yaml, ~60 k parameters
    "RPN": {"NUM_POINTS": 2048,
            "SA_CONFIG": {"NPOINTS": [512, 128, 32, 8],
                          "MLPS": [[[8, 8, 16], [8, 8, 16]], [[16, 16, 32], [16, 16, 32]],
                                   [[32, 32, 32], [32, 32, 32]], [[32, 32, 64], [32, 32, 64]]]},
            "FP_MLPS": [[128, 128], [32, 32], [32, 32], [32, 32]],
            "CLS_FC": [32], "REG_FC": [32]},
    "RCNN": {"XYZ_UP_LAYER": [128, 128], "NUM_POINTS": 128,
             "SA_CONFIG": {"NPOINTS": [32, 8, -1], "NSAMPLE": [16, 16, 16],
                           "MLPS": [[32, 32, 32], [32, 32, 64], [64, 64, 64]]},
             "CLS_FC": [32, 32], "REG_FC": [32, 32]},
    "TEST": {"RPN_PRE_NMS_TOP_N": 600, "RPN_POST_NMS_TOP_N": 20},
}


def g5():
    ref = O.load_reference_roipool()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    rng = np.random.default_rng(50)
    pts = rng.uniform([-12, 0, 18], [12, 3, 42], (4096, 3)).astype(np.float32)   # dense patch
    boxes = helpers.boxes3d(rng, 16, xz_scope=((-10, 10), (20, 40)))
    boxes[3, :3] = [300, 300, 300]                     # empty
    boxes[0] = [0, 2.6, 30, 4, 30, 30, 0.3]            # > 512 points
    boxes[1, :3] = pts[7] + [0, 0.8, 0]                # a handful of points
    feat = rng.standard_normal((4096, 9)).astype(np.float32)
    flag = torch.zeros((16, 4096), dtype=torch.long)
    ref.pts_in_boxes3d_cpu(flag, torch.from_numpy(pts), torch.from_numpy(boxes))
    pp, pf, pe = torch.zeros(16, 512, 3), torch.zeros(16, 512, 9), torch.zeros(16, dtype=torch.long)
    ref.roipool3d_cpu(torch.from_numpy(pts), torch.from_numpy(boxes), torch.from_numpy(feat), pp, pf, pe)
    np.savez_compressed(os.path.join(HERE, "g5_roipool_ref.npz"), pts=pts, boxes=boxes, feat=feat,
                        pts_flag=flag.numpy().astype(np.uint8), pooled_pts=pp.numpy(),
                        pooled_features=pf.numpy(),
                        pooled_empty_flag=pe.numpy())
    print("g5: hits per box", flag.sum(1).tolist())


def g7():
    H.install()
    from lib.utils.bbox_transform import decode_bbox_target
    import lib.utils.kitti_utils as ku
    from lib.utils.calibration import Calibration
    rng = np.random.default_rng(70)
    anchor = torch.tensor([1.52563191462, 1.62856739989, 3.88311640418])
    out = {}
    # RPN flavour (proposal_layer.py:23-30): points (N,3), 76 channels, xz fine, full-circle heading
    xyz = torch.from_numpy(rng.uniform([-40, -1, 0], [40, 3, 70], (300, 3)).astype(np.float32))
    reg = torch.from_numpy(rng.standard_normal((300, 76)).astype(np.float32))
    out["rpn_xyz"], out["rpn_reg"] = xyz.numpy(), reg.numpy()
    out["rpn_boxes"] = decode_bbox_target(xyz.clone(), reg.clone(), anchor_size=anchor, loc_scope=3.0, loc_bin_size=0.5,
                                          num_head_bin=12, get_xz_fine=True, get_y_by_bin=False,
                                          get_ry_fine=False).numpy()
    # RCNN flavour (eval_rcnn.py:516-523): RoIs (N,7), 46 channels, fine heading
    rois = torch.from_numpy(helpers.boxes3d(rng, 200))
    reg2 = torch.from_numpy(rng.standard_normal((200, 46)).astype(np.float32))
    out["rcnn_rois"], out["rcnn_reg"] = rois.numpy(), reg2.numpy()
    out["rcnn_boxes"] = decode_bbox_target(rois.clone(), reg2.clone(), anchor_size=anchor, loc_scope=1.5, loc_bin_size=0.5,
                                           num_head_bin=9, get_xz_fine=True, get_y_by_bin=False, loc_y_scope=0.5,
                                           loc_y_bin_size=0.25, get_ry_fine=True).numpy()
    out["bev"] = ku.boxes3d_to_bev_torch(rois).numpy()
    out["enlarged"] = ku.enlarge_box3d(rois, 1.0).numpy()
    pc = torch.from_numpy(rng.standard_normal((200, 16, 5)).astype(np.float32))
    out["rot_pc_in"] = pc.numpy().copy()
    out["rot_pc_out"] = ku.rotate_pc_along_y_torch(pc.clone(), rois[:, 6]).numpy()
    corners = ku.boxes3d_to_corners3d(rois.numpy())
    out["corners3d"] = corners
    P2 = np.array([[707.05, 0., 604., 45.], [0., 707.05, 180., 0.2], [0., 0., 1., 0.003]], dtype=np.float32)
    calib = Calibration({"P2": P2, "R0": np.eye(3, dtype=np.float32), "Tr_velo2cam": np.zeros((3, 4), np.float32)})
    ib, ic = calib.corners3d_to_img_boxes(corners)
    out["img_boxes"], out["img_corners"] = ib, ic
    np.savez_compressed(os.path.join(HERE, "g7_glue_ref.npz"), **out)
    print("g7 done")


def g8(intensity=False):
    """the reference PointRCNN (tiny shapes) run here: inputs, weights and every output of one joint RPN+RCNN pass + the final stage
    of eval_rcnn.py.  intensity: cfg.RPN.USE_INTENSITY = True, pts_input (B, N, 4) = xyz | intensity - 0.5 (kitti_rcnn_dataset.py:321-338)
    -> g8i_e2e_tiny_intensity_ref.npz"""
    import copy
    over = copy.deepcopy(TINY)
    if intensity:
        over["RPN"]["USE_INTENSITY"] = True
    model, cfg = H.reference_model(over)
    torch.manual_seed(9 if intensity else 8)
    # random-init leaves the heads near zero; spread them so that decisions are not degenerate
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "reg_layer" in name or "cls_layer" in name:
                if p.dim() > 1:
                    p.copy_(torch.randn_like(p) * 0.3)
                else:
                    p.copy_(torch.randn_like(p) * 0.5)
        model.rpn.rpn_cls_layer[-1].conv.bias.zero_()     # ~half of the points become foreground
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.running_mean.copy_(torch.randn_like(m.running_mean) * 0.1)
                m.running_var.copy_(torch.rand_like(m.running_var) + 0.5)
    pts = torch.from_numpy(helpers.scenes(2, 2048, seed0=80))
    if intensity:
        refl = np.random.default_rng(81).random((2, 2048, 1)).astype(np.float32) - np.float32(0.5)
        pts = torch.cat([pts, torch.from_numpy(refl)], dim=2)
    with torch.no_grad():
        ret = model({"pts_input": pts})
        # centre the segmentation threshold (sigmoid > 0.3 <=> raw > -0.8473) on the median score so
        # that roughly half of the points are foreground, then run the pass that is recorded
        model.rpn.rpn_cls_layer[-1].conv.bias += (-0.8473 - ret["rpn_cls"].median())
        ret = model({"pts_input": pts})
    from lib.utils.bbox_transform import decode_bbox_target
    import lib.utils.kitti_utils as ku
    import lib.utils.iou3d.iou3d_utils as iu
    B = 2
    anchor = torch.from_numpy(cfg.CLS_MEAN_SIZE[0])
    rcnn_cls = ret["rcnn_cls"].view(B, -1, ret["rcnn_cls"].shape[1])
    rcnn_reg = ret["rcnn_reg"].view(B, -1, ret["rcnn_reg"].shape[1])
    pred = decode_bbox_target(ret["rois"].view(-1, 7), rcnn_reg.view(-1, rcnn_reg.shape[-1]), anchor_size=anchor,
                              loc_scope=cfg.RCNN.LOC_SCOPE, loc_bin_size=cfg.RCNN.LOC_BIN_SIZE,
                              num_head_bin=cfg.RCNN.NUM_HEAD_BIN, get_xz_fine=True,
                              get_y_by_bin=cfg.RCNN.LOC_Y_BY_BIN, loc_y_scope=cfg.RCNN.LOC_Y_SCOPE,
                              loc_y_bin_size=cfg.RCNN.LOC_Y_BIN_SIZE, get_ry_fine=True).view(B, -1, 7)
    norm = torch.sigmoid(rcnn_cls)
    inds = norm > cfg.RCNN.SCORE_THRESH
    M = pred.shape[1]
    final_boxes = np.zeros((B, M, 7), np.float32); final_scores = np.zeros((B, M), np.float32)
    final_num = np.zeros((B,), np.int32)
    for k in range(B):
        cur = inds[k].view(-1)
        if cur.sum() == 0:
            continue
        sel_boxes, sel_raw = pred[k, cur], rcnn_cls[k, cur]
        keep = iu.nms_gpu(ku.boxes3d_to_bev_torch(sel_boxes), sel_raw.view(-1), cfg.RCNN.NMS_THRESH).view(-1)
        n = len(keep)
        final_boxes[k, :n] = sel_boxes[keep].numpy(); final_scores[k, :n] = sel_raw[keep].view(-1).numpy()
        final_num[k] = n
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    np.savez_compressed(os.path.join(HERE, "g8i_e2e_tiny_intensity_ref.npz" if intensity else "g8_e2e_tiny_ref.npz"), pts=pts.numpy(),
                        rois=ret["rois"].numpy(), roi_scores_raw=ret["roi_scores_raw"].numpy(),
                        rpn_cls=ret["rpn_cls"].numpy(), rcnn_cls=ret["rcnn_cls"].numpy(), rcnn_reg=ret["rcnn_reg"].numpy(),
                        seg_result=ret["seg_result"].numpy(), final_boxes=final_boxes, final_scores=final_scores,
                        final_num=final_num, state_keys=np.array(list(sd.keys())),
                        **{"w/" + k: v for k, v in sd.items()})
    if intensity:
        cfg.RPN.USE_INTENSITY = False                     # (the reference's cfg is a module global: leave it as found)
    print("g8i:" if intensity else "g8:", "params", sum(v.size for v in sd.values()), "final_num", final_num.tolist(),
          "seg fg", int(ret["seg_result"].sum()), "nonzero rois", int((ret["rois"].abs().sum(-1) > 0).sum()))


FULL_SEED = 1204            # g12: weights (helpers.seeded_state_dict) and scenes


def full_scenes(kind, seed0):
    """g12's input batches (N = 16384): kind "u" = SURVEY 8d's uniform scene, "l" = LiDAR-shaped sweeps (synth.lidar_scene), B = 2;
    kind "p" (round 5, the product runner's launch shape): TWO batches of B = 8 -- eight uniform scenes, then eight LiDAR-shaped
    sweeps -- i.e. one pair of the graphed runner.  -> list of (B, 16384, 3) arrays"""
    S = importlib.import_module("3d_adapt_auto_driving_amd.synth")
    if kind == "p":
        return [np.stack([S.scene(seed0 + i, 16384) for i in range(8)], 0), np.stack([S.lidar_scene(seed0 + 8 + i, 16384) for i in range(8)], 0)]
    if kind == "d":       # g13: tools/cfgs/double.yaml:39 -- NUM_POINTS 32768, everything else default.yaml's; B = 1
        return [np.stack([S.scene(seed0, 32768)], 0)]
    return [np.stack([(S.scene if kind == "u" else S.lidar_scene)(seed0 + i, 16384) for i in range(2)], 0)]


def g12(kind):
    """BASELINE configs[2] shapes (cfgs/default.yaml, N = 16384, 100 RoIs x 512 points): B = 2 once on uniform scenes
    (g12u_e2e_full_ref.npz) and once on LiDAR-shaped ones (g12l_...), and -- round 5, VERDICT r4 task 3 -- at configs[2]'s LITERAL
    batch, two forward passes of B = 8 (g12p_...: outputs only, RPN tensors subsampled): the REFERENCE PointRCNN (point_rcnn.py:26-70,
    rcnn_net.py:127-185, proposal_layer.py:15-119) run here under the shims with seeded weights (helpers.seeded_state_dict:
    the 3.9 M parameters regenerate from the seed; the fixture holds a checksum, the one calibrated bias and OUTPUTS only) +
    the final stage of eval_rcnn.py:516-530,611-629.  Intermediate tensors recorded through forward hooks on the reference's
    modules (for localising a divergence, VERDICT r3 task 1): the RCNN SA levels' sampled centres and per-RoI cloud sums."""
    import time
    model, cfg = H.reference_model()
    sd, checksum = helpers.seeded_state_dict(model.state_dict(), FULL_SEED)
    model.load_state_dict(sd)
    hooks, cap = [], {}
    for i, m in enumerate(model.rcnn_net.SA_modules):
        hooks.append(m.register_forward_hook(lambda mod, inp, out, i=i: cap.setdefault("sa%d" % i, []).append((inp[0].clone(), out[0].clone() if out[0] is not None else None))))
    t0 = time.time()
    seed0 = {"p": FULL_SEED + 100, "d": FULL_SEED + 200}.get(kind, FULL_SEED)
    batches = [torch.from_numpy(b) for b in full_scenes(kind, seed0)]
    with torch.no_grad():
        ret = model({"pts_input": batches[0]})
        # centre the segmentation threshold (sigmoid > 0.3 <=> raw > -0.8473) on the 70th percentile of the scores: ~30 % foreground
        shift = float(-0.8473 - torch.quantile(ret["rpn_cls"].view(-1), 0.7))
        model.rpn.rpn_cls_layer[-1].conv.bias += shift
        cls_bias = model.rpn.rpn_cls_layer[-1].conv.bias.detach().clone().numpy()
        cap.clear()
        rets = [model({"pts_input": pts}) for pts in batches]
    ret = {k: torch.cat([r[k] for r in rets], 0) for k in ("rois", "roi_scores_raw", "rpn_cls", "rpn_reg", "backbone_features", "seg_result", "rcnn_cls", "rcnn_reg")}
    # NOTE for the tests: with 100 RoIs per scene some neighbours in the score order are closer than f32 rounding of the MLPs
    # (printed below); their ORDER is not defined by the reference either (cuDNN there, MKL here), so tests compare RoI rows up to
    # swaps inside groups of RoIs whose reference scores agree within the tolerance.
    print("g12%s: min gap between neighbouring RoI scores %.3g" % (kind, np.abs(np.diff(ret["roi_scores_raw"].numpy(), axis=1)).min()))
    print("g12%s: reference passes in %.1f s" % (kind, time.time() - t0))
    for h in hooks:
        h.remove()
    from lib.utils.bbox_transform import decode_bbox_target
    import lib.utils.kitti_utils as ku
    import lib.utils.iou3d.iou3d_utils as iu
    B = ret["rois"].shape[0]
    anchor = torch.from_numpy(cfg.CLS_MEAN_SIZE[0])
    rcnn_cls = ret["rcnn_cls"].view(B, -1, ret["rcnn_cls"].shape[1])
    rcnn_reg = ret["rcnn_reg"].view(B, -1, ret["rcnn_reg"].shape[1])
    pred = decode_bbox_target(ret["rois"].view(-1, 7), rcnn_reg.view(-1, rcnn_reg.shape[-1]), anchor_size=anchor,
                              loc_scope=cfg.RCNN.LOC_SCOPE, loc_bin_size=cfg.RCNN.LOC_BIN_SIZE,
                              num_head_bin=cfg.RCNN.NUM_HEAD_BIN, get_xz_fine=True,
                              get_y_by_bin=cfg.RCNN.LOC_Y_BY_BIN, loc_y_scope=cfg.RCNN.LOC_Y_SCOPE,
                              loc_y_bin_size=cfg.RCNN.LOC_Y_BIN_SIZE, get_ry_fine=True).view(B, -1, 7)
    inds = torch.sigmoid(rcnn_cls) > cfg.RCNN.SCORE_THRESH
    M = pred.shape[1]
    final_boxes = np.zeros((B, M, 7), np.float32); final_scores = np.zeros((B, M), np.float32)
    final_num = np.zeros((B,), np.int32)
    for k in range(B):
        cur = inds[k].view(-1)
        if cur.sum() == 0:
            continue
        sel_boxes, sel_raw = pred[k, cur], rcnn_cls[k, cur]
        keep = iu.nms_gpu(ku.boxes3d_to_bev_torch(sel_boxes), sel_raw.view(-1), cfg.RCNN.NMS_THRESH).view(-1)
        n = len(keep)
        final_boxes[k, :n] = sel_boxes[keep].numpy(); final_scores[k, :n] = sel_raw[keep].view(-1).numpy()
        final_num[k] = n
    pooled_xyz = torch.cat([c[0] for c in cap["sa0"]], 0)            # (100 B, 512, 3) canonical RoI clouds
    common = dict(seed=np.int64(FULL_SEED), scene_seed0=np.int64(seed0), weights_checksum=np.float64(checksum),
                  rpn_cls_bias=cls_bias, rois=ret["rois"].numpy(), roi_scores_raw=ret["roi_scores_raw"].numpy(),
                  seg_result=np.packbits(ret["seg_result"].numpy().astype(np.uint8), axis=1),
                  rcnn_cls=ret["rcnn_cls"].numpy(), rcnn_reg=ret["rcnn_reg"].numpy(), decoded=pred.numpy(),
                  pooled_xyz_sum=pooled_xyz.double().sum(1).numpy(),
                  final_boxes=final_boxes, final_scores=final_scores, final_num=final_num)
    if kind == "p":
        # 16 scenes: the RPN tensors subsampled harder (every 16th score, every 256th regression row); the points whose score lies
        # within the tests' tolerance of the segmentation threshold -- where the flag is not compared -- as a bit mask instead
        cls = ret["rpn_cls"].numpy()[..., 0].astype(np.float64)
        undecided = np.abs(cls - np.log(0.3 / 0.7)) <= helpers.TOL * np.maximum(1.0, np.abs(cls))
        common.update(rpn_cls=ret["rpn_cls"].numpy()[:, ::16, 0], rpn_cls_stride=np.int64(16),
                      rpn_reg_sub=ret["rpn_reg"].numpy()[:, ::256], rpn_reg_stride=np.int64(256),
                      seg_undecided=np.packbits(undecided, axis=1), batch=np.int64(8))
    else:
        sub = slice(0, ret["rpn_cls"].shape[1], 64)
        common.update(rpn_cls=ret["rpn_cls"].numpy()[..., 0], rpn_reg_sub=ret["rpn_reg"].numpy()[:, sub],
                      backbone_features_sub=ret["backbone_features"].numpy()[:, :, sub],
                      sa1_new_xyz=torch.cat([c[1] for c in cap["sa0"]], 0).numpy(), sa2_new_xyz=torch.cat([c[1] for c in cap["sa1"]], 0).numpy())
    np.savez_compressed(os.path.join(HERE, "g13_e2e_double_ref.npz" if kind == "d" else "g12%s_e2e_full_ref.npz" % kind), **common)
    print("g12%s: checksum %.6f, final_num %s, seg fg %s, nonzero rois %s, rcnn score range %.3f..%.3f" % (
        kind, checksum, final_num.tolist(), ret["seg_result"].sum(1).tolist(), (ret["rois"].abs().sum(-1) > 0).sum(1).tolist(),
        float(rcnn_cls.min()), float(rcnn_cls.max())))


KITTI_SEED = 1100           # g11: fake KITTI tree (helpers.write_fake_kitti_tree) and writer boxes


def g11():
    """Reference-EXECUTED pins of the host input stage and of the result writer (VERDICT r3 task 8): on a fake KITTI tree
    (helpers.write_fake_kitti_tree: five scenes, one per branch of the sampler) the reference's own
    KittiRCNNDataset.get_rpn_sample (kitti_rcnn_dataset.py:249-342: Calibration.lidar_to_rect / rect_to_img, get_valid_flag :201,
    the near / far sampler on the legacy ``np.random`` stream) in TEST mode, and the reference's save_kitti_format
    (tools/eval_rcnn.py:76-101) with its Calibration (calibration.py:107-125).  The tree regenerates from the seed; the fixture
    holds the reference's OUTPUTS: per scene the valid flags, the chosen rows (recovered from pts_rect: every valid row is
    unique), pts_input, and the result text."""
    import logging
    import tempfile
    import types
    H.install()
    if "tensorboardX" not in sys.modules:            # tools/eval_rcnn.py imports it for the checkpoint-polling loop (unused here)
        try:
            import tensorboardX  # noqa: F401
        except ImportError:
            tb = types.ModuleType("tensorboardX"); tb.SummaryWriter = None
            sys.modules["tensorboardX"] = tb
    argv, sys.argv = sys.argv, ["eval_rcnn.py", "--eval_mode", "rcnn"]     # the reference parses its command line at import
    sys.path.append(os.path.join(H.REF, "tools"))
    try:
        ref_eval = importlib.import_module("eval_rcnn")
    finally:
        sys.argv = argv
    assert ref_eval.__file__.startswith("/root/reference/")
    from lib.config import cfg, cfg_from_file
    cfg_from_file(os.path.join(H.REF, "tools", "cfgs", "default.yaml"))
    cfg.RCNN.ENABLED = True; cfg.RPN.ENABLED = cfg.RPN.FIXED = True
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    from lib.utils.calibration import Calibration
    out = {"seed": np.int64(KITTI_SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        ids = helpers.write_fake_kitti_tree(tmp, KITTI_SEED)
        ds = KittiRCNNDataset(root_dir=tmp, npoints=cfg.RPN.NUM_POINTS, split="val", mode="TEST", random_select=True,
                              classes=cfg.CLASSES, logger=logging.getLogger("g11"), npoints_faraway=4000)
        out["ids"] = np.array(ids, np.int64)
        branches = []
        for pos, sid in enumerate(ids):
            calib = ds.get_calib(sid)
            lidar = ds.get_lidar(sid)
            shape = ds.get_image_shape(sid)
            rect = calib.lidar_to_rect(lidar[:, 0:3])
            img, depth = calib.rect_to_img(rect)
            flag = ds.get_valid_flag(rect, img, depth, shape)
            for variant, seed_fn in (("", lambda: np.random.seed(1024 + sid)),):
                seed_fn()
                sample = ds.get_rpn_sample(pos)
            pin = sample["pts_input"]
            assert sample["sample_id"] == sid and pin.shape == (cfg.RPN.NUM_POINTS, 3) and pin.dtype == np.float32
            valid_rows = rect[flag][:, 0:3]
            # recover the chosen row of every output point (rows of a sweep are unique)
            order = np.lexsort(valid_rows.T[::-1])
            sorted_rows = valid_rows[order]
            keyv = np.ascontiguousarray(sorted_rows).view([("", np.float32)] * 3).ravel()
            keyp = np.ascontiguousarray(pin).view([("", np.float32)] * 3).ravel()
            where = np.searchsorted(keyv, keyp)
            choice = order[where]
            assert np.array_equal(valid_rows[choice], pin)
            nv, nnear = int(flag.sum()), int((valid_rows[:, 2] < 40.0).sum())
            branches.append((helpers.KITTI_CASES[pos], nv, nnear, nv - nnear))
            out["lidar_sum_%d" % sid] = np.float64(lidar.astype(np.float64).sum())
            out["shape_%d" % sid] = np.array(shape[:2], np.int64)
            out["valid_%d" % sid] = np.packbits(flag)
            out["n_raw_%d" % sid] = np.int64(len(lidar))
            out["choice_%d" % sid] = choice.astype(np.int32)
            out["rect_sub_%d" % sid] = rect[::97].astype(np.float32)
            out["img_sub_%d" % sid] = img[::97].astype(np.float32)
            out["depth_sub_%d" % sid] = depth[::97].astype(np.float32)
            out["pts_input_sum_%d" % sid] = np.float64(pin.astype(np.float64).sum())
        # the sequential stream of a single-process loader: np.random.seed(1024) as tools/eval_rcnn.py:26 sets it, scenes in order
        np.random.seed(1024)
        seq = [ds.get_rpn_sample(pos)["pts_input"] for pos in range(len(ids))]
        out["seq_pts_input_sum"] = np.array([p.astype(np.float64).sum() for p in seq])
        out["seq_first_rows"] = np.stack([p[:8] for p in seq], 0)
        print("g11 sampler branches (case, valid, near, far):", branches)
        b = {c: (nv, nn, nf) for c, nv, nn, nf in branches}
        assert b["normal"][0] > 16384 and b["normal"][2] <= 4000 and b["normal"][1] >= 16384 - b["normal"][2]
        assert b["many_far"][2] > 4000 and b["many_far"][1] >= 12384
        assert 8192 < b["pad_without_replacement"][0] < 16384 and b["pad_with_replacement"][0] < 8192
        assert b["near_short"][0] > 16384 and b["near_short"][1] < 16384 - min(4000, b["near_short"][2])
        # the writer
        boxes, scores = helpers.writer_boxes(KITTI_SEED + 50)
        texts = []
        for sid in ids[:2]:
            calib = Calibration(os.path.join(tmp, "KITTI", "object", "training", "calib", "%06d.txt" % sid))
            shape = ds.get_image_shape(sid)
            os.makedirs(os.path.join(tmp, "res"), exist_ok=True)
            ref_eval.save_kitti_format(sid, calib, boxes.copy(), os.path.join(tmp, "res"), scores.copy(), shape)
            texts.append(open(os.path.join(tmp, "res", "%06d.txt" % sid)).read())
        ref_eval.save_kitti_format(999, calib, boxes[:0].copy(), os.path.join(tmp, "res"), scores[:0].copy(), shape)
        assert open(os.path.join(tmp, "res", "000999.txt")).read() == ""
        out["writer_text"] = np.array(texts)
        out["writer_lines"] = np.array([t.count("\n") for t in texts])
        print("g11 writer: %d boxes -> %s lines" % (len(boxes), out["writer_lines"].tolist()))
        assert 0 < out["writer_lines"].min() < len(boxes)
    np.savez_compressed(os.path.join(HERE, "g11_input_writer_ref.npz"), **out)


def synth_label_sets(n_img=60, seed=2024):
    """Synthetic KITTI label lines and detection lines for the AP-evaluator fixture: cars over 3..68 m with
    all occlusion / truncation levels, Vans, Pedestrians, DontCare regions; detections = jittered ground
    truth (various IoU), duplicates, false positives, other-class detections, one image without detections
    and one without labels."""
    from importlib import import_module
    S = import_module("3d_adapt_auto_driving_amd.synth")
    K = import_module("3d_adapt_auto_driving_amd.kitti_utils")
    calib = S.SyntheticCalib()
    rng = np.random.default_rng(seed)

    def line(name, trunc, occ, box, score=None):
        corners = K.boxes3d_to_corners3d(box[None].astype(np.float32))
        img, _ = calib.corners3d_to_img_boxes(corners)
        x1, y1, x2, y2 = np.clip(img[0], [0, 0, 0, 0], [1241, 374, 1241, 374])
        beta = np.arctan2(box[2], box[0])
        alpha = -np.sign(beta) * np.pi / 2 + beta + box[6]
        s = "%s %.2f %d %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" % (
            name, trunc, occ, alpha, x1, y1, x2, y2, box[3], box[4], box[5], box[0], box[1], box[2], box[6])
        return s if score is None else s + " %.4f" % score

    gts, dts = [], []
    for i in range(n_img):
        g, d = [], []
        n_obj = 0 if i == 5 else int(rng.integers(2, 9))
        for _ in range(n_obj):
            box = np.array([rng.uniform(-15, 15), rng.uniform(1.4, 1.8), rng.uniform(3, 68), rng.normal(1.55, 0.1),
                            rng.normal(1.63, 0.1), rng.normal(3.9, 0.4), rng.uniform(-np.pi, np.pi)])
            name = rng.choice(["Car", "Car", "Car", "Car", "Van", "Pedestrian", "Cyclist"])
            if name == "Pedestrian":
                box[3:6] = [1.75, 0.6, 0.8]
            g.append(line(name, float(rng.choice([0, 0, 0.1, 0.2, 0.4, 0.6])), int(rng.choice([0, 0, 1, 2, 3])), box))
            if i != 7 and rng.random() < 0.85:                       # detected, with a random amount of jitter
                jit = box.copy()
                scale = float(rng.choice([0.02, 0.1, 0.3, 0.8]))
                jit[[0, 2]] += rng.normal(0, scale, 2)
                jit[1] += rng.normal(0, 0.1 * scale)
                jit[3:6] *= 1 + rng.normal(0, 0.05, 3) * scale
                jit[6] += rng.normal(0, 0.3 * scale)
                d.append(line("Car" if name != "Pedestrian" else "Pedestrian", 0, 0, jit, float(rng.uniform(-2, 6))))
                if rng.random() < 0.15:                               # duplicate detection of the same object
                    jit2 = jit.copy(); jit2[[0, 2]] += rng.normal(0, 0.1, 2)
                    d.append(line("Car", 0, 0, jit2, float(rng.uniform(-2, 6))))
        for _ in range(int(rng.integers(0, 3))):                      # DontCare regions (2D only)
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 300)
            g.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10" %
                     (x1, y1, x1 + rng.uniform(20, 120), y1 + rng.uniform(10, 60)))
        if i != 7:
            for _ in range(int(rng.integers(0, 5))):                  # false positives
                box = np.array([rng.uniform(-20, 20), rng.uniform(1.4, 1.8), rng.uniform(3, 75), 1.5, 1.6, 3.9,
                                rng.uniform(-np.pi, np.pi)])
                d.append(line("Car", 0, 0, box, float(rng.uniform(-3, 3))))
        gts.append(g)
        dts.append(d)
    return gts, dts


def g10():
    """Reference AP evaluator on the synthetic label sets (see the header for the two import shims)."""
    import tempfile
    import types
    import numba_shim as NS
    riou, cu = NS.import_reference_rotate_iou()      # the reference's own K18 (numba + numba.cuda interpreted)
    calls = {"n": 0, "pairs": 0, "undefined": 0}
    _ref_eval = riou.rotate_iou_gpu_eval

    def counted(boxes, query_boxes, criterion=-1, device_id=0):
        out = _ref_eval(boxes, query_boxes, criterion, device_id)
        calls["n"] += 1
        calls["pairs"] += out.size
        if out.size and cu.last_undefined is not None:
            calls["undefined"] += int(cu.last_undefined.sum())
        return out
    riou.rotate_iou_gpu_eval = counted
    if "skimage" not in sys.modules:                  # kitti_common imports skimage.io for image sizes only (unused here)
        sk = types.ModuleType("skimage")
        sk.io = types.ModuleType("skimage.io")
        sys.modules["skimage"], sys.modules["skimage.io"] = sk, sk.io
    sys.path.append("/root/reference/evaluate")
    eval2 = importlib.import_module("eval2")
    kc = importlib.import_module("kitti_common")
    gts, dts = synth_label_sets()
    with tempfile.TemporaryDirectory() as tmp:
        for sub, sets in (("gt", gts), ("dt", dts)):
            os.makedirs(os.path.join(tmp, sub))
            for i, lines in enumerate(sets):
                with open(os.path.join(tmp, sub, "%06d.txt" % i), "w") as f:
                    f.write("\n".join(lines))
        ids = list(range(len(gts)))
        gt_annos = kc.get_label_annos(os.path.join(tmp, "gt"), ids)
        dt_annos = kc.get_label_annos(os.path.join(tmp, "dt"), ids)
    out = {"gt_lines": np.array(["\n".join(l) for l in gts]), "dt_lines": np.array(["\n".join(l) for l in dts])}
    text, ret = eval2.get_official_eval_result(gt_annos, dt_annos, 0, "kitti")
    out["result_text"] = np.array(text)
    for k in ("Car_3d_easy", "Car_3d_moderate", "Car_3d_hard", "Car_bev_easy", "Car_bev_moderate", "Car_bev_hard",
              "Car_image_easy", "Car_image_moderate", "Car_image_hard"):
        out[k] = np.float64(ret[k])
    min_overlaps = np.stack([np.array([[0.7, 0.5, 0.5]] * 3), np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])], 0)
    for metric in (0, 1, 2):
        r = eval2.eval_class(gt_annos, dt_annos, [0, 1], "kitti", [0, 1, 2, 3, 4, 5], metric, min_overlaps[:, :, :2],
                             compute_aos=(metric == 0))
        out["precision_m%d" % metric] = r["precision"]
        out["recall_m%d" % metric] = r["recall"]
        if metric == 0:
            out["aos_m0"] = r["orientation"]
    # one image's raw matching statistics for the C-ABI entry, both passes
    ov = eval2.calculate_iou_partly(dt_annos, gt_annos, 2, 50)[0]
    stats = []
    for i in range(len(gt_annos)):
        nv, ig, idt, dc = eval2.clean_data(gt_annos[i], dt_annos[i], 0, "kitti", 1)
        gtd = np.concatenate([gt_annos[i]["bbox"], gt_annos[i]["alpha"][..., None]], 1)
        dtd = np.concatenate([dt_annos[i]["bbox"], dt_annos[i]["alpha"][..., None], dt_annos[i]["score"][..., None]], 1)
        dcb = np.stack(dc, 0) if len(dc) else np.zeros((0, 4))
        for fp_pass, th in ((False, 0.0), (True, 0.5)):
            tp, fp, fn, sim, thr = eval2.compute_statistics_jit(ov[i], gtd, dtd, np.array(ig, np.int64), np.array(idt, np.int64),
                                                                dcb, 2, 0.5, th, fp_pass, False)
            stats.append([i, int(fp_pass), tp, fp, fn, len(thr), float(np.sum(thr))])
    out["image_stats_3d"] = np.array(stats, dtype=np.float64)
    assert sys.modules["rotate_iou"].__file__.startswith("/root/reference/") and eval2.rotate_iou_gpu_eval is counted
    assert calls["n"] > 0 and calls["undefined"] == 0, calls
    out["riou_source"] = np.array("reference evaluate/rotate_iou.py via tests/golden/numba_shim.py: %(n)d calls, %(pairs)d pairs" % calls)
    np.savez_compressed(os.path.join(HERE, "g10_ap_eval_ref.npz"), **out)
    print("g10:", text.split("\n")[0], "|", text.split("\n")[3], "|", calls)


def g9_boxes():
    """256 + 256 centre-format boxes [cx, cy, w, h, angle] with the pair classes VERDICT r2 asked for."""
    rng = np.random.default_rng(909)
    n = 256

    def rnd(m, spread):
        return np.stack([rng.uniform(-spread, spread, m), rng.uniform(-spread, spread, m), rng.uniform(1.4, 2.2, m),
                         rng.uniform(3.0, 5.0, m), rng.uniform(-np.pi, np.pi, m)], 1)
    a, q = rnd(n, 9.0), rnd(n, 9.0)
    q[0:16] = a[0:16]                                                   # identical (diagonal pairs)
    q[16:24] = a[16:24]; q[16:24, 4] += np.pi                           # identical up to a half turn
    a[24:32, 4] = 0; q[24:32] = a[24:32]; q[24:32, 0] += a[24:32, 2]    # axis-aligned, touching along an edge
    a[32:40, 4] = 0; q[32:40] = a[32:40]; q[32:40, 0] += a[32:40, 2]; q[32:40, 1] += a[32:40, 3]   # touching at a corner
    q[40:56] = a[40:56]; q[40:56, 2:4] *= 0.4                           # nested, same angle
    q[56:72] = a[56:72]; q[56:72, 2:4] *= 0.3; q[56:72, 4] = rng.uniform(-np.pi, np.pi, 16)       # nested, other angle
    a[72:88, 2] = 0.05; q[72:88, :2] = a[72:88, :2]                     # thin slivers crossing a box
    q[88:96, 2] = 0.02; q[88:96, 3] = 0.02                              # tiny boxes
    a[96:112] = rnd(16, 9.0); a[96:112, :2] += 1000.0                   # far apart from everything
    a[112:128, 4] = rng.choice([0, np.pi / 2, -np.pi / 2, np.pi], 16)   # axis-aligned angles among rotated ones
    q[112:128, 4] = rng.choice([0, np.pi / 2, -np.pi / 2, np.pi], 16)
    q[128:136] = a[128:136]; q[128:136, :2] += rng.normal(0, 1e-3, (8, 2))   # nearly identical
    a[136:144, 2:4] = [[30.0, 30.0]]                                     # huge boxes that contain many others
    a[144:160] = rnd(16, 2.0); q[144:160] = rnd(16, 2.0)                # a dense clump: every pair overlaps
    return a.astype(np.float32), q.astype(np.float32)


def _g9_rows(args):
    lo, hi = args
    import numba_shim as NS
    mod, cu = NS.import_reference_rotate_iou()
    a, q = g9_boxes()
    res = {}
    for crit in (-1, 0, 1, 2):
        res[crit] = NS.reference_rotate_iou_eval(mod, cu, a[lo:hi], q, crit)
    return lo, hi, res


def g9():
    """The reference's own rotate_iou.py on the interpreter of numba_shim.py (see the header)."""
    import multiprocessing as mp
    a, q = g9_boxes()
    n = a.shape[0]
    chunks = [(lo, min(lo + 16, n)) for lo in range(0, n, 16)]
    out = {"boxes": a, "query_boxes": q}
    iou = {c: np.zeros((n, q.shape[0]), np.float32) for c in (-1, 0, 1, 2)}
    und = np.zeros((n, q.shape[0]), bool)
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        for lo, hi, res in pool.imap_unordered(_g9_rows, chunks):
            for c in (-1, 0, 1, 2):
                iou[c][lo:hi] = res[c][0]
                und[lo:hi] |= res[c][1]
    for c in (-1, 0, 1, 2):
        out["iou_c%d" % c] = iou[c]
    out["undefined"] = und
    np.savez_compressed(os.path.join(HERE, "g9_rotate_iou_ref.npz"), **out)
    print("g9: pairs", und.size, "overlapping", int((iou[2] > 0).sum()), "undefined in the reference", int(und.sum()))


def g9l():
    """A second, independent sample for rotate_iou (tests/test_oracle.py::test_rotate_iou_live_reference_run_matches_oracle): 70 x 20
    random boxes (rng 77; 70 rows = two thread blocks, the second one ragged), criteria -1 and 1, the reference's own rotate_iou.py
    on the interpreter of numba_shim.py."""
    import numba_shim as NS
    mod, cu = NS.import_reference_rotate_iou()
    rng = np.random.default_rng(77)

    def cb(n):
        return np.stack([rng.uniform(-4, 4, n), rng.uniform(-4, 4, n), rng.uniform(1.4, 2.2, n), rng.uniform(3, 5, n),
                         rng.uniform(-np.pi, np.pi, n)], 1).astype(np.float32)
    a, q = cb(70), cb(20)
    out = {"boxes": a, "query_boxes": q}
    for crit in (-1, 1):
        out["iou_c%d" % crit], out["undefined_c%d" % crit] = NS.reference_rotate_iou_eval(mod, cu, a, q, crit)
    np.savez_compressed(os.path.join(HERE, "g9l_rotate_iou_sample_ref.npz"), **out)
    print("g9l: overlapping pairs", {c: int((out["iou_c%d" % c] > 0).sum()) for c in (-1, 1)})


def g14():
    """The reference's KittiRCNNDataset.filtrate_objects + kitti_utils.objs_to_boxes3d in EVAL and TRAIN mode on the label file of
    tests/test_host_logic.py::test_recall_gt_set_is_class_only_in_eval_like_the_reference (LABELS_GT, stored beside the boxes)."""
    import tempfile
    from test_host_logic import LABELS_GT
    H.install()
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    import lib.utils.kitti_utils as ku
    from lib.config import cfg as rcfg
    assert rcfg.PC_REDUCE_BY_RANGE
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "000001.txt")
        with open(path, "w") as f:
            f.write(LABELS_GT)
        objs = ku.get_objects_from_label(path)

    class Fake:
        classes = ("Background", "Car")
        check_pc_range = staticmethod(KittiRCNNDataset.check_pc_range)
    out = {"labels": np.array(LABELS_GT)}
    for mode in ("EVAL", "TRAIN"):
        Fake.mode = mode
        out["boxes3d_" + mode.lower()] = ku.objs_to_boxes3d(KittiRCNNDataset.filtrate_objects(Fake, objs)).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "g14_kitti_labels_ref.npz"), **out)
    print("g14: kept", {m: len(out["boxes3d_" + m]) for m in ("eval", "train")})


def g_ops():
    rng = np.random.default_rng(1)
    out = {}
    # G1 ball query: B=2,N=1024,M=256; empty ball, under-full ball, duplicate cloud
    xyz = helpers.scenes(2, 1024, seed0=100)
    xyz[1, 512:] = xyz[1, :512]                         # duplicate-point cloud
    sel = O.furthest_point_sample(xyz, 256).astype(np.int64)
    new = np.take_along_axis(xyz, sel[..., None].repeat(3, -1), 1)
    new[0, 0] = [500, 500, 500]
    out["bq_xyz"], out["bq_new"] = xyz, new
    for r in (0.1, 0.2, 0.4, 2.0):
        for ns in (16, 32, 64):
            out["bq_r%g_ns%d" % (r, ns)] = O.ball_query(r, ns, xyz, new)
    # G2 FPS incl. lattice + duplicates (tie rule) for several n
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    lat = g[rng.permutation(len(g))].astype(np.float32)
    for n, m in ((128, 32), (512, 128), (1000, 100), (1024, 256), (2048, 512)):
        cloud = lat[:n][None].copy()
        out["fps_lat_in_%d" % n] = cloud
        out["fps_lat_%d" % n] = O.furthest_point_sample(cloud, m)
        rnd = helpers.scenes(1, n, seed0=200 + n)
        out["fps_rnd_in_%d" % n] = rnd
        out["fps_rnd_%d" % n] = O.furthest_point_sample(rnd, m)
    # G3 three_nn with ties
    unk = helpers.scenes(1, 512, seed0=300)
    kn = unk[:, ::8].copy(); kn[0, 1] = kn[0, 0]
    d2, i3 = O.three_nn(unk, kn)
    out["nn_unknown"], out["nn_known"], out["nn_d2"], out["nn_idx"] = unk, kn, d2, i3
    # G6 NMS + overlap on 256 boxes
    bx = helpers.bev_boxes(rng, 256, spread=10.0)
    out["nms_boxes"] = bx
    out["nms_rot_keep"] = O.nms(bx, 0.1)
    out["nms_norm_keep"] = O.nms_normal(bx, 0.5)
    out["overlap"] = O.boxes_overlap_bev(bx[:64], bx[64:128])
    out["iou_bev"] = O.boxes_iou_bev(bx[:64], bx[64:128])
    # G9 rotate_iou
    cb = np.stack([rng.uniform(-6, 6, 80), rng.uniform(-6, 6, 80), rng.uniform(1.4, 2, 80), rng.uniform(3, 5, 80),
                   rng.uniform(-np.pi, np.pi, 80)], 1).astype(np.float32)
    out["riou_boxes"] = cb
    for crit in (-1, 0, 1, 2):
        out["riou_c%d" % crit] = O.rotate_iou_eval(cb[:50], cb[50:], crit)
    np.savez_compressed(os.path.join(HERE, "g_ops_oracle.npz"), **out)
    print("g_ops done")


if __name__ == "__main__":
    assert H.available(), "/root/reference is not mounted: fixtures can only be regenerated in the build container"
    todo = sys.argv[1:] or ["g5", "g7", "g_ops", "g8", "g8i", "g9", "g9l", "g10", "g11", "g12u", "g12l", "g12p", "g13", "g14"]      # e.g. ``make_golden.py g9 g10``
    for name in todo:
        {"g5": g5, "g7": g7, "g_ops": g_ops, "g8": g8, "g8i": lambda: g8(intensity=True), "g9": g9, "g9l": g9l, "g10": g10, "g11": g11, "g12u": lambda: g12("u"), "g12l": lambda: g12("l"), "g12p": lambda: g12("p"), "g13": lambda: g12("d"), "g14": g14}[name]()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)) // 1024, "KiB")
