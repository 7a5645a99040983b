"""Generates tests/golden/g16_rpn_labels_ref.npz: RPN labels as the REFERENCE's own
KittiRCNNDataset.generate_rpn_training_labels (lib/datasets/kitti_rcnn_dataset.py:385-414: kitti_utils.boxes3d_to_corners3d,
enlarge_box3d, in_hull = scipy Delaunay.find_simplex) computes them.

RUN IN THE BUILD CONTAINER ONLY (imports the reference through ref_harness, read-only; needs scipy):
    python tests/golden/make_golden_rpn_eval.py
The fixture holds data only.

Contents (per case c):
  lidar      LiDAR-shaped scenes regenerated from their seeds (synth.lidar_scene_with_labels(seed, 16384, n_cars)): seeds, n_cars;
             scene 2 has no car.  Extra Van / Pedestrian / DontCare objects are not boxes of the label pass (EVAL keeps Car only).
  crafted    hand-made boxes (ry = 0, +-pi, pi/2, overlapping boxes where the order decides, a zero-size box) and points exactly on
             faces, edges and corners, in the ignore band, inside and outside; pts are stored.
  many       a scene with 300 boxes over a LiDAR cloud.
  <c>_gt_<s> (g, 7) f32 boxes, <c>_pts_<s> (crafted / many: (n, 3) f32 points), <c>_cls_<s> int8 labels,
  <c>_regidx_<s> / <c>_reg_<s>  the rows of the regression labels that are not all zero and their values (f32),
  corners_in / corners_ref      boxes and the reference's boxes3d_to_corners3d of them (pins the f32 matmul order).
  a_*        part (a): the reference's eval_one_epoch_rpn on tests/rpn_tree.py's labelled tree (see part_a): its ret_dict, the RoIs and
             scores of the proposal layer, per scene the seg_result columns (labels, predictions, xyz sums), the detection text, and
             every features/ file's dtype, shape and rows ::97.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402

LIDAR_SEEDS = (1601, 1602, 1603, 1604)
LIDAR_CARS = (10, 14, 0, 6)


def crafted():
    f32 = np.float32
    boxes = np.array([
        [0.0, 1.5, 10.0, 1.5, 1.6, 4.0, 0.0],            # axis-aligned
        [5.0, 1.6, 12.0, 1.5, 1.6, 4.0, np.pi],          # ry = +pi
        [-5.0, 1.6, 12.0, 1.5, 1.6, 4.0, -np.pi],        # ry = -pi
        [0.0, 1.6, 20.0, 1.4, 1.8, 3.6, np.pi / 2],      # ry = pi/2
        [0.5, 1.5, 11.0, 1.5, 1.6, 4.0, 0.3],            # overlaps box 0: later box overrides
        [8.0, 1.0, 25.0, 0.0, 0.0, 0.0, 0.0],            # zero size: an empty hull, a 0.4 m ignore cube
        [-8.0, 1.7, 30.0, 1.5, 1.7, 4.2, 1.1],
        [-8.3, 1.7, 30.5, 1.5, 1.7, 4.2, -2.0],          # overlaps the previous one
    ], dtype=f32)
    rng = np.random.default_rng(16)
    pts = []
    for b in boxes:
        x, y, z, h, w, l, ry = b
        # local grid incl. faces, edges, corners (exact in f32 for ry = 0 / pi), band points just outside
        for fx in (-0.5, -0.25, 0.0, 0.25, 0.5, 0.5 + 0.1 / max(l, 1e-3), -0.5 - 0.3 / max(l, 1e-3)):
            for fy in (0.0, -0.5, -1.0, 0.05, -1.1):
                for fz in (-0.5, 0.0, 0.5, 0.5 + 0.1 / max(w, 1e-3)):
                    lx, ly, lz = f32(fx) * l, f32(fy) * h, f32(fz) * w
                    c, s = np.cos(f32(ry)), np.sin(f32(ry))
                    pts.append([x + lx * c + lz * s, y + ly, z - lx * s + lz * c])
        pts.extend((np.array([x, y, z]) + rng.uniform(-3, 3, (60, 3)) * [1, 0.5, 1]).tolist())
    pts = np.array(pts, dtype=f32)
    # the reference's own corners: points exactly on corners of the (rotated) boxes
    from lib.utils import kitti_utils as K
    cor = K.boxes3d_to_corners3d(boxes)
    big = K.boxes3d_to_corners3d(K.enlarge_box3d(boxes, extra_width=0.2))
    pts = np.concatenate([pts, cor.reshape(-1, 3), big.reshape(-1, 3), ((cor[:, 0] + cor[:, 1]) / 2).astype(f32),
                          ((cor[:, 0] + cor[:, 5]) / 2).astype(f32)]).astype(f32)
    return boxes, pts


A_SEED = 1612             # seeded full-size RPN weights (helpers.seeded_state_dict)


def part_a(out):
    """(a) the reference's own eval_one_epoch_rpn (--eval_mode rpn --save_result --save_rpn_feature, batch size 2, one process) on
    the labelled fake tree of tests/rpn_tree.py, with seeded weights.  The loader's sampler is seeded per scene
    (np.random.seed(1024 + sample id) in front of every sample), the stream kitti_io.KittiSource.load uses (pinned by g11)."""
    import importlib
    import logging
    import tempfile
    import types
    import torch
    import helpers
    import rpn_tree
    if "tensorboardX" not in sys.modules:
        tb = types.ModuleType("tensorboardX"); tb.SummaryWriter = None
        sys.modules["tensorboardX"] = tb
    model, cfg = H.reference_model({"RCNN": {"ENABLED": False}}, eval_mode="rpn")
    cfg.RPN.ENABLED, cfg.RCNN.ENABLED = True, False
    argv, sys.argv = sys.argv, ["eval_rcnn.py", "--eval_mode", "rpn", "--save_result", "--save_rpn_feature", "--batch_size", "2"]
    sys.path.append(os.path.join(H.REF, "tools"))
    try:
        ref_eval = importlib.import_module("eval_rcnn")
    finally:
        sys.argv = argv
    assert ref_eval.__file__.startswith("/root/reference/") and ref_eval.args.save_rpn_feature and not ref_eval.args.test
    sd, checksum = helpers.seeded_state_dict(model.state_dict(), A_SEED)
    model.load_state_dict(sd)
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    import lib.utils.iou3d.iou3d_utils as iu
    captured = []
    pl_forward = model.rpn.proposal_layer.forward

    def capture(*a, **k):
        r = pl_forward(*a, **k)
        captured.append((r[0].clone(), r[1].clone()))
        return r
    model.rpn.proposal_layer.forward = capture
    with tempfile.TemporaryDirectory() as tmp:
        ids = rpn_tree.write_labelled_kitti_tree(tmp)
        ds = KittiRCNNDataset(root_dir=tmp, npoints=cfg.RPN.NUM_POINTS, split="val", mode="EVAL", random_select=True,
                              classes=cfg.CLASSES, logger=logging.getLogger("g16"), npoints_faraway=4000)
        get = ds.get_rpn_sample

        def seeded(index):
            np.random.seed(1024 + int(ds.sample_id_list[index]))
            return get(index)
        ds.get_rpn_sample = seeded
        with torch.no_grad():     # the segmentation threshold centred on the 70th percentile of the scores, as g12
            s0 = seeded(0)
            raw = model({"pts_input": torch.from_numpy(s0["pts_input"][None])})["rpn_cls"]
            model.rpn.rpn_cls_layer[-1].conv.bias += float(-0.8473 - torch.quantile(raw.view(-1), 0.7))
        captured.clear()
        loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, num_workers=0, collate_fn=ds.collate_batch)
        res_dir = os.path.join(tmp, "res")
        with torch.no_grad():
            ret = ref_eval.eval_one_epoch_rpn(model, loader, "g16", res_dir, logging.getLogger("g16"))
        out["a_ids"] = np.array(ids, np.int64)
        out["a_seed"] = np.int64(A_SEED)
        out["a_weights_checksum"] = np.float64(checksum)
        out["a_rpn_cls_bias"] = model.rpn.rpn_cls_layer[-1].conv.bias.detach().clone().numpy()
        out["a_ret_keys"] = np.array(sorted(ret))
        out["a_ret_values"] = np.array([float(ret[k]) for k in sorted(ret)])
        out["a_rois"] = torch.cat([c[0] for c in captured]).numpy()
        out["a_roi_scores"] = torch.cat([c[1] for c in captured]).numpy()
        margins = []
        for pos, sid in enumerate(ids):
            seg = np.load(os.path.join(res_dir, "seg_result", "%06d.npy" % sid))
            out["a_seg_xyz_sum_%d" % sid] = seg[:, :3].astype(np.float64).sum(0)
            out["a_seg_gt_%d" % sid] = seg[:, 3].astype(np.int8)
            out["a_seg_pred_%d" % sid] = seg[:, 4].astype(np.int8)
            out["a_seg_shape_%d" % sid] = np.array(seg.shape)
            out["a_det_%d" % sid] = np.array(open(os.path.join(res_dir, "detections", "data", "%06d.txt" % sid)).read())
            fdir = os.path.join(res_dir, "features")
            for suf in ("", "_xyz", "_seg", "_intensity", "_rawscore"):
                a = np.load(os.path.join(fdir, "%06d%s.npy" % (sid, suf)))
                out["a_feat%s_dtype_%d" % (suf, sid)] = np.array(str(a.dtype))
                out["a_feat%s_shape_%d" % (suf, sid)] = np.array(a.shape)
                out["a_feat%s_%d" % (suf, sid)] = a[::97]
            raw = np.load(os.path.join(fdir, "%06d_rawscore.npy" % sid)).astype(np.float64)
            margins.append(float(np.abs(raw - np.log(0.3 / 0.7)).min()))
            gt = ds.filtrate_objects(ds.get_label(sid))
            if gt:
                from lib.utils import kitti_utils as K
                g = torch.from_numpy(K.objs_to_boxes3d(gt).astype(np.float32))
                best = iu.boxes_iou3d_gpu(captured[pos // 2][0][pos % 2], g).max(dim=0).values.numpy()
                out["a_gt_best_iou_%d" % sid] = best
                print("g16a scene %d: %d cars, best IoUs %s" % (sid, len(gt), np.round(best, 3).tolist()))
        print("g16a ret_dict", ret)
        print("g16a min |raw - logit(0.3)| per scene", margins)


def main():
    H.install()
    from lib.datasets.kitti_rcnn_dataset import KittiRCNNDataset
    from lib.utils import kitti_utils as K
    from importlib import import_module
    synth = import_module("3d_adapt_auto_driving_amd.synth")
    gen = KittiRCNNDataset.generate_rpn_training_labels
    out = {"lidar_seeds": np.array(LIDAR_SEEDS), "lidar_cars": np.array(LIDAR_CARS)}

    def record(case, s, pts, gt, keep_pts):
        cls, reg = gen(pts, gt)
        out["%s_gt_%d" % (case, s)] = gt
        if keep_pts:
            out["%s_pts_%d" % (case, s)] = pts
        out["%s_cls_%d" % (case, s)] = cls.astype(np.int8)
        idx = np.nonzero(np.any(reg != 0, axis=1))[0].astype(np.int32)
        out["%s_regidx_%d" % (case, s)] = idx
        out["%s_reg_%d" % (case, s)] = reg[idx]
        print(case, s, "boxes", gt.shape[0], "fg", int((cls == 1).sum()), "ignore", int((cls == -1).sum()))

    for s, (seed, nc) in enumerate(zip(LIDAR_SEEDS, LIDAR_CARS)):
        pts, cars = synth.lidar_scene_with_labels(seed, 16384, nc)
        record("lidar", s, np.ascontiguousarray(pts[:, :3], dtype=np.float32), cars.astype(np.float32).reshape(-1, 7), False)
    boxes, pts = crafted()
    record("crafted", 0, pts, boxes, True)
    rng = np.random.default_rng(300)
    many = np.zeros((300, 7), dtype=np.float32)
    many[:, 0] = rng.uniform(-38, 38, 300); many[:, 2] = rng.uniform(2, 68, 300); many[:, 1] = rng.uniform(1.0, 2.0, 300)
    many[:, 3] = rng.uniform(0.5, 3, 300); many[:, 4] = rng.uniform(0.4, 3, 300); many[:, 5] = rng.uniform(0.4, 6, 300)
    many[:, 6] = rng.uniform(-np.pi, np.pi, 300)
    mpts = synth.lidar_scene_with_labels(1699, 16384, 10)[0][:, :3].astype(np.float32)
    record("many", 0, np.ascontiguousarray(mpts), many, True)
    cin = np.concatenate([boxes, many]).astype(np.float32)
    out["corners_in"] = cin
    out["corners_ref"] = K.boxes3d_to_corners3d(cin)
    part_a(out)
    path = os.path.join(HERE, "g16_rpn_labels_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
