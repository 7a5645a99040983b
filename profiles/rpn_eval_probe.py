"""Times of --eval_mode rpn: the label kernel (csrc/rpn_labels.hip) for B = 8, N = 16384 and G = 20 / 60 / 300 boxes per scene,
the numpy path, the reference's Delaunay labels (scipy) when scipy is present, and the RPN-mode driver's scenes/s on the
synthetic source.  Prints one JSON line.

    python profiles/rpn_eval_probe.py [--scenes 256] [--batch 8]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "3d_adapt_auto_driving_amd"


def boxes(rng, G):
    b = np.zeros((G, 7), dtype=np.float32)
    b[:, 0] = rng.uniform(-30, 30, G); b[:, 2] = rng.uniform(3, 65, G); b[:, 1] = rng.uniform(1.2, 2.0, G)
    b[:, 3] = rng.uniform(1.3, 1.7, G); b[:, 4] = rng.uniform(1.5, 1.8, G); b[:, 5] = rng.uniform(3.5, 4.5, G)
    b[:, 6] = rng.uniform(-np.pi, np.pi, G)
    return b


def delaunay_labels(pts, gt):
    """the reference's generate_rpn_training_labels restated with scipy (timing only)"""
    from scipy.spatial import Delaunay
    rpn_eval = importlib.import_module(PKG + ".rpn_eval")
    big = gt.copy(); big[:, 3:6] += np.float32(0.4); big[:, 1] += np.float32(0.2)
    ry = gt[:, 6]
    c0 = rpn_eval.box_corners(gt, np.cos(ry), np.sin(ry))
    c1 = rpn_eval.box_corners(big, np.cos(ry), np.sin(ry))
    cls = np.zeros(len(pts), np.int32)
    for k in range(len(gt)):
        fg = Delaunay(c0[k]).find_simplex(pts) >= 0
        cls[fg] = 1
        cls[fg != (Delaunay(c1[k]).find_simplex(pts) >= 0)] = -1
    return cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    import torch
    rpn_eval = importlib.import_module(PKG + ".rpn_eval")
    synth = importlib.import_module(PKG + ".synth")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    B, N = 8, 16384
    pts = np.stack([synth.lidar_scene_with_labels(500 + s, N, 10)[0][:, :3] for s in range(B)]).astype(np.float32)
    tp = torch.from_numpy(pts).to(dev)
    scores = torch.randn((B, N), device=dev)
    res = {"B": B, "N": N}
    for G in (20, 60, 300):
        gt, counts, trig = rpn_eval.pack_gt([boxes(rng, G) for _ in range(B)])
        st = torch.zeros((B, 3), dtype=torch.int32, device=dev)
        for _ in range(5):
            rpn_eval.rpn_labels(tp, gt, counts, device=dev, trig=trig, scores_raw=scores, thresh=0.3, stats=st)
        torch.cuda.synchronize()
        # device time of the whole call (H2D of the boxes + both launches), events around 50 calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            rpn_eval.rpn_labels(tp, gt, counts, device=dev, trig=trig, scores_raw=scores, thresh=0.3, stats=st)
        e1.record(); torch.cuda.synchronize()
        res["kernel_ms_G%d" % G] = round(e0.elapsed_time(e1) / 50, 4)
        t0 = time.perf_counter()
        rpn_eval.rpn_labels(pts, gt, counts, device="cpu", trig=trig, want_reg=True)
        res["numpy_ms_G%d" % G] = round((time.perf_counter() - t0) * 1e3, 1)
        try:
            t0 = time.perf_counter()
            delaunay_labels(pts[0], gt[0, :G])
            res["delaunay_ms_per_scene_G%d" % G] = round((time.perf_counter() - t0) * 1e3, 1)
        except ImportError:
            res["delaunay_ms_per_scene_G%d" % G] = "scipy not present"
    er = importlib.import_module(PKG + ".eval_rcnn")
    config = importlib.import_module(PKG + ".config")
    kitti_io = importlib.import_module(PKG + ".kitti_io")
    cfg = config.make_cfg(); config.apply_eval_defaults(cfg, "rpn")
    model = er.build_model(cfg, dev, seed=0).eval()
    src = kitti_io.SyntheticSource(cfg, args.scenes)
    er.eval_scenes_rpn(model, cfg, dev, src, src.ids[:2 * args.batch], args.batch, stats=rpn_eval.RpnStats(dev))
    stats = rpn_eval.RpnStats(dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    er.eval_scenes_rpn(model, cfg, dev, src, src.ids, args.batch, stats=stats)
    stats.result()
    res["rpn_driver_synthetic_scenes_per_s"] = round(args.scenes / (time.perf_counter() - t0), 1)
    # a KITTI-format tree (synth.write_kitti_tree: 16 distinct ray-cast sweeps) with label files holding the sweeps' cars: file reads,
    # rectification and the host sampler on the feeding thread; then again with --save_result --save_rpn_feature writers on
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        synth.write_kitti_tree(tmp, args.scenes, pool=16, processes=8)
        ldir = os.path.join(tmp, "KITTI", "object", "training", "label_2")
        os.makedirs(ldir, exist_ok=True)
        cars = [synth.lidar_raw_with_labels(50000 + k)[1] for k in range(16)]
        for i in range(args.scenes):
            with open(os.path.join(ldir, "%06d.txt" % i), "w") as f:
                for x, y, z, h, w, l, ry in cars[i % 16]:
                    f.write("Car 0.00 0 0.00 0 0 10 10 %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (h, w, l, x, y, z, ry))
        ksrc = kitti_io.KittiSource(tmp, cfg, "val")
        er.eval_scenes_rpn(model, cfg, dev, ksrc, ksrc.ids[:2 * args.batch], args.batch, stats=rpn_eval.RpnStats(dev))
        for save in (False, True):
            out = os.path.join(tmp, "out") if save else None
            t0 = time.perf_counter()
            er.eval_scenes_rpn(model, cfg, dev, ksrc, ksrc.ids, args.batch, out, save_feature=save, stats=rpn_eval.RpnStats(dev))
            res["rpn_driver_kitti_tree_scenes_per_s" + ("_with_files" if save else "")] = round(len(ksrc.ids) / (time.perf_counter() - t0), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
