"""Times RpnTrainInput.batch() for 8 scenes x 16384 points from 120 k-point clouds with 30 labels: the device path (uploads and the
per-scene reads inside the call, database resident; median of seven calls with the range) against the package's cpu path on the same
inputs, and the share of the call spent in the host's legacy-stream draws.   python profiles/train_input_probe.py
The reference's own loader is not timed (it needs shapely)."""
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "3d_adapt_auto_driving_amd"


def write_tree(root, n_scenes=8, n_points=120000, n_labels=30):
    import helpers
    from PIL import Image
    base = os.path.join(root, "KITTI", "object", "training")
    for sub in ("velodyne", "calib", "label_2", "planes", "image_2"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
    for sid in range(n_scenes):
        rng = np.random.default_rng(5000 + sid)
        cal = helpers.fake_kitti_calib(rng)
        boxes = [(rng.uniform(-35, 35), 1.65, 6 + 2.1 * k, rng.uniform(-3, 3)) for k in range(n_labels)]
        rect = [np.stack([rng.uniform(-40, 40, n_points), rng.uniform(-1, 2.5, n_points), rng.uniform(0, 70, n_points)], 1)]
        rect += [np.array([x, y - 0.75, z]) + rng.uniform(-0.7, 0.7, (400 if k % 2 else 60, 3)) for k, (x, y, z, _) in enumerate(boxes)]
        rect = np.concatenate(rect)               # every second car has more than 100 points (the "easy" list)
        Rv, tv = cal["Tr_velo_to_cam"][:, :3], cal["Tr_velo_to_cam"][:, 3]
        velo = (rect @ cal["R0_rect"] - tv) @ Rv
        np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32).tofile(os.path.join(base, "velodyne", "%06d.bin" % sid))
        with open(os.path.join(base, "calib", "%06d.txt" % sid), "w") as f:
            for key in ("P0", "P1", "P2", "P3", "R0_rect", "Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in cal[key].reshape(-1))))
        with open(os.path.join(base, "label_2", "%06d.txt" % sid), "w") as f:
            for x, y, z, ry in boxes:
                f.write("Car 0.00 0 0.00 100.00 100.00 200.00 160.00 1.50 1.60 3.90 %.2f %.2f %.2f %.2f\n" % (x, y, z, ry))
        with open(os.path.join(base, "planes", "%06d.txt" % sid), "w") as f:
            f.write("# Plane\nWidth 4\nHeight 1\n0.0 -1.0 0.0 1.65\n")
        Image.new("RGB", (1242, 375)).save(os.path.join(base, "image_2", "%06d.png" % sid))
    with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(n_scenes)))


def main():
    import torch
    T = importlib.import_module(PKG + ".train_input")
    G = importlib.import_module(PKG + ".gt_database")
    cfg = importlib.import_module(PKG + ".config").make_cfg()
    cfg["GT_AUG_ENABLED"], cfg["GT_AUG_RAND_NUM"], cfg["GT_AUG_APPLY_PROB"] = True, True, 1.0
    with tempfile.TemporaryDirectory() as root:
        write_tree(root)
        G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cuda", log=lambda *a: None)
        db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
        for device, calls in (("cuda", 8), ("cpu", 2)):
            src = T.RpnTrainInput(root, cfg, db, npoints=16384, seed=1, device=device)
            times, shares = [], []
            for k in range(calls):
                src.stats["draw_seconds"] = 0.0
                t0 = time.perf_counter()
                src.batch(range(8))
                if device == "cuda":
                    torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if k or device == "cpu":                                     # the device path's first call warms up
                    times.append(dt)
                    shares.append(src.stats["draw_seconds"] / dt)
            print("%s: batch() of 8 scenes median %.1f ms (min %.1f, max %.1f, %d calls, file reads included); "
                  "host stream draws %.0f %% of the call" % (device, 1e3 * np.median(times), 1e3 * min(times), 1e3 * max(times),
                                                             len(times), 100 * np.median(shares)))


if __name__ == "__main__":
    main()
