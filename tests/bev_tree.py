"""A tiny KITTI-format tree for the BEV renderer's tests (tests/test_bev.py, tests/test_gpu_bev.py): 3 scenes of at most 500 points
with Car / Van / Pedestrian labels, its stat_norm conversion on the host, and a result folder with detections."""
import json
import os

import numpy as np

from conftest import pkg

G27 = os.path.join(os.path.dirname(__file__), "golden", "g27_bev_mask_ref.npz")
IDS = ["000000", "000001", "000002"]
STATS_SRC = {"height": {"mean": 1.52, "std": 0.14}, "width": {"mean": 1.63, "std": 0.10}, "length": {"mean": 3.88, "std": 0.43}}
STATS_DST = {"height": {"mean": 1.77, "std": 0.22}, "width": {"mean": 1.93, "std": 0.15}, "length": {"mean": 4.91, "std": 0.56}}
BOXES = [[("Car", [-3.0, 1.60, 8.0, 1.50, 1.60, 3.90, 0.30]), ("Van", [4.0, 1.70, 14.0, 2.00, 1.90, 5.00, -1.40]),
          ("Pedestrian", [0.5, 1.60, 5.0, 1.75, 0.60, 0.80, 2.0])],
         [("Car", [2.5, 1.65, 10.0, 1.45, 1.62, 4.05, 1.57])],
         [("Car", [-5.0, 1.60, 16.0, 1.55, 1.66, 4.20, -2.8]), ("Car", [6.0, 1.62, 6.5, 1.50, 1.58, 3.70, 0.0])]]


def label_line(cls, box, score=None):
    x, y, z, h, w, l, ry = box
    s = "%s 0.00 0 %.2f 100.00 120.00 180.00 200.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (cls, ry, h, w, l, x, y, z, ry)
    return s + (" %.2f" % score if score is not None else "")


def calib_text():
    return str(np.load(G27, allow_pickle=False)["calib_text"])


def make_tree(root):
    """root/src: the tree; root/dst: stat_norm convert --device cpu of it; root/results: detections for the first two ids -> paths"""
    SN = pkg("stat_norm")
    src, dst, res = os.path.join(root, "src"), os.path.join(root, "dst"), os.path.join(root, "results")
    tr = os.path.join(src, "training")
    for d in ("velodyne", "label_2", "calib"):
        os.makedirs(os.path.join(tr, d))
    os.makedirs(res)
    calib = SN.Calib(SN.parse_calib(calib_text()))
    for s, i in enumerate(IDS):
        rng = np.random.default_rng(40 + s)
        n_bg = (300, 120, 380)[s]
        rect = [np.stack([rng.uniform(-9, 9, n_bg), rng.uniform(-1.0, 1.8, n_bg), rng.uniform(1, 19, n_bg)], 1)]
        for _, (x, y, z, h, w, l, ry) in BOXES[s]:
            f = np.stack([rng.uniform(-0.45, 0.45, 40) * l, rng.uniform(-0.9, -0.1, 40) * h, rng.uniform(-0.45, 0.45, 40) * w], 1)
            rect.append(np.dot(f, SN._rot(ry).T) + [x, y, z])
        rect = np.concatenate(rect)
        velo = np.concatenate([calib.rect_to_velo(rect), rng.uniform(0, 1, (len(rect), 1))], 1).astype(np.float32)
        assert len(velo) <= 500
        velo.tofile(os.path.join(tr, "velodyne", i + ".bin"))
        with open(os.path.join(tr, "label_2", i + ".txt"), "w") as f:
            f.write("".join(label_line(c, b) + "\n" for c, b in BOXES[s]))
        with open(os.path.join(tr, "calib", i + ".txt"), "w") as f:
            f.write(calib_text())
        if s < 2:                                # the last id has no result file: no detections
            with open(os.path.join(res, i + ".txt"), "w") as f:
                for k, (c, b) in enumerate(BOXES[s]):
                    big = [b[0] + 0.3, b[1], b[2] - 0.4, b[3], b[4] + 0.3, b[5] + 0.9, b[6] + 0.05]
                    f.write(label_line(c, big, score=0.9 - 0.7 * k) + "\n")           # the second one is below the threshold
    for name, ids in (("train", IDS[:2]), ("val", IDS[2:]), ("trainval", IDS)):
        with open(os.path.join(src, name + ".txt"), "w") as f:
            f.write("\n".join(ids) + "\n")
    stats = []
    for name, st in (("s.json", STATS_SRC), ("d.json", STATS_DST)):
        stats.append(os.path.join(root, name))
        with open(stats[-1], "w") as f:
            json.dump(st, f)
    SN.main(["convert", src, dst, "--src_stats", stats[0], "--dst_stats", stats[1], "--device", "cpu", "--image_size", "1242", "375"])
    return src, dst, res
