"""A small labelled fake KITTI tree for the GT database (tests/golden g18, tests/test_gt_database.py, tests/test_gpu_gt_database.py).

tests/rpn_tree.py's tree cannot express what the database's filter and extraction branch on (levels, objects without points, a pair
of overlapping boxes), so this builder writes its own: KITTI/object/training/{velodyne, calib, label_2}/%06d.* and
KITTI/ImageSets/train.txt, a few thousand points per scene, everything from one seed.

  scene 0  two overlapping Cars that share points (Easy, Moderate), a Car whose 2-D box is 20 px high and a Car with occlusion 3
           (both UnKnown: filtered out), a Car far from every point (an entry with no points), Van / DontCare lines, a Pedestrian
           (Easy) and a Cyclist (Hard)
  scene 1  no valid object of any class: a Van, a DontCare, an UnKnown Car and an UnKnown Pedestrian
  scene 2  a 24 m long Car with points along its whole length (those more than 10 m from the centre along x are outside:
           roipool3d.cpp:86), a rotated Car, a truncated Car (0.60: UnKnown), two Pedestrians, one of them with no points
  scene 3  one Car, one Cyclist, and a Tram
"""
import os

import numpy as np

import helpers

TREE_SEED = 1800
SAMPLE_IDS = (3, 14, 25, 36)
N_BACKGROUND = 2400
N_CLUSTER = 160

# cls, truncation, occlusion, box2d height, (h, w, l), (x, y_bottom, z), ry, points around it
_SCENES = (
    (("Car", 0.00, 0, 60, (1.52, 1.63, 3.88), (2.00, 1.65, 14.00), 0.30, True),
     ("Car", 0.10, 1, 45, (1.48, 1.60, 4.10), (2.90, 1.62, 15.10), 0.55, True),          # overlaps the first
     ("Car", 0.00, 0, 19, (1.50, 1.60, 3.90), (-6.00, 1.70, 30.00), -1.20, True),        # height 20 < 25
     ("Car", 0.00, 3, 50, (1.50, 1.60, 3.90), (8.00, 1.70, 22.00), 2.00, True),          # occlusion unknown
     ("Car", 0.00, 0, 40, (1.45, 1.58, 3.70), (34.00, 1.60, 66.00), -2.60, False),       # valid, no point inside
     ("Van", 0.00, 0, 70, (2.10, 1.90, 5.00), (-8.00, 1.75, 18.00), 1.57, True),
     ("Pedestrian", 0.00, 0, 80, (1.75, 0.60, 0.80), (-2.50, 1.68, 9.00), 0.10, True),
     ("Cyclist", 0.40, 2, 30, (1.70, 0.60, 1.80), (5.00, 1.66, 11.00), -0.70, True),
     ("DontCare",)),
    (("Van", 0.00, 0, 70, (2.10, 1.90, 5.00), (3.00, 1.75, 20.00), -0.40, True),
     ("DontCare",),
     ("Car", 0.00, 0, 12, (1.50, 1.60, 3.90), (-4.00, 1.70, 45.00), 0.00, True),
     ("Pedestrian", 0.00, 3, 60, (1.70, 0.55, 0.70), (1.00, 1.66, 8.00), 0.90, True)),
    (("Car", 0.00, 0, 55, (1.60, 1.80, 24.00), (0.00, 1.70, 25.00), 0.00, True),          # the 10 m rule cuts its ends off
     ("Car", 0.20, 1, 35, (1.55, 1.66, 4.20), (-9.00, 1.72, 33.00), -2.35, True),
     ("Car", 0.60, 0, 90, (1.50, 1.62, 3.80), (6.00, 1.60, 6.00), 0.05, True),           # truncation 0.6
     ("Pedestrian", 0.00, 1, 26, (1.80, 0.65, 0.90), (4.00, 1.70, 16.00), 3.10, True),
     ("Pedestrian", 0.30, 2, 25, (1.60, 0.50, 0.60), (-30.00, 1.60, 64.00), -3.10, False),
     ("DontCare",)),
    (("Car", 0.15, 0, 39, (1.40, 1.55, 3.50), (-3.00, 1.58, 12.00), 1.00, True),           # height 40: Easy at the bound
     ("Cyclist", 0.00, 0, 41, (1.72, 0.58, 1.75), (7.00, 1.69, 19.00), -1.57, True),
     ("Tram", 0.00, 0, 99, (3.50, 2.60, 15.00), (-12.00, 1.90, 40.00), 0.02, True)),
)


def _label_line(rng, rec):
    u0, v0 = rng.uniform(0, 900), rng.uniform(100, 200)
    if rec[0] == "DontCare":
        return "DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n" % (u0, v0, u0 + 40, v0 + 30)
    cls, trunc, occ, height, hwl, pos, ry, _ = rec
    alpha = rng.uniform(-np.pi, np.pi)
    return "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (
        (cls, trunc, occ, alpha, u0, v0, u0 + 1.5 * height, v0 + height) + hwl + pos + (ry,))


def _cluster(rng, rec):
    """Rect-frame points in and around the box: 1.3 x its extents, so that some fall outside every face."""
    _, _, _, _, (h, w, l), (x, y, z), ry, _ = rec
    loc = rng.uniform(-0.65, 0.65, (N_CLUSTER, 3)) * [l, h, w]
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([x + loc[:, 0] * c + loc[:, 2] * s, y - h / 2 + loc[:, 1], z - loc[:, 0] * s + loc[:, 2] * c], 1)


def scene(pos, seed=TREE_SEED):
    """-> (velodyne (n, 4) f32, calib dict, label lines) of scene ``pos``."""
    rng = np.random.default_rng(seed + pos)
    cal = helpers.fake_kitti_calib(rng)
    lines = [_label_line(rng, rec) for rec in _SCENES[pos]]
    rect = [np.stack([rng.uniform(-20, 20, N_BACKGROUND), rng.uniform(-1.0, 2.2, N_BACKGROUND), rng.uniform(3, 60, N_BACKGROUND)], 1)]
    rect += [_cluster(rng, rec) for rec in _SCENES[pos] if rec[0] != "DontCare" and rec[-1]]
    rect = np.concatenate(rect, 0)
    rect = rect[rng.permutation(len(rect))]
    rect = rect[:len(rect) - (pos * 29) % 64]                                    # clouds of different, non-tile-aligned sizes
    Rv, tv = cal["Tr_velo_to_cam"][:, :3], cal["Tr_velo_to_cam"][:, 3]
    velo = (rect @ cal["R0_rect"] - tv) @ Rv                                       # rect = R0 (Rv x + tv)
    lidar = np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32)
    return lidar, cal, lines


def write_gt_tree(root, seed=TREE_SEED):
    """-> the sample ids of a tree under ``root`` (KITTI/object/training/{velodyne, calib, label_2}, KITTI/ImageSets/train.txt)"""
    base = os.path.join(root, "KITTI", "object", "training")
    for sub in ("velodyne", "calib", "label_2"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
    for pos, sid in enumerate(SAMPLE_IDS):
        lidar, cal, lines = scene(pos, seed)
        lidar.tofile(os.path.join(base, "velodyne", "%06d.bin" % sid))
        with open(os.path.join(base, "calib", "%06d.txt" % sid), "w") as f:
            for key in ("P0", "P1", "P2", "P3", "R0_rect", "Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in cal[key].reshape(-1))))
        with open(os.path.join(base, "label_2", "%06d.txt" % sid), "w") as f:
            f.writelines(lines)
    with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in SAMPLE_IDS))
    return list(SAMPLE_IDS)
