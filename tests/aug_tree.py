"""A labelled fake KITTI tree for augmented-scene generation (tests/golden g19, tests/test_aug_scene.py, tests/test_gpu_aug_scene.py):
tests/gt_tree.py's layout (its label lines and point clusters are reused) plus ``planes/`` and ``image_2/``, six scenes, enough cars
for a database of 27 entries.

What the tree holds for the tool's branches:
  A0 / A1 / A2   three cars in three scenes, in a row along x with 0.15 m between neighbours: pasted into one scene the second is
                 rejected against the first only because of the + 0.5 enlargement; B0 / B1 the same along z (the w side)
  a car at z = 72 (outside PC_AREA_SCOPE: the range-check skip), a car without points (the fewer-than-5-points skip), a car at
  z = 3.6 whose image box is wider than 80 % of the image (its label line is dropped), a pedestrian at z = 55 (outside the People
  scope) and one without points; scene 5 has no pedestrian or cyclist (skipped for People).  Every database object keeps its x, z,
  so a candidate pasted into its own scene meets its original.
  The plane files of the odd scenes are written with the normal facing down (get_road_plane flips it).
"""
import os

import numpy as np

import gt_tree
import helpers

TREE_SEED = 1900
SAMPLE_IDS = (2, 7, 11, 19, 23, 30)
IMG_SHAPE = (375, 1242)
N_BACKGROUND = 1600
CAR = (1.50, 1.60, 4.00)

# cls, truncation, occlusion, box2d height, (h, w, l), (x, y_bottom, z), ry, points around it
_SCENES = (
    (("Car", 0.00, 0, 60, CAR, (-10.00, 1.65, 12.00), 0.00, True),                       # A0
     ("Car", 0.10, 1, 45, (1.48, 1.60, 4.10), (6.00, 1.70, 20.00), 0.40, True),
     ("Car", 0.00, 0, 50, (1.52, 1.63, 3.88), (-3.00, 1.62, 33.00), -1.30, True),
     ("Car", 0.20, 1, 35, (1.55, 1.66, 4.20), (12.00, 1.68, 45.00), 2.80, True),
     ("Car", 0.00, 0, 40, (1.45, 1.58, 3.70), (0.00, 1.60, 72.00), 0.20, True),          # outside PC_AREA_SCOPE
     ("Pedestrian", 0.00, 0, 80, (1.75, 0.60, 0.80), (3.00, 1.66, 9.00), 0.10, True),
     ("Cyclist", 0.40, 2, 30, (1.70, 0.60, 1.80), (-6.00, 1.70, 25.00), -0.70, True),
     ("DontCare",)),
    (("Car", 0.00, 0, 60, CAR, (-5.85, 1.65, 12.00), 0.00, True),                        # A1
     ("Car", 0.00, 0, 42, (1.50, 1.62, 3.80), (9.00, 1.70, 28.00), 1.20, True),
     ("Car", 0.15, 0, 39, (1.40, 1.55, 3.50), (-14.00, 1.66, 40.00), -0.20, True),
     ("Car", 0.00, 1, 30, (1.60, 1.70, 4.40), (3.00, 1.60, 52.00), 0.90, True),
     ("Car", 0.00, 0, 40, (1.45, 1.58, 3.70), (30.00, 1.60, 66.00), -2.60, False),       # no point inside
     ("Pedestrian", 0.00, 1, 26, (1.80, 0.65, 0.90), (-2.00, 1.70, 14.00), 3.10, True),
     ("Pedestrian", 0.30, 2, 25, (1.60, 0.50, 0.60), (-25.00, 1.60, 45.00), -3.10, False),
     ("DontCare",)),
    (("Car", 0.00, 0, 60, CAR, (-1.70, 1.65, 12.00), 0.00, True),                        # A2
     ("Car", 0.00, 0, 55, (1.50, 1.60, 3.90), (15.00, 1.72, 18.00), -2.00, True),
     ("Car", 0.25, 1, 33, (1.46, 1.58, 3.60), (-8.00, 1.64, 26.00), 0.10, True),
     ("Car", 0.00, 2, 28, (1.58, 1.68, 4.30), (5.00, 1.70, 38.00), 1.57, True),
     ("Van", 0.00, 0, 70, (2.10, 1.90, 5.00), (-16.00, 1.75, 48.00), 1.57, True),
     ("Cyclist", 0.00, 0, 41, (1.72, 0.58, 1.75), (10.00, 1.68, 32.00), -1.57, True),
     ("Pedestrian", 0.00, 0, 44, (1.70, 0.55, 0.70), (2.00, 1.70, 55.00), 0.90, True)),  # outside the People scope
    (("Car", 0.00, 0, 48, CAR, (8.00, 1.66, 50.00), 0.00, True),                         # B0
     ("Car", 0.00, 0, 52, (1.50, 1.62, 3.80), (-16.00, 1.70, 16.00), 0.70, True),
     ("Car", 0.10, 1, 44, (1.44, 1.56, 3.66), (2.00, 1.63, 24.00), -0.60, True),
     ("Car", 0.30, 2, 27, (1.62, 1.72, 4.50), (-5.00, 1.70, 44.00), 3.00, True),
     ("Pedestrian", 0.00, 0, 70, (1.68, 0.62, 0.84), (6.00, 1.66, 12.00), 1.00, True),
     ("Cyclist", 0.10, 1, 36, (1.74, 0.60, 1.70), (-11.00, 1.70, 30.00), 0.30, True),
     ("DontCare",)),
    (("Car", 0.00, 0, 48, CAR, (8.00, 1.66, 51.75), 0.00, True),                         # B1
     ("Car", 0.00, 1, 37, (1.50, 1.60, 3.90), (-12.00, 1.70, 22.00), -1.00, True),
     ("Car", 0.05, 0, 46, (1.47, 1.61, 4.05), (14.00, 1.65, 34.00), 0.30, True),
     ("Car", 0.00, 0, 90, (1.50, 1.62, 3.80), (0.00, 1.70, 8.00), 0.00, True),
     ("Pedestrian", 0.20, 1, 31, (1.66, 0.58, 0.76), (-7.00, 1.70, 18.00), -2.00, True),
     ("Cyclist", 0.00, 0, 50, (1.70, 0.62, 1.82), (4.00, 1.68, 42.00), 2.20, True)),
    (("Car", 0.00, 0, 58, (1.50, 1.60, 3.90), (-4.00, 1.68, 15.00), 0.50, True),
     ("Car", 0.00, 1, 40, (1.53, 1.64, 4.12), (11.00, 1.70, 25.00), -0.80, True),
     ("Car", 0.28, 2, 29, (1.43, 1.57, 3.58), (-15.00, 1.62, 36.00), 1.90, True),
     ("Car", 0.00, 0, 60, CAR, (0.00, 1.70, 3.60), 0.00, True),                          # wider than 80 % of the image
     ("Car", 0.00, 0, 26, (1.50, 1.60, 3.90), (6.00, 1.70, 57.00), 0.20, True),          # the last entry: never drawn
     ("Tram", 0.00, 0, 99, (3.50, 2.60, 15.00), (-12.00, 1.90, 48.00), 0.02, True)),
)


def scene(pos, seed=TREE_SEED):
    """-> (velodyne (n, 4) f32, calib dict, label lines, plane (4,)) of scene ``pos``."""
    rng = np.random.default_rng(seed + pos)
    cal = helpers.fake_kitti_calib(rng)
    lines = [gt_tree._label_line(rng, rec) for rec in _SCENES[pos]]
    rect = [np.stack([rng.uniform(-20, 20, N_BACKGROUND), rng.uniform(-1.0, 2.2, N_BACKGROUND), rng.uniform(3, 60, N_BACKGROUND)], 1)]
    rect += [gt_tree._cluster(rng, rec) for rec in _SCENES[pos] if rec[0] != "DontCare" and rec[-1]]
    rect = np.concatenate(rect, 0)
    rect = rect[rng.permutation(len(rect))]
    rect = rect[:len(rect) - (pos * 29) % 64]                                    # clouds of different, non-tile-aligned sizes
    Rv, tv = cal["Tr_velo_to_cam"][:, :3], cal["Tr_velo_to_cam"][:, 3]
    velo = (rect @ cal["R0_rect"] - tv) @ Rv
    lidar = np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32)
    plane = np.array([rng.uniform(-0.01, 0.01), -1.0, rng.uniform(-0.01, 0.01), 1.65 + rng.uniform(-0.05, 0.05)])
    return lidar, cal, lines, plane if pos % 2 == 0 else -plane


def write_aug_tree(root, seed=TREE_SEED):
    """-> the sample ids of a tree under ``root``: KITTI/object/training/{velodyne, calib, label_2, planes, image_2} and
    KITTI/ImageSets/train.txt"""
    from PIL import Image
    base = os.path.join(root, "KITTI", "object", "training")
    for sub in ("velodyne", "calib", "label_2", "planes", "image_2"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
    for pos, sid in enumerate(SAMPLE_IDS):
        lidar, cal, lines, plane = scene(pos, seed)
        lidar.tofile(os.path.join(base, "velodyne", "%06d.bin" % sid))
        with open(os.path.join(base, "calib", "%06d.txt" % sid), "w") as f:
            for key in ("P0", "P1", "P2", "P3", "R0_rect", "Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in cal[key].reshape(-1))))
        with open(os.path.join(base, "label_2", "%06d.txt" % sid), "w") as f:
            f.writelines(lines)
        with open(os.path.join(base, "planes", "%06d.txt" % sid), "w") as f:
            f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%.6e" % v for v in plane))
        Image.new("RGB", (IMG_SHAPE[1], IMG_SHAPE[0])).save(os.path.join(base, "image_2", "%06d.png" % sid))
    with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in SAMPLE_IDS))
    return list(SAMPLE_IDS)
