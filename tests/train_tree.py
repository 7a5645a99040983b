"""A labelled fake KITTI tree for the RPN training input stage (tests/golden g20, tests/test_train_input.py,
tests/test_gpu_train_input.py), with a layout of its own: every object stands near a node of a 7 m x 7 m grid (x = -35 + 7 i,
z = 8 + 7 j).  Two objects of the SAME node overlap heavily (IoU far above 1e-3), two objects of different nodes are metres apart
even with w, l + 0.5 on both, so under the online overlap rule no pair of the tree comes near the band 0 < IoU < 1e-3 -- whatever the
random stream draws.  The generator of g20 checks this on the reference's run.

  P / Q        two cars at ry = 0 on one row, 0.15 m between them (node (2, 1) and 4.15 m further along x; node (3, 1) stays empty):
               they collide only through the + 0.5 enlargement
  shared nodes cars of different scenes on one node: pasted into a third scene the second is rejected against the first only
  scene 1      40 raw points and Vans (not of the class, but label boxes) on almost every node of the database: fewer than 512 points
  scene 2      66 Tram labels far outside PC_AREA_SCOPE: more than 64 non-DontCare boxes
  scene 3      700 raw points and Vans on most nodes: between npoints / 2 and npoints points
  a car at z = 72 (the range-check skip), a car without points (the fewer-than-5-points skip); cars with ~30 points ("hard") and with
  more than 100 ("easy")
  400007       a pre-made aug scene (id >= 200000): rect rows in KITTI/aug_scene/training/rectified_data, its label in label_2 (the
               reference's get_label reads label_2 below id 2 000 000), calib / image / plane of scene 7

``ImageSets/train.txt`` lists the six scenes (the GT database is made from it), ``ImageSets/train_online.txt`` adds 400007.
Use npoints = 1024 and npoints_faraway = 128.  ``make_scene`` / ``write_scene`` build any such tree from scene specs (the GPU sweep's small trees).
"""
import os

import numpy as np

import helpers

TREE_SEED = 2000
SPLIT = "train_online"
NPOINTS, NPOINTS_FARAWAY = 1024, 128
IMG_SHAPE = (375, 1242)
AUG_ID = 400007
BASE_IDS = (2, 7, 11, 19, 23, 30)
SAMPLE_IDS = BASE_IDS + (AUG_ID,)
N_EXTRA_LABELS = 66
EMPTY_NODE = (3, 1)


def node(i, j):
    return -35.0 + 7.0 * i, 8.0 + 7.0 * j


# the database's nodes: scene position -> [(i, j, points)]; shared nodes appear in two scenes
_CARS = {
    0: [(2, 1, 40), (5, 2, 300), (7, 4, 30), (4, 6, 300), (8, 1, 30)],          # (2, 1) is P
    1: [(6, 1, 30), (5, 2, 30), (3, 4, 40)],
    2: [(7, 4, 300), (6, 6, 30), (2, 3, 300), (8, 1, 30), (4, 1, 30)],
    3: [(5, 5, 30), (4, 6, 30)],
    4: [(3, 4, 300), (6, 3, 30), (8, 5, 300), (6, 1, 300), (5, 0, 30)],
    5: [(2, 3, 30), (6, 6, 300), (7, 2, 30), (4, 3, 300)],
}
_Q_SCENE = 1                                                                      # Q goes into scene 1
_VAN_KEEP = {1: ((5, 0), (7, 2)), 3: ((4, 3), (6, 3), (5, 0), (8, 5))}            # the database nodes these scenes leave free
_BACKGROUND = {0: 2500, 1: 40, 2: 2300, 3: 700, 4: 2600, 5: 2100}


def _line(cls, hwl, pos, ry, alpha, occ=0, box_h=60.0):
    return "%s 0.00 %d %.2f 100.00 100.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (
        (cls, occ, alpha, 100.0 + 1.5 * box_h, 100.0 + box_h) + tuple(hwl) + tuple(pos) + (ry,))


def _cluster(rng, hwl, pos, ry, n):
    """n rect-frame points in and around the box (1.3 x its extents)"""
    h, w, l = hwl
    x, y, z = pos
    loc = rng.uniform(-0.65, 0.65, (n, 3)) * [l, h, w]
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([x + loc[:, 0] * c + loc[:, 2] * s, y - h / 2 + loc[:, 1], z - loc[:, 0] * s + loc[:, 2] * c], 1)


def car_on_node(rng, i, j):
    """-> (hwl, pos, ry) of a car within 0.3 m of node (i, j)"""
    x, z = node(i, j)
    hwl = (round(rng.uniform(1.4, 1.6), 2), round(rng.uniform(1.55, 1.7), 2), round(rng.uniform(3.6, 4.2), 2))
    pos = (round(x + rng.uniform(-0.3, 0.3), 2), round(rng.uniform(1.6, 1.72), 2), round(z + rng.uniform(-0.3, 0.3), 2))
    return hwl, pos, round(rng.uniform(-3.1, 3.1), 2)


def scene_spec(pos, seed=TREE_SEED):
    """-> (label lines, [(hwl, pos, ry, points)] clusters, background points) of scene ``pos``"""
    rng = np.random.default_rng(seed + pos)
    lines, clusters = [], []
    for i, j, n in _CARS[pos]:
        hwl, p, ry = car_on_node(rng, i, j)
        if (pos, i, j) == (0, 2, 1):                                             # P
            hwl, p, ry = (1.5, 1.6, 4.0), (node(2, 1)[0], 1.65, node(2, 1)[1]), 0.0
        lines.append(_line("Car", hwl, p, ry, rng.uniform(-3.1, 3.1)))
        clusters.append((hwl, p, ry, n))
    if pos == _Q_SCENE:                                                          # Q
        hwl, p = (1.5, 1.6, 4.0), (node(2, 1)[0] + 4.15, 1.65, node(2, 1)[1])
        lines.append(_line("Car", hwl, p, 0.0, 0.3))
        clusters.append((hwl, p, 0.0, 40))
    if pos == 0:
        lines.append(_line("Car", (1.45, 1.58, 3.7), (0.0, 1.6, 72.0), 0.2, 0.1))                 # outside PC_AREA_SCOPE
        clusters.append(((1.45, 1.58, 3.7), (0.0, 1.6, 72.0), 0.2, 40))
        lines.append("DontCare -1 -1 -10 500.00 150.00 540.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10\n")
    if pos == 4:
        lines.append(_line("Car", (1.5, 1.6, 3.9), node(9, 8)[:1] + (1.6,) + node(9, 8)[1:], -2.6, 1.0))  # no point inside
    if pos in _VAN_KEEP:
        nodes = sorted({(i, j) for cars in _CARS.values() for i, j, _ in cars} | {(2, 1)})
        own = {(i, j) for i, j, _ in _CARS[pos]}
        for i, j in nodes:
            if (i, j) not in own and (i, j) not in _VAN_KEEP[pos] and not (pos == _Q_SCENE and (i, j) == (2, 1)):
                hwl, p, ry = car_on_node(rng, i, j)
                if (i, j) == (2, 1):                                             # P's pose: Q meets it through the enlargement only
                    hwl, p, ry = (1.5, 1.6, 4.0), (node(2, 1)[0], 1.65, node(2, 1)[1]), 0.0
                lines.append(_line("Van", hwl, p, ry, 0.0))
    if pos == 2:
        lines += [_line("Tram", (3.5, 2.6, 15.0), (60.0 + 4.0 * (k % 2), 1.9, 90.0 + 20.0 * k), 0.02, 0.0) for k in range(N_EXTRA_LABELS)]
    lines.append(_line("Pedestrian", (1.75, 0.6, 0.8), node(10, 8)[:1] + (1.66,) + node(10, 8)[1:], 0.1, 0.5))
    return lines, clusters, _BACKGROUND[pos]


def make_scene(rng, lines, clusters, n_background):
    """-> (velodyne (n, 4) f32, calib dict, plane (4,), rect rows (n, 4) f32)"""
    cal = helpers.fake_kitti_calib(rng)
    rect = [np.stack([rng.uniform(-20, 20, n_background), rng.uniform(-1.0, 2.2, n_background), rng.uniform(3, 60, n_background)], 1)]
    rect += [_cluster(rng, hwl, p, ry, n) for hwl, p, ry, n in clusters]
    rect = np.concatenate(rect, 0)
    rect = rect[rng.permutation(len(rect))]
    Rv, tv = cal["Tr_velo_to_cam"][:, :3], cal["Tr_velo_to_cam"][:, 3]
    velo = (rect @ cal["R0_rect"] - tv) @ Rv
    inten = rng.random((len(velo), 1))
    plane = np.array([rng.uniform(-0.01, 0.01), -1.0, rng.uniform(-0.01, 0.01), 1.65 + rng.uniform(-0.05, 0.05)])
    return (np.concatenate([velo, inten], 1).astype(np.float32), cal, plane,
            np.concatenate([rect, inten], 1).astype(np.float32))


def write_scene(root, sid, lidar, cal, lines, plane):
    from PIL import Image
    base = os.path.join(root, "KITTI", "object", "training")
    for sub in ("velodyne", "calib", "label_2", "planes", "image_2"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    if lidar is not None:
        lidar.tofile(os.path.join(base, "velodyne", "%06d.bin" % sid))
    with open(os.path.join(base, "label_2", "%06d.txt" % sid), "w") as f:
        f.writelines(lines)
    if cal is None:
        return
    with open(os.path.join(base, "calib", "%06d.txt" % sid), "w") as f:
        for key in ("P0", "P1", "P2", "P3", "R0_rect", "Tr_velo_to_cam", "Tr_imu_to_velo"):
            f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in cal[key].reshape(-1))))
    with open(os.path.join(base, "planes", "%06d.txt" % sid), "w") as f:
        f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % " ".join("%.6e" % v for v in plane))
    Image.new("RGB", (IMG_SHAPE[1], IMG_SHAPE[0])).save(os.path.join(base, "image_2", "%06d.png" % sid))


def write_aug_rows(root, sid, rows, lines):
    d = os.path.join(root, "KITTI", "aug_scene", "training", "rectified_data")
    os.makedirs(d, exist_ok=True)
    os.makedirs(os.path.join(root, "KITTI", "aug_scene", "training", "aug_label"), exist_ok=True)
    rows.astype(np.float32).tofile(os.path.join(d, "%06d.bin" % sid))
    write_scene(root, sid, None, None, lines, None)


def write_split(root, name, ids):
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
    with open(os.path.join(root, "KITTI", "ImageSets", name + ".txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in ids))


def write_train_tree(root, seed=TREE_SEED):
    """-> the sample ids of ``train_online``"""
    for pos, sid in enumerate(BASE_IDS):
        lines, clusters, nb = scene_spec(pos, seed)
        lidar, cal, plane, rows = make_scene(np.random.default_rng(seed + 50 + pos), lines, clusters, nb)
        write_scene(root, sid, lidar, cal, lines, plane if pos % 2 == 0 else -plane)
        if sid == AUG_ID % 200000:
            # the pre-made aug scene: this scene's labels over a fuller cloud in the rect frame
            more = make_scene(np.random.default_rng(seed + 90), lines, clusters, 1800)[3]
            write_aug_rows(root, AUG_ID, more, lines)
    write_split(root, "train", BASE_IDS)
    write_split(root, SPLIT, SAMPLE_IDS)
    return list(SAMPLE_IDS)
