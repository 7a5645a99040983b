"""A fake KITTI tree WITH label files, for the RPN evaluation mode (tests/golden g16 part a, tests/test_gpu_rpn_eval.py).

helpers.write_fake_kitti_tree writes the clouds, calibrations and images; this adds label_2/%06d.txt: the cars the sweep was
ray-cast with (synth.lidar_raw_with_labels), plus Van / Pedestrian / DontCare lines that the EVAL-mode class filter drops.  The
scene at NO_CAR_POS gets no Car line, so that a scene without GT is batched with one that has GT."""
import numpy as np

import helpers

TREE_SEED = 1600
NO_CAR_POS = 2
_synth = helpers._synth


def label_lines(seed, with_cars=True):
    cars = _synth.lidar_raw_with_labels(seed)[1] if with_cars else np.zeros((0, 7))
    rng = np.random.default_rng(seed + 99)
    fmt = "%s 0.00 0 %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n"
    box2d = lambda: tuple(rng.uniform(0, 300, 2)) + tuple(rng.uniform(300, 600, 2))
    lines = []
    for x, y, z, h, w, l, ry in cars:
        lines.append(fmt % (("Car", -1.0) + box2d() + (h, w, l, x, y, z, ry)))
    for name, hwl in (("Van", (2.1, 1.9, 5.0)), ("Pedestrian", (1.7, 0.6, 0.8)), ("DontCare", (-1, -1, -1))):
        x, z, ry = rng.uniform(-10, 10), rng.uniform(8, 50), rng.uniform(-np.pi, np.pi)
        if name == "DontCare":
            lines.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n" % box2d())
        else:
            lines.append(fmt % ((name, 0.5) + box2d() + hwl + (x, 1.65, z, ry)))
    return lines


def write_labelled_kitti_tree(root, seed=TREE_SEED):
    """-> the sample ids of a tree under ``root`` (KITTI/object/training/{velodyne, calib, image_2, label_2}, ImageSets/val.txt)"""
    import os
    ids = helpers.write_fake_kitti_tree(root, seed)
    for pos, sid in enumerate(ids):
        with open(os.path.join(root, "KITTI", "object", "training", "label_2", "%06d.txt" % sid), "w") as f:
            f.writelines(label_lines(seed + pos, with_cars=pos != NO_CAR_POS))
    return ids
