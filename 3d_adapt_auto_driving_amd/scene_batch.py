"""What the ragged-scene data modules share on the host (gt_database.py, stat_norm.py, aug_scene.py, train_input.py, road_planes.py, beam_resample.py;
the device side is csrc/scene_tiles.hpp and csrc/placement.hpp): a batch of scenes packed back to back with its offsets and 64-point tiles,
the one-copy upload of a call's host arrays, the
valid-point filter of the reference's loaders in numpy, the small box / database / label helpers of object placement, and the sample
list of a split (with the few-shot --subsample rule).
"""
import os
import random
import types

import numpy as np

from . import kitti_io

TILE = 64                                # points per tile of the device passes (one wave)
MAX_IO_WORKERS = 16


def cum(a):
    """counts -> offsets (len + 1) int64"""
    return np.concatenate([[0], np.cumsum(a)]).astype(np.int64)


def as_calib(c, cls=kitti_io.Calibration, make=None):
    """A ``cls`` as it is; anything else (a calib file path, the file's dict) through ``make``, by default ``cls`` itself"""
    return c if isinstance(c, cls) else (make or cls)(c)


def check_device(device):
    if str(device) != "cpu" and not str(device).startswith("cuda"):
        raise ValueError("device must be 'cpu' or 'cuda[:i]'")


def to_device(device):
    """-> the upload of a host array (made contiguous) to ``device``"""
    import torch
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)


def upload_arrays(arrays, device):
    """Host arrays -> one pinned buffer, ONE asynchronous copy -> (the device buffer, the arrays' device addresses)"""
    import torch
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 255) // 256 * 256
    host = torch.empty(max(total, 256), dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    for a, o in zip(arrays, offs):
        view[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf = host.to(device, non_blocking=True)
    return buf, [buf.data_ptr() + o for o in offs]


def pack_scenes(clouds, n_boxes, calibs=None, shapes=None):
    """Scenes back to back.  clouds: per scene (n, 4) f32; n_boxes: boxes per scene -> n, nt (tiles), nb, their offsets pt_off,
    tile_off, box_off (int64; the kernels read them as int32), velo (sum n, 4) (one zero row when there is no point), max_tiles
    and, with ``calibs`` (kitti_io.Calibration), calib (S, PRCNN_CALIB_ROW) f32 = DeviceInputStage.pack_calib with the image ``shapes``, or
    without them (S, 12) f32 = the lidar -> rect matrix np.dot(V2C.T, R0.T)."""
    p = types.SimpleNamespace()
    p.n = np.array([len(c) for c in clouds], dtype=np.int64)
    p.nt = (p.n + TILE - 1) // TILE
    p.nb = np.array(list(n_boxes), dtype=np.int64)
    p.pt_off, p.tile_off, p.box_off = cum(p.n), cum(p.nt), cum(p.nb)
    p.max_tiles = int(p.nt.max()) if len(p.n) else 0
    p.velo = np.concatenate(list(clouds)) if p.pt_off[-1] else np.zeros((1, 4), np.float32)
    if calibs is not None and shapes is not None:
        p.calib = np.stack([kitti_io.DeviceInputStage.pack_calib(c, s) for c, s in zip(calibs, shapes)]).astype(np.float32)
    elif calibs is not None:
        p.calib = np.stack([np.dot(c.V2C.T, c.R0.T).astype(np.float32).reshape(12) for c in calibs])
    return p


def offsets_to_device(p, dev):
    """-> pt_off, tile_off, box_off as the kernels read them (int32)"""
    return [dev(a.astype(np.int32)) for a in (p.pt_off, p.tile_off, p.box_off)]


def valid_points(pts, calib, img_shape, scope, is_rect=False, reduce=True):
    """The loaders' filter (generate_aug_scene.py:241-249, kitti_rcnn_dataset.py:251-274) -> (pts_rect (m, 3) f32, intensity (m,) f32)
    of the points in the image, at depth >= 0 and (``reduce``) inside ``scope``, compared as float64.  ``is_rect``: the rows are
    in the rect frame already (a pre-made aug scene)."""
    pts_rect = pts[:, 0:3] if is_rect else calib.lidar_to_rect(pts[:, 0:3])
    pts_img, depth = calib.rect_to_img(pts_rect)
    flag = np.logical_and(np.logical_and(pts_img[:, 0] >= 0, pts_img[:, 0] < img_shape[1]),
                          np.logical_and(pts_img[:, 1] >= 0, pts_img[:, 1] < img_shape[0]))
    flag = np.logical_and(flag, depth >= 0)
    if reduce:
        x, y, z = (pts_rect[:, k].astype(np.float64) for k in range(3))
        (x0, x1), (y0, y1), (z0, z1) = np.asarray(scope, dtype=np.float64).reshape(3, 2)
        flag = flag & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1) & (z >= z0) & (z <= z1)
    return pts_rect[flag][:, 0:3], pts[:, 3][flag]


def check_pc_range(xyz, scope):
    (x0, x1), (y0, y1), (z0, z1) = scope
    return bool((x0 <= float(xyz[0]) <= x1) and (y0 <= float(xyz[1]) <= y1) and (z0 <= float(xyz[2]) <= z1))


def boxes_of_labels(objs, positions=None):
    """Label objects -> (g, 7) f32 [x, y_bottom, z, h, w, l, ry]; ``positions`` stand in for the objects' own ``t``"""
    boxes = np.zeros((len(objs), 7), dtype=np.float32)
    for k, o in enumerate(objs):
        boxes[k, 0:3], boxes[k, 3], boxes[k, 4], boxes[k, 5], boxes[k, 6] = o.t if positions is None else positions[k], o.h, o.w, o.l, o.ry
    return boxes


def enlarged(boxes):
    """(7,) or (g, 7) boxes with w + 0.5, l + 0.5 in their own dtype, as ``cur_gt_boxes3d[:, 4:6] += 0.5``"""
    big = boxes.copy()
    big[..., 4] += 0.5
    big[..., 5] += 0.5
    return big


def place_on_plane(box, plane):
    """A database box (7,) f32 put on the road plane (f64) -> (box (7,) f32, move_height f64)"""
    a, b, c, d = plane
    box = box.copy()
    cur_height = (-d - a * box[0] - c * box[2]) / b
    move = np.float64(box[1]) - cur_height
    box[1] = np.float32(np.float64(box[1]) - move)
    return box, np.float64(move)


def database_rows(db):
    """A GT database -> (rows (sum n, 4) f32 = x, y, z, intensity of all entries back to back, counts, offsets)"""
    rows = [np.concatenate((np.asarray(e["points"], np.float32).reshape(-1, 3), np.asarray(e["intensity"], np.float32).reshape(-1, 1)), 1)
            for e in db]
    counts = np.array([len(e["points"]) for e in db], dtype=np.int64)
    return (np.ascontiguousarray(np.concatenate(rows, 0), dtype=np.float32) if rows else np.zeros((0, 4), np.float32)), counts, cum(counts)


def no_label_error(who, sample_id):
    return ValueError("%s: sample %06d has no label besides DontCare: the overlap test has nothing to compare with "
                      "(the reference raises here)" % (who, sample_id))


def class_whitelist(classes, include_similar=False, sitting_with=("Pedestrian",)):
    """The class names a loader keeps: ``classes``, with ``include_similar`` also Van beside Car and Person_sitting beside any of
    ``sitting_with``"""
    white = list(classes)
    if include_similar:
        if "Car" in classes:
            white.append("Van")
        if any(c in classes for c in sitting_with):
            white.append("Person_sitting")
    return white


def sample_list_file(root, split="train", subsample=-1, shuffle_subsample=None):
    """The file sample_id_list reads: ImageSets/<split>.txt, or with ``subsample > 0`` on ``train`` train_car1.txt (car_split.py writes
    it) or train_car1_<shuffle_subsample>.txt"""
    sets = os.path.join(root, "KITTI", "ImageSets")
    if subsample > 0 and split == "train":
        return os.path.join(sets, "train_car1.txt" if shuffle_subsample is None else "train_car1_{}.txt".format(shuffle_subsample))
    return os.path.join(sets, split + ".txt")


def sample_id_list(root, split="train", subsample=-1, shuffle_subsample=None):
    """kitti_dataset.py:18-33.  With ``subsample > 0`` on ``train`` the list is train_car1.txt, or train_car1_<shuffle_subsample>.txt,
    cut to the first ``subsample`` ids.  A missing train_car1_<shuffle_subsample>.txt is written from an UNSEEDED random.shuffle of
    train_car1.txt, as the reference does: its order is not reproducible (keep the file to keep the list)."""
    path = sample_list_file(root, split, subsample, shuffle_subsample)
    if subsample > 0 and split == "train":
        if shuffle_subsample is not None and not os.path.isfile(path):
            with open(sample_list_file(root, split, subsample)) as f:
                temp = [x.strip() for x in f.readlines()]
            random.shuffle(temp)
            with open(path, "w") as f:
                for item in temp:
                    f.write("{}\n".format(item))
        with open(path) as f:
            return [x.strip() for x in f.readlines()][:subsample]
    with open(path) as f:
        return [x.strip() for x in f.readlines()]
