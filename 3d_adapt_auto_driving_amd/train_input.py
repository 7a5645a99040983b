"""The RPN training input stage (reference: lib/datasets/kitti_rcnn_dataset.py get_rpn_sample in TRAIN mode, with
apply_gt_aug_to_one_scene, the near / far sampler, data_augmentation (stage 1), generate_rpn_training_labels and collate_batch): a
KITTI-format tree plus a GT database (gt_database.py) -> RPN training batches.  No loss, no optimizer, no backward pass.

  src = RpnTrainInput(root, cfg, gt_database_dir, split="train", classes="Car", npoints=16384, npoints_faraway=4000,
                      with_replace=False, seed=None, device="cuda", subsample=-1, shuffle_subsample=None, sample_ids=None,
                      obj_scale=None, obj_scale_prob=1.0)
  len(src)                    the reference's sample_id_list after preprocess_rpn_training_data
                              (the list is scene_batch.sample_id_list's: with ``subsample > 0`` on ``train`` the first ``subsample``
                              ids of train_car1.txt or train_car1_<shuffle_subsample>.txt; ``sample_ids``, an explicit list, replaces
                              the read -- what the ranks of a process group are handed; the object filter follows either)
  batch = src.batch(indices)  the dict collate_batch returns for [dataset[i] for i in indices]

``device="cuda"`` runs csrc/train_input.hip and csrc/rpn_labels.hip; the per-point entries are device tensors and never visit the host.
``device="cpu"`` follows the reference try by try in numpy and returns numpy arrays: it is the checker, not a second product path.

Command line:
  python -m 3d_adapt_auto_driving_amd.train_input --root R --gt_database_dir DB.pkl [--class_name Car] [--split train] [--npoints N]
         [--batch_size B] [--epochs E] [--device cuda|cpu] [--save_dir D] [--cfg_file F] [--seed S] [--subsample N]
         [--shuffle_subsample S] [--obj_scale LO HI [--obj_scale_prob P]]
walks the split in order and prints scenes/s; with --save_dir one ``batch_%06d.npz`` per batch is written.

The random stream.  The target is ONE process calling ``dataset[i]`` in order (num_workers=0); the reference's global np.random is a
legacy RandomState the object owns.  Per sample the draws are: ``rand() < GT_AUG_APPLY_PROB``; ``randint(10, GT_EXTRA_NUM)`` (or the
constant); per try ``rand()`` against GT_AUG_HARD_RATIO and a ``randint`` into the easy / hard list (split at 100 points), or one
``randint`` when the ratio is 0; the sampler's ``choice`` / ``shuffle``; ``1 - rand(3)``, ``uniform`` (angle), ``uniform`` (scale).  No
GT-aug draw depends on a geometric result: the exits of a try (range check, fewer than 5 points, cnt > extra_gt_num) look at the
database entry only, so the host replays the tries and hands the device the ordered list of at most GT_EXTRA_NUM + 1 (<= 16)
candidates, already on the road plane in f64.  The sampler's draws need only the counts of the new cloud (kept points, near kept
points, the accepted objects): they are drawn as ranks into the near list and the far list, and the device maps rank to row.  The
NUMBER of the sampler's draws depends on those counts and the GT-aug draws of the next sample follow them in the stream, so the device
path reads its few ints scene by scene (B small reads per batch); the output rows and the labels of the batch are one launch group.

Random object scaling (``obj_scale=(lo, hi)``, object_scale.py).  After everything above, per sample in batch order and with g final gt
boxes (class-filtered labels, then accepted database objects): ``u = ros_rng.rand(g)``, ``rr = ros_rng.uniform(lo, hi, g)`` (both always
drawn), ``factor = where(u < obj_scale_prob, rr, 1.0)``; object_scale.scale_objects then rescales the emitted pts_rect (and pts_input) and
the final boxes, and rpn_labels and gt_boxes3d see the scaled points and boxes.  ``ros_rng`` is a RandomState of its own
(``RandomState(None)`` when seed is None, else ``RandomState((seed + 20200519) % 2**32)``): the legacy stream above is never touched by the
option, so everything it decides (GT-aug, sampler, augmentation) is the same with and without it.  On the device path it is one launch
for the batch behind prcnn_train_emit and one read of the hit counts; ``last_scaled`` lists (sample id, box index, factor, hits) of the
last batch().

The in-place drift.  The reference does not copy ``new_gt_obj``: ``obj.pos[1] -= move_height`` accumulates on the database entry
with every try that reaches the overlap test (accepted or not), and the label box of a pasted object is built later from ``obj.pos`` by
objs_to_boxes3d, not from the placed box.  Reproduced: the object keeps its own f32 copy of every entry's pos and shifts it.

The overlap rule is kitti_utils.get_iou3d on the f32 corner arrays (not the offline tool's): height overlap from the corner means, BEV
polygon intersection (here: an f64 clip of convex quadrilaterals, quad_intersection_area, the same operations on host and device), the
union from the two volume terms, accepted when the f32 maximum over the scene's non-DontCare boxes (w, l + 0.5) and all earlier
accepted candidates (w, l + 0.5) is < 1e-8.  The argument for agreeing with shapely: a decision can differ only where the two clips
disagree about an area of the order of 1e-8 of the boxes, i.e. for pairs that touch within rounding; tests/golden g20 (the reference's
run over a stand-in for shapely) is kept out of 0 < IoU < 1e-3 and agrees in every decision.
"""
import argparse
import ctypes as C
import os
import time

import numpy as np

from . import _lib, kitti_io, kitti_utils
from .aug_scene import road_plane
from .gt_database import box_trig, class_tuple, load_gt_database
from .kitti_io import Object3d, png_size
from .scene_batch import (TILE, boxes_of_labels, check_device, check_pc_range, class_whitelist, cum, database_rows, enlarged,  # noqa: F401
                          no_label_error, offsets_to_device, pack_scenes, place_on_plane, sample_id_list, to_device, valid_points)

MAX_CAND = 16                      # csrc/placement.hpp PLACE_MAX_CAND = prcnn_aug_max_candidates()
TRY_TIMES = 100
HARD_POINTS = 100                  # an entry with more points is "easy"
NEAR_DEPTH = 40.0
AUG_ID_BASE = 200000               # sample ids from here on are pre-made aug scenes (rectified_data)
AUG_LABEL_BASE = 2000000           # sic: get_label reads label_2 below this id
ROS_SEED_OFFSET = 20200519         # object scaling's RandomState is seeded (seed + this) % 2**32
AUG_DIRS = {"Car": "aug_scene", "Pedestrian": "aug_scene_ped", "Cyclist": "aug_scene_cyclist"}
DEFAULTS = {"AUG_DATA": True, "AUG_METHOD_LIST": ["rotation", "scaling", "flip"], "SCALE_MIN_MAX_RANGE": [0.95, 1.05],
            "AUG_METHOD_PROB": [0.5, 0.5, 0.5], "AUG_ROT_RANGE": 18, "GT_AUG_ENABLED": False, "GT_EXTRA_NUM": 15,
            "GT_AUG_RAND_NUM": False, "GT_AUG_APPLY_PROB": 0.75, "GT_AUG_HARD_RATIO": 0.6, "PC_REDUCE_BY_RANGE": True,
            "INCLUDE_SIMILAR_TYPE": False}                                   # lib/config.py's values for the keys config.py lacks
KIND_KEPT, KIND_NEAR, KIND_FAR, KIND_DB = _lib.PRCNN_TR_KEPT, _lib.PRCNN_TR_NEAR, _lib.PRCNN_TR_FAR, _lib.PRCNN_TR_DB   # emit codes:
KIND_SHIFT, SLOT_SHIFT, REC = _lib.PRCNN_TR_KIND_SHIFT, _lib.PRCNN_TR_SLOT_SHIFT, _lib.PRCNN_TR_REC    # kind | slot | value; record doubles


def _opt(cfg, name):
    return cfg[name] if name in cfg else DEFAULTS[name]


# ------------------------------------------------------------------------------------------------------------------ overlap rule
def quad_area(q):
    """(4, 2) f64 ring -> area (shoelace, summed in ring order)"""
    s = 0.0
    for i in range(4):
        j = (i + 1) & 3
        s = s + (float(q[i][0]) * float(q[j][1]) - float(q[j][0]) * float(q[i][1]))
    return 0.5 * abs(s)


def quad_intersection_area(A, B):
    """Area of the intersection of two convex quadrilaterals ((4, 2) f64 rings, either orientation): A clipped by the four edges of
    B (Sutherland-Hodgman) in f64; csrc/train_input.hip tr_quad_clip_area is the same operations in the same order."""
    px, pz = [float(A[i][0]) for i in range(4)], [float(A[i][1]) for i in range(4)]
    bx, bz = [float(B[i][0]) for i in range(4)], [float(B[i][1]) for i in range(4)]
    sb = 0.0
    for i in range(4):
        j = (i + 1) & 3
        sb = sb + (bx[i] * bz[j] - bx[j] * bz[i])
    sign = 1.0 if sb >= 0.0 else -1.0
    for e in range(4):
        if not px:
            break
        f = (e + 1) & 3
        ax, az = bx[e], bz[e]
        ex, ez = bx[f] - ax, bz[f] - az
        qx, qz = [], []
        n = len(px)
        for i in range(n):
            k = 0 if i + 1 == n else i + 1
            cx, cz, nx, nz = px[i], pz[i], px[k], pz[k]
            dc = sign * (ex * (cz - az) - ez * (cx - ax))
            dn = sign * (ex * (nz - az) - ez * (nx - ax))
            ic, inn = dc >= 0.0, dn >= 0.0
            if ic and len(qx) < 9:
                qx.append(cx)
                qz.append(cz)
            if ic != inn and len(qx) < 9:
                t = dc / (dc - dn)
                qx.append(cx + t * (nx - cx))
                qz.append(cz + t * (nz - cz))
        px, pz = qx, qz
    n = len(px)
    if n < 3:
        return 0.0
    s = 0.0
    for i in range(n):
        k = 0 if i + 1 == n else i + 1
        s = s + (px[i] * pz[k] - px[k] * pz[i])
    return 0.5 * abs(s)


def overlap_records(boxes):
    """(k, 7) f32 boxes (already enlarged) -> (k, REC) f64: what get_iou3d reads of boxes3d_to_corners3d(boxes): the four BEV corners
    (x, z) of the bottom face, min_h, max_h (f32 corner means) and area * (max_h - min_h) as the reference's numpy rounds it (a Python
    float times an f32 scalar: f32)."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 7)
    rec = np.zeros((boxes.shape[0], REC), dtype=np.float64)
    if boxes.shape[0] == 0:
        return rec
    corners = kitti_utils.boxes3d_to_corners3d(boxes)
    min_h = -corners[:, 0:4, 1].sum(axis=1) / 4.0
    max_h = -corners[:, 4:8, 1].sum(axis=1) / 4.0
    quad = corners[:, 0:4][:, :, [0, 2]].astype(np.float64)
    rec[:, 0:8] = quad.reshape(-1, 8)
    rec[:, 8], rec[:, 9] = min_h, max_h
    for k in range(boxes.shape[0]):
        rec[k, 10] = np.float32(quad_area(quad[k])) * np.float32(max_h[k] - min_h[k])
    return rec


def record_iou3d(a, b):
    """get_iou3d's entry for (new box a, present box b) from their records -> f32"""
    f32 = np.float32
    hov = f32(min(f32(a[9]), f32(b[9]))) - f32(max(f32(a[8]), f32(b[8])))
    if hov <= 0:
        return f32(0.0)
    o3 = quad_intersection_area(a[0:8].reshape(4, 2), b[0:8].reshape(4, 2)) * float(hov)
    un = float(f32(a[10]) + f32(b[10])) - o3
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(np.float64(o3) / np.float64(un))


# ------------------------------------------------------------------------------------------------------------------- the sampler
def sample_choice(rng, near_ids, far_ids, npoints, npoints_faraway, with_replace):
    """kitti_rcnn_dataset.py:289-321 over the near and far lists of the new cloud (``near_ids`` / ``far_ids``: what stands for a
    point -- its index on the host path, its code on the device path; the draws need only the lengths)."""
    n = len(near_ids) + len(far_ids)
    if npoints < n:
        far = far_ids
        if len(far) > npoints_faraway:
            far = rng.choice(far, npoints_faraway, replace=False)
        if len(near_ids) < npoints - len(far):
            near = rng.choice(near_ids, npoints - len(far), replace=True)
        else:
            near = rng.choice(near_ids, npoints - len(far), replace=with_replace)
        choice = np.concatenate((near, far), axis=0) if len(far) > 0 else near
        rng.shuffle(choice)
        return choice
    return None


def sample_choice_all(rng, all_ids, npoints):
    """... :310-321: the cloud has at most npoints points"""
    choice = all_ids
    n = len(all_ids)
    if npoints > n:
        extra = rng.choice(choice, npoints - n, replace=n < npoints - n)
        choice = np.concatenate((choice, extra), axis=0)
    rng.shuffle(choice)
    return choice


# ------------------------------------------------------------------------------------------------------------- box augmentation
def draw_augmentation(rng, cfg):
    """data_augmentation's draws -> (angle | None, scale | None, flip, aug_method)"""
    aug_list, prob = _opt(cfg, "AUG_METHOD_LIST"), _opt(cfg, "AUG_METHOD_PROB")
    enable = 1 - rng.rand(3)
    angle = scale = None
    method = []
    if "rotation" in aug_list and enable[0] < prob[0]:
        rot = _opt(cfg, "AUG_ROT_RANGE")
        angle = rng.uniform(-np.pi / rot, np.pi / rot)
        method.append(["rotation", angle])
    if "scaling" in aug_list and enable[1] < prob[1]:
        lo, hi = _opt(cfg, "SCALE_MIN_MAX_RANGE")
        scale = rng.uniform(lo, hi)
        method.append(["scaling", scale])
    flip = "flip" in aug_list and bool(enable[2] < prob[2])
    if flip:
        method.append("flip")
    return angle, scale, flip, method


def augment_boxes(boxes, alpha, angle, scale, flip):
    """data_augmentation (stage 1) of the boxes, in numpy as the reference writes it (their f32 arctan2 bits are numpy's)"""
    boxes = boxes.copy()
    if angle is not None:
        boxes = kitti_utils.rotate_pc_along_y(boxes, rot_angle=angle)
        x, z = boxes[:, 0], boxes[:, 2]
        beta = np.arctan2(z, x)
        boxes[:, 6] = np.sign(beta) * np.pi / 2 + alpha - beta
    if scale is not None:
        boxes[:, 0:6] = boxes[:, 0:6] * scale
    if flip:
        boxes[:, 0] = -boxes[:, 0]
        boxes[:, 6] = np.sign(boxes[:, 6]) * np.pi - boxes[:, 6]
    return boxes


def augment_points(pts, angle, scale, flip):
    pts = pts.copy()
    if angle is not None:
        pts = kitti_utils.rotate_pc_along_y(pts, rot_angle=angle)
    if scale is not None:
        pts = pts * scale
    if flip:
        pts[:, 0] = -pts[:, 0]
    return pts


def rotation_terms(angle):
    """rotmat.T of rotate_pc_along_y as (m00, m10, m01, m11): x' = x m00 + z m10, z' = x m01 + z m11"""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, -s], [s, c]])
    t = np.transpose(rot)
    return float(t[0, 0]), float(t[1, 0]), float(t[0, 1]), float(t[1, 1])


def check_obj_scale(obj_scale, prob):
    """-> ((lo, hi) | None, probability) of random object scaling; ValueError for a range or a probability that makes no sense"""
    prob = float(prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError("train_input: obj_scale_prob must lie in [0, 1], got %r" % prob)
    if obj_scale is None:
        return None, prob
    lo, hi = (float(v) for v in obj_scale)
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("train_input: obj_scale must be (lo, hi) with 0 < lo <= hi, got (%r, %r)" % (lo, hi))
    return (lo, hi), prob


_TrainBatch = _lib.struct("prcnn_train_batch")


class RpnTrainInput:
    def __init__(self, root, cfg, gt_database_dir=None, split="train", classes="Car", npoints=16384, npoints_faraway=4000,
                 with_replace=False, seed=None, device="cuda", subsample=-1, shuffle_subsample=None, sample_ids=None, obj_scale=None,
                 obj_scale_prob=1.0):
        check_device(device)
        self.obj_scale, self.obj_scale_prob = check_obj_scale(obj_scale, obj_scale_prob)
        self.root, self.cfg, self.split, self.device = root, cfg, split, str(device)
        self.classes = class_tuple(classes)
        self.npoints, self.npoints_faraway, self.with_replace = int(npoints), int(npoints_faraway), bool(with_replace)
        self.rng = np.random.RandomState(seed)
        self.ros_rng = np.random.RandomState(None if seed is None else (int(seed) + ROS_SEED_OFFSET) % 2 ** 32)   # object scaling's own stream
        self.last_scaled = []                                 # the last batch(): (sample id, box index, factor, hits) per final gt box
        self.stats = {"draw_seconds": 0.0}
        self.decisions = []                                   # device="cpu": (sample id, database entry, accepted, max iou) per test
        self.last_kept = []                                   # the last batch(): (sample id, scene points left after the removal)
        self.base = os.path.join(root, "KITTI", "object", "testing" if split == "test" else "training")
        aug_root = os.path.join(root, "KITTI", AUG_DIRS.get(classes, "aug_scene"), "training")
        self.aug_pts_dir = os.path.join(aug_root, "rectified_data")
        self.aug_label_dir = os.path.join(aug_root, "aug_label")
        self.scope = np.asarray(cfg.PC_AREA_SCOPE, dtype=np.float64).reshape(3, 2)
        self.reduce = bool(_opt(cfg, "PC_REDUCE_BY_RANGE"))
        if sample_ids is None:                                # kitti_dataset.py:18-33, the few-shot cut included
            sample_ids = sample_id_list(root, split, subsample, shuffle_subsample)
        self.listed_ids = [int(x) for x in sample_ids]        # before the object filter
        self.sample_id_list = [i for i in self.listed_ids if len(self.filtrate_objects(self.labels(i))) > 0]
        self.gt_aug = bool(_opt(cfg, "GT_AUG_ENABLED"))
        self.hard_ratio = float(_opt(cfg, "GT_AUG_HARD_RATIO"))
        self.db = None
        if gt_database_dir is not None:
            db = load_gt_database(gt_database_dir) if isinstance(gt_database_dir, str) else list(gt_database_dir)
            self._set_database(db)
        if self.gt_aug and self.db is None:
            raise ValueError("train_input: cfg.GT_AUG_ENABLED needs a GT database")

    def __len__(self):
        return len(self.sample_id_list)

    # ------------------------------------------------------------------------------------------------------------------ database
    def _set_database(self, db):
        self.db = db
        self.db_box = [np.asarray(e["gt_box3d"], dtype=np.float32).copy() for e in db]
        self.db_pos = [np.array(e["obj"].pos, dtype=np.float32) for e in db]            # the drifting copy (see the docstring)
        self.db_rows, self.db_n, self.db_off = database_rows(db)
        if self.hard_ratio > 0:
            self.easy = [k for k in range(len(db)) if self.db_n[k] > HARD_POINTS]
            self.hard = [k for k in range(len(db)) if self.db_n[k] <= HARD_POINTS]
        if self.device != "cpu":
            import torch
            if _lib.call("prcnn_aug_max_candidates") != MAX_CAND:
                raise _lib.PrcnnError("train_input: MAX_CAND differs from the library's")
            self.t_db = torch.from_numpy(self.db_rows if len(self.db_rows) else np.zeros((1, 4), np.float32)).to(self.device)
            self.db_trig = box_trig(np.stack(self.db_box)) if db else np.zeros((0, 2), np.float32)

    def generator_state(self):
        return self.rng.get_state()

    def scale_generator_state(self):
        return self.ros_rng.get_state()

    def _draw_factors(self, g):
        """object scaling's draws for a sample with g final gt boxes -> (g,) f64"""
        u = self.ros_rng.rand(g)
        rr = self.ros_rng.uniform(self.obj_scale[0], self.obj_scale[1], g)
        return np.where(u < self.obj_scale_prob, rr, 1.0)

    # --------------------------------------------------------------------------------------------------------------- front half
    def labels(self, sample_id):
        d = os.path.join(self.base, "label_2") if sample_id < AUG_LABEL_BASE else self.aug_label_dir
        with open(os.path.join(d, "%06d.txt" % sample_id)) as f:
            return [Object3d(line) for line in f.readlines()]

    def filtrate_objects(self, objs):
        white = class_whitelist(self.classes, _opt(self.cfg, "INCLUDE_SIMILAR_TYPE"))
        return [o for o in objs if o.cls_type in white and not (self.reduce and not check_pc_range(o.t, self.scope))]

    def load_scene(self, sample_id):
        """-> dict: pts (n, 4) f32 (raw velodyne rows, or rect rows for a pre-made aug scene), is_rect, calib, shape, all_boxes (the
        non-DontCare labels), objs (the class-filtered labels), plane"""
        base_id = sample_id % AUG_ID_BASE
        calib = kitti_io.Calibration(os.path.join(self.base, "calib", "%06d.txt" % base_id))
        width, height = png_size(os.path.join(self.base, "image_2", "%06d.png" % base_id))
        if sample_id < AUG_ID_BASE:
            pts = np.fromfile(os.path.join(self.base, "velodyne", "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
        else:
            pts = np.fromfile(os.path.join(self.aug_pts_dir, "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
        objs = self.labels(sample_id)
        every = [o for o in objs if o.cls_type != "DontCare"]
        plane = road_plane(os.path.join(self.base, "planes", "%06d.txt" % base_id)) if self.gt_aug else None
        return {"id": sample_id, "pts": np.ascontiguousarray(pts), "is_rect": sample_id >= AUG_ID_BASE, "calib": calib,
                "shape": (int(height), int(width), 3), "all_boxes": boxes_of_labels(every),
                "objs": self.filtrate_objects(objs), "plane": plane}

    def valid_points(self, sc):
        """get_rpn_sample :251-274 in numpy -> (pts_rect (m, 3) f32, intensity (m,) f32)"""
        return valid_points(sc["pts"], sc["calib"], sc["shape"], self.scope, sc["is_rect"], self.reduce)

    # ------------------------------------------------------------------------------------------------------------ GT-aug: draws
    def _draw_entry(self):
        rng = self.rng
        if self.hard_ratio > 0:
            p = rng.rand()
            pool = self.easy if p > self.hard_ratio else self.hard
            return pool[rng.randint(0, len(pool))]
        return int(rng.randint(0, len(self.db)))

    def _tries(self, plane):
        """The loop of apply_gt_aug_to_one_scene as a generator: yields (entry, placed box (7,) f32, move_height f64) for every try
        that reaches the overlap test, after shifting the entry's drifting pos."""
        cfg = self.cfg
        extra = self.rng.randint(10, _opt(cfg, "GT_EXTRA_NUM")) if _opt(cfg, "GT_AUG_RAND_NUM") else _opt(cfg, "GT_EXTRA_NUM")
        cnt = 0
        for _ in range(TRY_TIMES):
            if cnt > extra:
                break
            k = self._draw_entry()
            if self.reduce and not check_pc_range(self.db_box[k][0:3], self.scope):
                continue
            if self.db_n[k] < 5:
                continue
            box, move = place_on_plane(self.db_box[k], plane)
            self.db_pos[k][1] = np.float32(np.float64(self.db_pos[k][1]) - move)
            cnt += 1
            yield k, box, move

    def replay_candidates(self, plane):
        """The draws of one apply_gt_aug_to_one_scene call -> [(entry, box, move)] in try order (the host replay)"""
        out = list(self._tries(plane))
        if len(out) > MAX_CAND:
            raise ValueError("train_input: %d candidates reach the overlap test in one scene; the device code holds %d "
                             "(GT_EXTRA_NUM + 1 must be <= %d)" % (len(out), MAX_CAND, MAX_CAND))
        return out

    # --------------------------------------------------------------------------------------------------------------- labels out
    def _gt_of(self, sc, accepted):
        """-> (gt_boxes3d (g, 7) f32, gt_alpha (g,) f32) of the class-filtered labels and the accepted entries (their DRIFTED pos)"""
        objs = list(sc["objs"]) + [self.db[k]["obj"] for k in accepted]
        boxes = boxes_of_labels(objs, [o.t for o in sc["objs"]] + [self.db_pos[k] for k in accepted])
        alpha = np.zeros(len(objs), dtype=np.float32)
        for i, o in enumerate(objs):
            alpha[i] = o.alpha
        return boxes, alpha

    # ----------------------------------------------------------------------------------------------------------------- cpu path
    def _sample_cpu(self, sample_id):
        import torch
        from . import roipool3d_utils, rpn_eval
        cfg, rng = self.cfg, self.rng
        sc = self.load_scene(sample_id)
        pts_rect, inten = self.valid_points(sc)
        accepted, n_scene = [], pts_rect.shape[0]
        if self.gt_aug and rng.rand() < _opt(cfg, "GT_AUG_APPLY_PROB"):
            cur = overlap_records(enlarged(sc["all_boxes"]))
            flag = np.ones(pts_rect.shape[0], dtype=np.int32)
            new_pts, new_int = [], []
            for k, box, move in self._tries(sc["plane"]):
                rec = overlap_records(enlarged(box).reshape(1, 7))[0]
                if cur.shape[0] == 0:
                    raise no_label_error("train_input", sc["id"])
                iou = np.array([record_iou3d(rec, r) for r in cur], dtype=np.float32)
                ok = bool(iou.max() < 1e-8)
                self.decisions.append((sample_id, int(k), ok, float(iou.max())))
                if not ok:
                    continue
                big = box.copy()
                big[3] += 2
                mask = roipool3d_utils.pts_in_boxes3d_cpu(torch.from_numpy(np.ascontiguousarray(pts_rect)),
                                                          torch.from_numpy(big.reshape(1, 7)))[0].numpy()
                flag[mask == 1] = 0
                p = np.asarray(self.db[k]["points"], dtype=np.float32).copy()
                p[:, 1] = (p[:, 1].astype(np.float64) - move).astype(np.float32)
                new_pts.append(p)
                new_int.append(np.asarray(self.db[k]["intensity"], dtype=np.float32))
                cur = np.concatenate((cur, rec.reshape(1, REC)), axis=0)
                accepted.append(k)
            if accepted:
                n_scene = int((flag == 1).sum())
                pts_rect = np.concatenate([pts_rect[flag == 1]] + new_pts, axis=0)
                inten = np.concatenate([inten[flag == 1]] + new_int, axis=0)
        self.last_kept.append((sample_id, n_scene))
        t0 = time.perf_counter()
        near = pts_rect[:, 2] < NEAR_DEPTH
        if self.npoints < len(pts_rect):
            choice = sample_choice(rng, np.where(near == 1)[0], np.where(near == 0)[0], self.npoints, self.npoints_faraway,
                                   self.with_replace)
        else:
            choice = sample_choice_all(rng, np.arange(0, len(pts_rect), dtype=np.int32), self.npoints)
        ret_pts = pts_rect[choice, :]
        feat = (inten[choice] - 0.5).reshape(-1, 1)
        gt, alpha = self._gt_of(sc, accepted)
        info = {"sample_id": sample_id, "random_select": True}
        aug_pts, aug_gt = ret_pts.copy(), gt.copy()
        if _opt(cfg, "AUG_DATA"):
            angle, scale, flip, method = draw_augmentation(rng, cfg)
            aug_pts = augment_points(aug_pts, angle, scale, flip)
            aug_gt = augment_boxes(aug_gt, alpha, angle, scale, flip)
            info["aug_method"] = method
        self.stats["draw_seconds"] += time.perf_counter() - t0
        if self.obj_scale is not None:
            from . import object_scale
            factors = self._draw_factors(aug_gt.shape[0])
            p2, g2, hits = object_scale.scale_objects(aug_pts[None], aug_gt[None], [aug_gt.shape[0]], factors[None], device="cpu")
            aug_pts, aug_gt = p2[0], g2[0]
            self.last_scaled += [(sample_id, k, float(factors[k]), int(hits[0, k])) for k in range(len(factors))]
        info["pts_input"] = np.concatenate((aug_pts, feat), axis=1) if cfg.RPN.USE_INTENSITY else aug_pts
        info["pts_rect"], info["pts_features"] = aug_pts, feat
        if not cfg.RPN.FIXED:
            cls, reg = rpn_eval.rpn_labels(aug_pts[None], aug_gt[None], [aug_gt.shape[0]], device="cpu")
            info["rpn_cls_label"], info["rpn_reg_label"] = cls[0], reg[0]
        info["gt_boxes3d"] = aug_gt
        return info

    @staticmethod
    def collate(samples):
        """collate_batch (kitti_rcnn_dataset.py:1125-1158) for numpy samples"""
        out = {}
        for key in samples[0]:
            vals = [s[key] for s in samples]
            if key == "gt_boxes3d":
                g = max(len(v) for v in vals)
                arr = np.zeros((len(vals), g, 7), dtype=np.float32)
                for i, v in enumerate(vals):
                    arr[i, :len(v)] = v
                out[key] = arr
            elif isinstance(vals[0], np.ndarray):
                out[key] = np.concatenate([v[np.newaxis, ...] for v in vals], axis=0)
            elif isinstance(vals[0], int):                  # a bool is an int: random_select becomes an i32 array too
                out[key] = np.array(vals, dtype=np.int32)
            else:
                out[key] = vals
        return out

    # -------------------------------------------------------------------------------------------------------------- device path
    def _batch_device(self, ids):
        import torch
        from . import rpn_eval
        cfg, rng, device = self.cfg, self.rng, self.device
        S, NP = len(ids), self.npoints
        scenes = [self.load_scene(i) for i in ids]
        pk = pack_scenes([sc["pts"] for sc in scenes], [len(sc["all_boxes"]) for sc in scenes], [sc["calib"] for sc in scenes],
                         [sc["shape"] for sc in scenes])
        nt, nb, tile_off, total = pk.nt, pk.nb, pk.tile_off, int(pk.pt_off[-1])
        if total >= 2 ** 31 - 64 or S * NP >= 2 ** 40:
            raise ValueError("train_input batch too large: split it")
        box_rec = [overlap_records(enlarged(sc["all_boxes"])) for sc in scenes]
        box_rec = np.concatenate(box_rec) if pk.box_off[-1] else np.zeros((1, REC), np.float64)
        is_rect = np.array([sc["is_rect"] for sc in scenes], dtype=np.uint8)
        dev = to_device(device)
        t_in = offsets_to_device(pk, dev) + [dev(a) for a in (pk.velo, pk.calib, self.scope.reshape(6), is_rect, box_rec)]
        t_cn = torch.zeros((S,), dtype=torch.int32, device=device)
        t_crec = torch.zeros((S, MAX_CAND, REC), dtype=torch.float64, device=device)
        t_cbox = torch.zeros((S, MAX_CAND, 7), dtype=torch.float32, device=device)
        t_ctrig = torch.zeros((S, MAX_CAND, 2), dtype=torch.float32, device=device)
        t_cmove = torch.zeros((S, MAX_CAND), dtype=torch.float64, device=device)
        m = max(1, total)
        t_rect = torch.empty((m, 4), dtype=torch.float32, device=device)
        t_valid = torch.empty((m,), dtype=torch.uint8, device=device)
        t_flag = torch.empty((m,), dtype=torch.uint8, device=device)
        t_cnt = torch.empty((max(1, 2 * int(tile_off[-1])),), dtype=torch.int32, device=device)
        t_lists = torch.empty((3, m), dtype=torch.int32, device=device)
        t_sizes = torch.zeros((S, MAX_CAND + 3), dtype=torch.int32, device=device)
        C_in = 4 if cfg.RPN.USE_INTENSITY else 3
        t_prect = torch.empty((S, NP, 3), dtype=torch.float32, device=device)
        t_pin = torch.empty((S, NP, C_in), dtype=torch.float32, device=device)
        t_feat = torch.empty((S, NP, 1), dtype=torch.float32, device=device)
        b = _TrainBatch(S, pk.max_tiles, NP, C_in, int(self.reduce), 0, 0, 0, len(self.db_rows) if self.db is not None else 0,
                        *[t.data_ptr() for t in t_in], t_cn.data_ptr(), t_crec.data_ptr(), t_cbox.data_ptr(), t_ctrig.data_ptr(),
                        t_cmove.data_ptr(), t_rect.data_ptr(), t_valid.data_ptr(), t_flag.data_ptr(), t_cnt.data_ptr(),
                        t_lists.data_ptr(), t_sizes.data_ptr(), self.t_db.data_ptr() if self.db is not None else None, None, None,
                        t_prect.data_ptr(), t_pin.data_ptr(), t_feat.data_ptr())
        stream = C.c_void_p(_lib.current_stream(t_rect))
        codes = np.zeros((S, NP), dtype=np.int64)
        aug = np.zeros((S, 6), dtype=np.float64)
        gts, methods, factor_rows = [], [], []
        for s, sc in enumerate(scenes):
            t0 = time.perf_counter()
            cand = []
            if self.gt_aug and rng.rand() < _opt(cfg, "GT_AUG_APPLY_PROB"):
                cand = self.replay_candidates(sc["plane"])
                if cand and nb[s] == 0:
                    raise no_label_error("train_input", sc["id"])
            self.stats["draw_seconds"] += time.perf_counter() - t0
            if cand:
                k = len(cand)
                boxes = np.stack([box for _, box, _ in cand])
                t_cn[s] = k
                t_crec[s, :k] = dev(overlap_records(enlarged(boxes)))
                t_cbox[s, :k] = dev(boxes)
                t_ctrig[s, :k] = dev(self.db_trig[[e for e, _, _ in cand]])
                t_cmove[s, :k] = dev(np.array([mv for _, _, mv in cand], dtype=np.float64))
            b.scene_begin, b.scene_end, b.max_tiles = s, s + 1, int(nt[s])        # the grid covers the launched scene's own tiles
            _lib.call("prcnn_train_place", C.byref(b), stream)
            sizes = t_sizes[s].cpu().numpy().astype(np.int64)               # the scene's few ints: the sampler's draws need them
            n_kept, n_near, n_acc = int(sizes[0]), int(sizes[1]), int(sizes[2])
            self.last_kept.append((sc["id"], n_kept))
            slots = [int(v) for v in sizes[3:3 + n_acc]]
            accepted = [cand[v][0] for v in slots]
            t0 = time.perf_counter()
            if accepted:
                rows = np.concatenate([np.arange(self.db_off[cand[v][0]], self.db_off[cand[v][0] + 1], dtype=np.int64) |
                                       (np.int64(v) << SLOT_SHIFT) | (np.int64(KIND_DB) << KIND_SHIFT) for v in slots])
                rows_near = self.db_rows[rows & ((1 << SLOT_SHIFT) - 1), 2] < np.float32(NEAR_DEPTH)
            else:
                rows, rows_near = np.zeros((0,), np.int64), np.zeros((0,), bool)
            if NP < n_kept + len(rows):
                near_ids = np.concatenate((np.arange(n_near, dtype=np.int64) | (np.int64(KIND_NEAR) << KIND_SHIFT), rows[rows_near]))
                far_ids = np.concatenate((np.arange(n_kept - n_near, dtype=np.int64) | (np.int64(KIND_FAR) << KIND_SHIFT), rows[~rows_near]))
                codes[s] = sample_choice(rng, near_ids, far_ids, NP, self.npoints_faraway, self.with_replace)
            else:
                if n_kept + len(rows) == 0:
                    raise ValueError("train_input: sample %06d has no valid point" % sc["id"])
                codes[s] = sample_choice_all(rng, np.concatenate((np.arange(n_kept, dtype=np.int64), rows)), NP)
            gt, alpha = self._gt_of(sc, accepted)
            if _opt(cfg, "AUG_DATA"):
                angle, scale, flip, method = draw_augmentation(rng, cfg)
                gt = augment_boxes(gt, alpha, angle, scale, flip)
                methods.append(method)
                if angle is not None:
                    aug[s, 0:4] = rotation_terms(angle)
                aug[s, 4] = np.float32(scale) if scale is not None else 1.0
                aug[s, 5] = (1 if angle is not None else 0) | (2 if scale is not None else 0) | (4 if flip else 0)
            gts.append(gt)
            if self.obj_scale is not None:
                factor_rows.append(self._draw_factors(gt.shape[0]))
            self.stats["draw_seconds"] += time.perf_counter() - t0
        t_codes, t_aug = dev(codes), dev(aug)
        b.codes, b.aug = t_codes.data_ptr(), t_aug.data_ptr()
        _lib.call("prcnn_train_emit", C.byref(b), stream)
        out = {"sample_id": np.array(ids, dtype=np.int32), "random_select": np.ones(S, dtype=np.int32)}
        if _opt(cfg, "AUG_DATA"):
            out["aug_method"] = methods
        out["pts_input"], out["pts_rect"], out["pts_features"] = t_pin, t_prect, t_feat
        gt, counts, trig = rpn_eval.pack_gt(gts)
        if self.obj_scale is not None:
            from . import object_scale
            factors = np.ones(gt.shape[:2], dtype=np.float64)
            for s, row in enumerate(factor_rows):
                factors[s, :len(row)] = row
            _, gt, t_hits = object_scale.scale_objects(t_prect, gt, counts, factors, trig=trig, device=device, extra=t_pin)
            hits = t_hits.cpu().numpy()                                      # the batch's one read
            self.last_scaled = [(int(ids[s]), k, float(factors[s, k]), int(hits[s, k])) for s in range(S) for k in range(int(counts[s]))]
        if not cfg.RPN.FIXED:
            out["rpn_cls_label"], out["rpn_reg_label"] = rpn_eval.rpn_labels(t_prect, gt, counts, device=device, trig=trig)
        out["gt_boxes3d"] = gt
        return out

    def batch(self, indices):
        ids = [int(self.sample_id_list[i]) for i in indices]
        self.last_kept, self.last_scaled = [], []
        if self.device == "cpu":
            return self.collate([self._sample_cpu(i) for i in ids])
        return self._batch_device(ids)


def obj_scale_args(a):
    """the --obj_scale / --obj_scale_prob of a parsed namespace as RpnTrainInput's keywords (both flags are absent unless given)"""
    if hasattr(a, "obj_scale_prob") and not hasattr(a, "obj_scale"):
        raise ValueError("--obj_scale_prob needs --obj_scale LO HI")
    kw = {}
    if hasattr(a, "obj_scale"):
        kw["obj_scale"] = tuple(a.obj_scale)
        if hasattr(a, "obj_scale_prob"):
            kw["obj_scale_prob"] = a.obj_scale_prob
    return kw


def main(argv=None):
    from . import config
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.train_input", description=__doc__.split("\n")[0])
    ap.add_argument("--root", type=str, required=True)
    ap.add_argument("--gt_database_dir", type=str, default=None)
    ap.add_argument("--cfg_file", type=str, default=None)
    ap.add_argument("--class_name", type=str, default="Car")
    ap.add_argument("--split", type=str, default="train")
    ap.add_argument("--npoints", type=int, default=16384)
    ap.add_argument("--npoints_faraway", type=int, default=4000)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--save_dir", type=str, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--subsample", type=int, default=-1)
    ap.add_argument("--shuffle_subsample", type=str, default=None)
    ap.add_argument("--obj_scale", type=float, nargs=2, metavar=("LO", "HI"), default=argparse.SUPPRESS)
    ap.add_argument("--obj_scale_prob", type=float, default=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    cfg = config.make_cfg()
    if a.cfg_file:
        config.cfg_from_file(cfg, a.cfg_file)
    elif a.gt_database_dir:
        cfg["GT_AUG_ENABLED"], cfg["GT_AUG_RAND_NUM"], cfg["GT_AUG_APPLY_PROB"] = True, True, 1.0    # what the shipped yamls set
    src = RpnTrainInput(a.root, cfg, a.gt_database_dir, a.split, a.class_name, a.npoints, a.npoints_faraway, seed=a.seed, device=a.device,
                        subsample=a.subsample, shuffle_subsample=a.shuffle_subsample, **obj_scale_args(a))
    if a.save_dir:
        os.makedirs(a.save_dir, exist_ok=True)
    done, t0, k = 0, time.perf_counter(), 0
    for _ in range(a.epochs):
        for i0 in range(0, len(src), max(1, a.batch_size)):
            got = src.batch(range(i0, min(i0 + a.batch_size, len(src))))
            done += len(got["sample_id"])
            if a.save_dir:
                arrs = {key: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for key, v in got.items() if key != "aug_method"}
                np.savez_compressed(os.path.join(a.save_dir, "batch_%06d.npz" % k), aug_method=np.array(repr(got.get("aug_method"))), **arrs)
            k += 1
    if a.device != "cpu":
        import torch
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%d scenes in %.3f s: %.2f scenes/s (%s)" % (done, dt, done / max(dt, 1e-9), a.device))


if __name__ == "__main__":
    main()
