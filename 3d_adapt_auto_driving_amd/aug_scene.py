"""Augmented scenes of a KITTI-format tree (reference: pointrcnn/tools/generate_aug_scene.py): objects of a GT database
(gt_database.py) pasted onto the road plane of every training scene, the scene's points under them removed.

  place_candidates(scenes, jobs, db, ...)   the geometric part for a batch: device="cuda" runs csrc/aug_scene.hip, device="cpu" is the
                                            numpy restatement that follows the reference loop try by try (the checker)
  replay_candidates(rng, db, scope)         the tool's random stream for one scene, replayed on the host
  generate_aug_scene(root, gt_database, save_dir, ...)   the reference's tool

Command line:
  python -m 3d_adapt_auto_driving_amd.aug_scene --root R --gt_database_dir DB.pkl [--save_dir D] [--class_name Car] [--split train]
         [--include_similar] [--aug_times 4] [--device cuda|cpu]

Written, as the reference writes it: ``<save_dir>/rectified_data/%06d.bin`` ((n, 4) f32: the kept original points in their order, then
the pasted objects' points in acceptance order), ``<save_dir>/aug_label/%06d.txt`` (the class-filtered original labels through
to_kitti_format, then save_kitti_format's lines with its 80 % image-size discard and its alpha formula; the class column is
``--class_name``, "People" included), ``<save_dir>/<split>_aug.txt`` (the original ids, then base_id + sample_id with base_id =
(epoch + 1) * 400000, no trailing newline; copied into ``<root>/KITTI/ImageSets/``, the reference's hard-coded target for its default
root) and ``<save_dir>/log_info.txt``.  Read: velodyne, calib, label_2, planes and the PNG header of image_2.

The random stream.  In aug_one_scene no draw depends on a geometric result: per scene ``randint(10, 15)`` once, then
``randint(0, len(db) - 1)`` per try (the LAST database entry can never be drawn; kept), and every exit of a try -- ``continue`` on the
centre range check, ``break`` on cnt > extra_gt_num, ``continue`` on fewer than 5 points, else cnt += 1 -- looks at the entry only.  So
the host replays the whole run's stream first (legacy RandomState, seed 1024; a scene the tool skips -- class != Car without an object
of the class -- draws nothing), which gives every (epoch, scene) its ordered list of at most 15 candidates that reach the overlap
test; what remains is geometric and runs batched on the device.

Arithmetic.  The road plane is get_road_plane's, f64.  cur_height = (-d - a x - c z) / b and move_height = y - cur_height are f64; the
box's y is rounded to f32 once (f32(f64(y) - move_height)).  ``new_gt_points[:, 1] -= move_height`` with move_height a float64 SCALAR:
under NEP 50 (numpy >= 2; the fixture was made with 2.2.6 and records it) this is f32(f64(y) - move_height) per point, not an f32
subtraction; both paths here spell that out and do not depend on the installed numpy.  A cloud of ONE raw point is different: numpy
hands its (1, 4) products to the BLAS's gemv kernels, whose summation order the device restates (csrc/point_chains.hpp) as the
OpenBLAS behind the fixture's numpy evaluates them, so for n == 1 the cpu checker's own result depends on the installed BLAS.  The valid-point filter compares the f32 rect
coordinates with PC_AREA_SCOPE as float64 (70.4 is not an f32 number); the image test is f32.  The overlap is
iou3d_utils.boxes_iou3d_gpu's, tested ``max < 1e-8`` in f32; the removal is pts_in_boxes3d_cpu's inside test over h + 2.  The device path
equals the cpu path bit for bit.

A scene whose non-DontCare label list is empty makes the reference raise (``iou3d.max()`` of an empty array) as soon as a candidate
reaches the overlap test: here that is a ValueError that names the sample, not invented behaviour.  (When no candidate reaches the
test the reference passes such a scene through unchanged, and so does this module.)

The cpu path evaluates the rotated overlap with the repository's host oracle (oracle/ext_cpu.py as iou3d_utils' backend): it is the
checker of the device path, not a second product path, and needs the repository checkout on sys.path.
"""
import argparse
import concurrent.futures as cf
import contextlib
import ctypes as C
import importlib
import os
import shutil
import threading

import numpy as np

from . import _lib, kitti_io, kitti_utils
from .gt_database import box_trig, class_tuple, load_gt_database, sample_id_list
from .kitti_io import Object3d, png_size
from .scene_batch import (MAX_IO_WORKERS, TILE, as_calib, boxes_of_labels, check_device, check_pc_range, class_whitelist, cum,  # noqa: F401
                          database_rows, enlarged, no_label_error, offsets_to_device, pack_scenes, place_on_plane, to_device, valid_points)

TRY_TIMES = 50
MAX_CAND = 16                            # csrc/placement.hpp PLACE_MAX_CAND (the loop admits at most 15)
SEED = 1024
PC_AREA_SCOPE = {True: np.array([[-40, 40], [-1, 3], [0, 70.4]]), False: np.array([[-30, 30], [-1, 3], [0, 50]])}


def area_scope(class_name):
    """PC_AREA_SCOPE of the tool: x, y, z ranges in the rect frame, with the tool's dtypes (float64 for Car, int64 otherwise)."""
    return PC_AREA_SCOPE[class_name == "Car"]


def road_plane(path):
    """kitti_dataset.py:72-85: line 4 of the planes file, normal facing up, normalised; f64."""
    with open(path) as f:
        lines = f.readlines()
    plane = np.asarray([float(v) for v in lines[3].split()])
    if plane[1] > 0:
        plane = -plane
    return plane / np.linalg.norm(plane[0:3])


def shifted_points(points, move):
    out = points.copy()
    out[:, 1] = (out[:, 1].astype(np.float64) - move).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------------------- random stream
def new_rng():
    """The tool's stream: np.random.seed(1024)."""
    return np.random.RandomState(SEED)


def _admit(entry, scope, cnt, extra_gt_num):
    """One try after its draw -> "range" | "break" | "few" | "test" (generate_aug_scene.py:183-197)."""
    if not check_pc_range(entry["gt_box3d"][0:3], scope):
        return "range"
    if cnt > extra_gt_num:
        return "break"
    if len(entry["points"]) < 5:
        return "few"
    return "test"


def replay_candidates(rng, db, scope, stats=None):
    """The draws of one aug_one_scene call -> the database indices that reach the overlap test, in try order."""
    extra_gt_num = rng.randint(10, 15)
    cnt, out = 0, []
    for _ in range(TRY_TIMES):
        idx = rng.randint(0, len(db) - 1)
        what = _admit(db[idx], scope, cnt, extra_gt_num)
        if stats is not None:
            stats[what] = stats.get(what, 0) + 1
        if what == "break":
            break
        if what == "test":
            cnt += 1
            out.append(int(idx))
    return out


# --------------------------------------------------------------------------------------------------------------------- cpu path
_backend_lock = threading.RLock()


@contextlib.contextmanager
def host_overlap_backend():
    """iou3d_utils over the host oracle for the block (unless a host stand-in is installed already).  The swap replaces a module
    global: it is NOT safe while another thread uses iou3d_utils (a device call through it would land in the oracle).  The lock keeps
    two checker calls from undoing each other's swap; this module's own thread pool only reads files and never touches iou3d_utils."""
    from . import iou3d_utils
    with _backend_lock:
        yield from _swapped_backend(iou3d_utils)


def _swapped_backend(iou3d_utils):
    if not getattr(iou3d_utils.iou3d_cuda, "IS_HIP_EXTENSION", False):
        yield
        return
    try:
        ext_cpu = importlib.import_module("oracle.ext_cpu")
    except ImportError as e:
        raise RuntimeError("aug_scene: device='cpu' is the checker and needs the repository's oracle/ package on sys.path") from e
    saved = iou3d_utils.iou3d_cuda
    iou3d_utils.iou3d_cuda = ext_cpu.iou3d_cpu
    try:
        yield
    finally:
        iou3d_utils.iou3d_cuda = saved


class _CpuScene:
    """The state of one aug_one_scene call (generate_aug_scene.py:161-234)."""

    def __init__(self, sample_id, pts_rect, intensity, all_boxes, plane):
        self.sample_id, self.pts_rect, self.intensity, self.plane = sample_id, pts_rect, intensity, plane
        self.cur = enlarged(all_boxes)
        self.flag = np.ones(pts_rect.shape[0], dtype=np.int32)
        self.accepted, self.tested = [], []             # (db index, box, move) ; db indices

    def try_candidate(self, idx, entry):
        import torch
        from . import iou3d_utils, roipool3d_utils
        box, move = place_on_plane(entry["gt_box3d"], self.plane)
        self.tested.append(int(idx))
        if self.cur.shape[0] == 0:
            raise no_label_error("aug_scene", self.sample_id)
        iou3d = iou3d_utils.boxes_iou3d_gpu(torch.from_numpy(box.reshape(1, 7)), torch.from_numpy(self.cur)).numpy()
        if not (iou3d.max() < np.float32(1e-8)):
            return False
        big = box.copy()
        big[3] += 2
        mask = roipool3d_utils.pts_in_boxes3d_cpu(torch.from_numpy(self.pts_rect), torch.from_numpy(big.reshape(1, 7)))[0].numpy()
        self.flag[mask == 1] = 0
        self.cur = np.concatenate((self.cur, enlarged(box).reshape(1, 7)), axis=0)
        self.accepted.append((int(idx), box, move))
        return True

    def rows(self, db):
        keep = self.flag == 1
        pts, inten = [self.pts_rect[keep]], [self.intensity[keep]]
        if self.accepted:
            pts += [shifted_points(db[i]["points"], move) for i, _, move in self.accepted]
            inten += [db[i]["intensity"] for i, _, _ in self.accepted]
        return np.concatenate((np.concatenate(pts, 0), np.concatenate(inten, 0).reshape(-1, 1)), axis=1).astype(np.float32)


def aug_one_scene_cpu(rng, sample_id, pts_rect, intensity, all_boxes, plane, db, scope):
    """aug_one_scene try by try, drawing from ``rng`` -> the _CpuScene after the loop."""
    st = _CpuScene(sample_id, pts_rect, intensity, all_boxes, plane)
    extra_gt_num = rng.randint(10, 15)
    cnt = 0
    with host_overlap_backend():
        for _ in range(TRY_TIMES):
            idx = rng.randint(0, len(db) - 1)
            what = _admit(db[idx], scope, cnt, extra_gt_num)
            if what == "break":
                break
            if what != "test":
                continue
            cnt += 1
            st.try_candidate(idx, db[idx])
    return st


def _norm_scene(scene):
    pts, calib, img_shape, boxes, plane = scene
    return (np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 4)), as_calib(calib), tuple(int(v) for v in img_shape[:2]),
            np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(-1, 7)), np.asarray(plane, dtype=np.float64).reshape(4))


def _check_jobs(scenes, jobs, db, ids):
    for s, cand in jobs:
        if not 0 <= s < len(scenes):
            raise ValueError("aug_scene: job names scene %d of %d" % (s, len(scenes)))
        if len(cand) > MAX_CAND:
            raise ValueError("aug_scene: %d candidates in one job (at most %d)" % (len(cand), MAX_CAND))
        if any(not 0 <= i < len(db) for i in cand):
            raise ValueError("aug_scene: candidate outside the database")
        if len(cand) and scenes[s][3].shape[0] == 0:
            raise no_label_error("aug_scene", ids[s] if ids is not None else s)


def _place_cpu(scenes, jobs, db, scope, ids):
    valid = {}
    out = []
    with host_overlap_backend():
        for s, cand in jobs:
            pts, calib, shape, boxes, plane = scenes[s]
            if s not in valid:
                valid[s] = valid_points(pts, calib, shape, scope)
            st = _CpuScene(ids[s] if ids is not None else s, valid[s][0], valid[s][1], boxes, plane)
            for i in cand:
                st.try_candidate(i, db[i])
            out.append((st.rows(db), [(i, box) for i, box, _ in st.accepted]))
    return out


# ------------------------------------------------------------------------------------------------------------------ device path
_AugBatch = _lib.struct("prcnn_aug_batch")


class AugPlacer:
    """The device path: the database's points (x, y, z, intensity rows + offsets) and (cos ry, sin ry) are uploaded once and stay."""

    def __init__(self, db, device="cuda"):
        import torch
        if _lib.call("prcnn_aug_max_candidates") != MAX_CAND:
            raise _lib.PrcnnError("aug_scene: MAX_CAND differs from the library's")
        self.device, self.db = device, db
        pts, self.db_n, self.db_off = database_rows(db)
        self.db_boxes = np.stack([e["gt_box3d"] for e in db]).astype(np.float32) if db else np.zeros((0, 7), np.float32)
        self.db_trig = box_trig(self.db_boxes)
        self.t_pts = torch.from_numpy(pts if len(pts) else np.zeros((1, 4), np.float32)).to(device)
        self.t_off = torch.from_numpy(self.db_off).to(device)

    def __call__(self, scenes, jobs, scope, ids=None):
        import torch
        scenes = [_norm_scene(s) for s in scenes]
        jobs = [(int(s), [int(i) for i in cand]) for s, cand in jobs]
        _check_jobs(scenes, jobs, self.db, ids)
        S, J = len(scenes), len(jobs)
        if J == 0:
            return []
        device = self.device
        pk = pack_scenes([p for p, _, _, _, _ in scenes], [len(b) for _, _, _, b, _ in scenes], [c for _, c, _, _, _ in scenes],
                         [shape for _, _, shape, _, _ in scenes])
        job_scene = np.array([s for s, _ in jobs], dtype=np.int32)
        jt_off = cum(pk.nt[job_scene])
        if pk.pt_off[-1] >= 2 ** 31 or jt_off[-1] >= 2 ** 31:
            raise ValueError("aug_scene batch too large: split it")
        boxes = np.concatenate([b for _, _, _, b, _ in scenes]) if pk.box_off[-1] else np.zeros((1, 7), np.float32)
        cand_n = np.array([len(c) for _, c in jobs], dtype=np.int32)
        cand_db = np.zeros((J, MAX_CAND), dtype=np.int32)
        cand_box = np.zeros((J, MAX_CAND, 7), dtype=np.float32)
        cand_trig = np.zeros((J, MAX_CAND, 2), dtype=np.float32)
        cand_move = np.zeros((J, MAX_CAND), dtype=np.float64)
        for j, (s, cand) in enumerate(jobs):
            for k, i in enumerate(cand):
                cand_box[j, k], cand_move[j, k] = place_on_plane(self.db[i]["gt_box3d"], scenes[s][4])
                cand_db[j, k], cand_trig[j, k] = i, self.db_trig[i]
        dev = to_device(device)
        t_in = offsets_to_device(pk, dev) + [dev(a) for a in (pk.velo, pk.calib, np.asarray(scope, dtype=np.float64).reshape(6), boxes)]
        t_rect = torch.empty((max(1, int(pk.pt_off[-1])), 4), dtype=torch.float32, device=device)
        t_valid = torch.empty((max(1, int(pk.pt_off[-1])),), dtype=torch.uint8, device=device)
        t_job = [dev(a) for a in (job_scene, jt_off, cand_n, cand_db, cand_box, cand_trig, cand_move)]
        t_sizes = torch.zeros((J, MAX_CAND + 2), dtype=torch.int32, device=device)
        t_cnt = torch.empty((max(1, int(jt_off[-1])),), dtype=torch.int32, device=device)
        b = _AugBatch(S, J, pk.max_tiles, len(self.db), *[t.data_ptr() for t in t_in], t_rect.data_ptr(), t_valid.data_ptr(),
                      *[t.data_ptr() for t in t_job], t_sizes.data_ptr(), t_cnt.data_ptr(), self.t_pts.data_ptr(), self.t_off.data_ptr(),
                      None, None, None)
        stream = C.c_void_p(_lib.current_stream(t_rect))
        _lib.call("prcnn_aug_place", C.byref(b), stream)
        sizes = t_sizes.cpu().numpy().astype(np.int64)                      # the one D2H that sizes the output
        obj_off = np.zeros((J, MAX_CAND + 1), dtype=np.int64)
        out_off = np.zeros(J + 1, dtype=np.int64)
        accepted = []
        for j, (s, cand) in enumerate(jobs):
            slots = [int(k) for k in sizes[j, 2:2 + sizes[j, 1]]]
            accepted.append(slots)
            rows = [self.db_n[cand[k]] for k in slots]
            obj_off[j, :len(slots) + 1] = out_off[j] + sizes[j, 0] + cum(rows)
            obj_off[j, len(slots) + 1:] = obj_off[j, len(slots)]
            out_off[j + 1] = obj_off[j, len(slots)]
        total = int(out_off[-1])
        t_out = torch.empty((max(1, total), 4), dtype=torch.float32, device=device)
        t_oo, t_bo = dev(out_off), dev(obj_off)
        b.out_off, b.obj_off, b.out = t_oo.data_ptr(), t_bo.data_ptr(), t_out.data_ptr()
        if total:
            _lib.call("prcnn_aug_write", C.byref(b), stream)
        out = t_out.cpu().numpy()                                           # ... and the one for the rows
        return [(np.ascontiguousarray(out[out_off[j]:out_off[j + 1]]),
                 [(cand[k], cand_box[j, k].copy()) for k in accepted[j]]) for j, (s, cand) in enumerate(jobs)]


def place_candidates(scenes, jobs, db, class_name="Car", device="cuda", ids=None, placer=None):
    """scenes: iterable of (points (n, 4) f32 as a velodyne .bin holds them, calibration (kitti_io.Calibration, a calib file path or its
    dict), image shape (h, w), boxes (g, 7) f32 = the non-DontCare labels [x, y_bottom, z, h, w, l, ry], road plane (4,) f64);
    jobs: iterable of (scene index, database indices that reach the overlap test, in try order; at most 16); db: a GT database.
    -> per job (rows (m, 4) f32 = the scene's valid points outside every accepted box (h + 2) in their order, then the accepted objects'
    points; [(database index, placed box (7,) f32)] in acceptance order).  ``ids`` names the scenes in error messages."""
    scope = area_scope(class_name)
    if device == "cpu":
        scenes = [_norm_scene(s) for s in scenes]
        jobs = [(int(s), [int(i) for i in cand]) for s, cand in jobs]
        _check_jobs(scenes, jobs, db, ids)
        return _place_cpu(scenes, jobs, db, scope, ids)
    check_device(device)
    placer = placer if placer is not None else AugPlacer(db, device)
    return placer(scenes, jobs, scope, ids)


# ------------------------------------------------------------------------------------------------------------------------ tool
def filtrate_objects(obj_list, classes, include_similar):
    white = class_whitelist(classes, include_similar, sitting_with=("Pedestrian", "Cyclist"))
    return [o for o in obj_list if o.cls_type in white]


def kitti_lines(class_name, calib, boxes, objs, img_shape):
    """save_kitti_format (generate_aug_scene.py:39-64) -> the lines; ``objs`` are the database entries' ``obj``."""
    corners3d = kitti_utils.boxes3d_to_corners3d(boxes)
    img_boxes, _ = calib.corners3d_to_img_boxes(corners3d)
    img_boxes[:, 0] = np.clip(img_boxes[:, 0], 0, img_shape[1] - 1)
    img_boxes[:, 1] = np.clip(img_boxes[:, 1], 0, img_shape[0] - 1)
    img_boxes[:, 2] = np.clip(img_boxes[:, 2], 0, img_shape[1] - 1)
    img_boxes[:, 3] = np.clip(img_boxes[:, 3], 0, img_shape[0] - 1)
    w, h = img_boxes[:, 2] - img_boxes[:, 0], img_boxes[:, 3] - img_boxes[:, 1]
    ok = np.logical_and(w < img_shape[1] * 0.8, h < img_shape[0] * 0.8)
    lines = []
    for k in range(boxes.shape[0]):
        if ok[k] == 0:
            continue
        x, z, ry = boxes[k, 0], boxes[k, 2], boxes[k, 6]
        beta = np.arctan2(z, x)
        alpha = -np.sign(beta) * np.pi / 2 + beta + ry
        lines.append("%s %.2f %d %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" %
                     (class_name, objs[k].trucation, int(objs[k].occlusion), alpha, img_boxes[k, 0], img_boxes[k, 1], img_boxes[k, 2],
                      img_boxes[k, 3], boxes[k, 3], boxes[k, 4], boxes[k, 5], boxes[k, 0], boxes[k, 1], boxes[k, 2], boxes[k, 6]))
    return lines


def generate_aug_scene(root, gt_database, save_dir, split="train", class_name="Car", include_similar=False, aug_times=4, device="cuda",
                       batch_size=8, workers=8, log=print, rng=None):
    """The reference's AugSceneGenerator.generate_aug_scene on ``root/KITTI/object/training`` with ``gt_database`` (a list, or the path
    of a pickle that gt_database.py or the reference wrote) -> the list of written sample ids (the split file's lines).  Scenes are read
    by a thread pool of ``workers`` (<= 16); the device works on batches of ``batch_size`` scenes x ``aug_times`` epochs.  ``log``
    receives the reference's printed lines.  A scene with no label besides DontCare raises ValueError when a candidate reaches the
    overlap test (the reference raises there; see the module docstring).  The printed lines and the ``Save to file`` lines of
    log_info.txt come out in the reference's order once the scenes are done; a run that raises part-way still logs, in that order, the
    files it had written, and writes no split file."""
    classes = class_tuple(class_name)
    scope = area_scope(class_name)
    rng = rng if rng is not None else new_rng()
    os.makedirs(save_dir, exist_ok=True)
    log_fp = open(os.path.join(save_dir, "log_info.txt"), "w")

    def log_print(text):
        log(text)
        print(text, file=log_fp)

    try:
        if isinstance(gt_database, str):
            db_path, gt_database = gt_database, load_gt_database(gt_database)
            log_print("Loading gt_database(%d) from %s" % (len(gt_database), db_path))
        db = gt_database
        names = sample_id_list(root, split)
        ids = [int(x) for x in names]
        base = os.path.join(root, "KITTI", "object", "testing" if split == "test" else "training")
        data_dir, label_dir = os.path.join(save_dir, "rectified_data"), os.path.join(save_dir, "aug_label")
        os.makedirs(data_dir, exist_ok=True)
        os.makedirs(label_dir, exist_ok=True)

        def load_labels(sample_id):
            with open(os.path.join(base, "label_2", "%06d.txt" % sample_id)) as f:
                objs = [Object3d(line) for line in f.readlines()]
            return boxes_of_labels([o for o in objs if o.cls_type != "DontCare"]), filtrate_objects(objs, classes, include_similar)

        def load(sample_id, labels=None):
            pts = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
            calib = kitti_io.Calibration(os.path.join(base, "calib", "%06d.txt" % sample_id))
            width, height = png_size(os.path.join(base, "image_2", "%06d.png" % sample_id))
            plane = road_plane(os.path.join(base, "planes", "%06d.txt" % sample_id))
            boxes, objs = labels if labels is not None else load_labels(sample_id)
            return pts, calib, (int(height), int(width), 3), boxes, plane, objs

        def skipped(objs):
            return class_name != "Car" and len(objs) == 0

        def write(epoch, sample_id, calib, shape, objs, rows, accepted):
            """the two files of one (epoch, scene) -> (label file, new objects)"""
            base_id = (epoch + 1) * 400000
            rows.astype(np.float32).tofile(os.path.join(data_dir, "%06d.bin" % (base_id + sample_id)))
            label_file = os.path.join(label_dir, "%06d.txt" % (base_id + sample_id))
            with open(label_file, "w") as f:
                for o in objs:
                    print(o.to_kitti_format(), file=f)
                if accepted:
                    extra = np.concatenate([box.reshape(1, 7) for _, box in accepted], axis=0)
                    for line in kitti_lines(class_name, calib, extra, [db[i]["obj"] for i, _ in accepted], shape):
                        print(line, file=f)
            return label_file, len(accepted)

        split_list = list(names)
        written = {}                                      # (epoch, position) -> (label file, new objects)
        pool = cf.ThreadPoolExecutor(max_workers=max(1, min(MAX_IO_WORKERS, int(workers))))
        complete = False
        try:
            if device == "cpu":
                # the reference's order of everything: epoch by epoch, scene by scene, try by try
                for epoch in range(aug_times):
                    for k, sample_id in enumerate(ids):
                        pts, calib, shape, boxes, plane, objs = load(sample_id)
                        if skipped(objs):
                            continue
                        pts_rect, intensity = valid_points(pts, calib, shape, scope)
                        st = aug_one_scene_cpu(rng, sample_id, pts_rect, intensity, boxes, plane, db, scope)
                        written[(epoch, k)] = write(epoch, sample_id, calib, shape, objs, st.rows(db), [(i, box) for i, box, _ in st.accepted])
            else:
                check_device(device)
                # the stream first: it needs the labels only.  Then the geometry, batch by batch, every epoch of a scene in one call
                labels = list(pool.map(load_labels, ids))
                cands = {}
                for epoch in range(aug_times):
                    for k in range(len(ids)):
                        if not skipped(labels[k][1]):
                            cands[(epoch, k)] = replay_candidates(rng, db, scope)
                placer = AugPlacer(db, device)
                batch_size = max(1, int(batch_size))
                groups = [list(range(k, min(k + batch_size, len(ids)))) for k in range(0, len(ids), batch_size)]
                pending = [pool.submit(load, ids[k], labels[k]) for k in groups[0]] if groups else []
                for gi, group in enumerate(groups):
                    loaded = [f.result() for f in pending]
                    pending = [pool.submit(load, ids[k], labels[k]) for k in groups[gi + 1]] if gi + 1 < len(groups) else []
                    keys = [(epoch, k) for epoch in range(aug_times) for k in group if (epoch, k) in cands]
                    got = placer([x[:5] for x in loaded], [(k - group[0], cands[(epoch, k)]) for epoch, k in keys], scope, [ids[k] for k in group])
                    for (epoch, k), (rows, accepted) in zip(keys, got):
                        _, calib, shape, _, _, objs = loaded[k - group[0]]
                        written[(epoch, k)] = write(epoch, ids[k], calib, shape, objs, rows, accepted)
            complete = True
        finally:
            pool.shutdown()
            # the printed lines and the split list in the reference's order (the device path writes batch by batch, every epoch of a
            # scene at once).  When the run raised part-way, the files written so far still get their lines, so log_info.txt names them
            for epoch in range(aug_times):
                for k, sample_id in enumerate(ids):
                    if complete or (epoch, k) in written:
                        log("process gt sample (%s, id=%06d)" % (split, sample_id))
                    if (epoch, k) in written:
                        log_print("Save to file (new_obj: %s): %s" % (written[(epoch, k)][1], written[(epoch, k)][0]))
                        split_list.append("%06d" % ((epoch + 1) * 400000 + sample_id))
        split_file = os.path.join(save_dir, "%s_aug.txt" % split)
        with open(split_file, "w") as f:
            f.write("\n".join(split_list))
        log_print("Save split file to %s" % split_file)
        target_dir = os.path.join(root, "KITTI/ImageSets/")
        shutil.copy(split_file, target_dir)
        log_print("Copy split file from %s to %s" % (split_file, target_dir))
    finally:
        log_fp.close()
    return split_list


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.aug_scene", description=__doc__.split("\n")[0])
    ap.add_argument("--mode", type=str, default="generator")
    ap.add_argument("--root", type=str, default="../data/")
    ap.add_argument("--class_name", type=str, default="Car")
    ap.add_argument("--save_dir", type=str, default="./../data/KITTI/aug_scene/training")
    ap.add_argument("--split", type=str, default="train")
    ap.add_argument("--gt_database_dir", type=str, default="gt_database/train_gt_database_3level_Car.pkl")
    ap.add_argument("--include_similar", action="store_true", default=False)
    ap.add_argument("--aug_times", type=int, default=4)
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--batch_size", type=int, default=8)
    a = ap.parse_args(argv)
    if a.mode == "generator":
        generate_aug_scene(a.root, a.gt_database_dir, a.save_dir, a.split, a.class_name, a.include_similar, a.aug_times, a.device, a.batch_size)


if __name__ == "__main__":
    main()
