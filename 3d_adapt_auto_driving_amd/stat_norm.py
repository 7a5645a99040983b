"""Statistical normalization (SN) of KITTI-format datasets: the method of "Train in Germany, Test in the USA".

Every Car / Van of a scene is rescaled toward the target domain's mean size: its LiDAR points are scaled in the box frame, its
label is rewritten, the 2-D boxes of all objects are re-projected and the occlusion-derived field is recomputed
(reference: stat_norm/stat.py get_dataset_stats, stat_norm/norm.py get_scale_map / rescale_ptc / scale_labels / convert).

  label_stats(root, split)       car-size statistics of a tree -> label_stats_<split>.json (the reference's text)
  scale_map(src, dst)            the per-axis scale factor of a box for a given ratio
  rescale_scenes(...)            rescale_ptc + scale_labels for a batch of scenes; device="cuda" runs csrc/stat_norm.hip,
                                 device="cpu" is the numpy restatement (the checker)
  convert_tree(src, dst, ...)    norm.convert: a whole tree, file I/O overlapped with the device through a small thread pool

Command line:
  python -m 3d_adapt_auto_driving_amd.stat_norm stats ROOT [--split train]
  python -m 3d_adapt_auto_driving_amd.stat_norm convert SRC DST --src_stats J --dst_stats J [--avoid_conflict] [--align_front]
         [--classes Car,Van] [--device cpu|cuda] [--image_size W H] [--batch N]

Arithmetic: f64 throughout, in the reference's order.  Its np.dot calls are OpenBLAS dgemm, fused multiply-add chains over the inner
index; the numpy path calls np.dot the same way, the kernels spell the chains out (tests/golden g15 pins both to the reference's own
output).  The reference builds its occlusion map as ``np.ones(uint8) * -1``, which numpy 1.x promotes to an int16 map with -1
background; that is the map painted here.
"""
import argparse
import concurrent.futures as cf
import copy
import ctypes as C
import json
import os
import shutil
from itertools import chain

import numpy as np

from . import _lib
from .kitti_io import Object3d, png_size, read_label_lines  # noqa: F401  (the label parser lives there; imported from here too)
from .scene_batch import MAX_IO_WORKERS, TILE, as_calib, check_device, cum, offsets_to_device, pack_scenes, to_device  # noqa: F401

RATIOS = np.arange(1, -0.1, -0.1)      # the avoid_conflict trial ratios; the last one is 2.22e-16, not 0
STAT_SUBJECTS = ("height", "width", "length")
SPLIT_DIRS = {"train": "training", "val": "training", "test": "testing"}

_T, _R, _XLO = _lib.PRCNN_SN_T, _lib.PRCNN_SN_R, _lib.PRCNN_SN_XLO      # the boxd record's layout (include/prcnn_hip.h)
_SCALE, _FSCALE, _SHIFT, _FLAG1 = _lib.PRCNN_SN_SCALE, _lib.PRCNN_SN_FSCALE, _lib.PRCNN_SN_SHIFT, _lib.PRCNN_SN_FLAG1


# ---------------------------------------------------------------------------------------------------------------- labels, calib
def parse_calib(text):
    """A KITTI calib file's text -> dict of float arrays (the date-like lines are skipped, as the reference does)."""
    data = {}
    for line in text.splitlines():
        line = line.rstrip()
        if not line:
            continue
        key, value = line.split(":", 1)
        try:
            data[key] = np.array([float(x) for x in value.split()])
        except ValueError:
            pass
    return data


class Calib:
    """The matrices kitti_util.Calibration holds.  ``R0_inv`` / ``C2V`` may be handed in (the fixtures carry the reference's own,
    so that the host LAPACK cannot enter a bitwise comparison)."""

    def __init__(self, calibs, R0_inv=None, C2V=None):
        self.P = np.reshape(calibs["P2"], [3, 4])
        self.V2C = np.reshape(calibs["Tr_velo_to_cam"], [3, 4])
        self.R0 = np.reshape(calibs["R0_rect"], [3, 3])
        if C2V is None:
            C2V = np.zeros_like(self.V2C)
            C2V[0:3, 0:3] = np.transpose(self.V2C[0:3, 0:3])
            C2V[0:3, 3] = np.dot(-np.transpose(self.V2C[0:3, 0:3]), self.V2C[0:3, 3])
        self.C2V = np.asarray(C2V, dtype=np.float64).reshape(3, 4)
        self.R0_inv = np.asarray(np.linalg.inv(self.R0) if R0_inv is None else R0_inv, dtype=np.float64).reshape(3, 3)

    @classmethod
    def from_file(cls, path):
        with open(path) as f:
            return cls(parse_calib(f.read()))

    @staticmethod
    def _hom(p):
        return np.hstack((p, np.ones((p.shape[0], 1))))

    def velo_to_rect(self, p):
        ref = np.dot(self._hom(p), np.transpose(self.V2C))
        return np.transpose(np.dot(self.R0, np.transpose(ref)))

    def rect_to_velo(self, p):
        ref = np.transpose(np.dot(self.R0_inv, np.transpose(p)))
        return np.dot(self._hom(ref), np.transpose(self.C2V))

    def rect_to_image2(self, p):
        uv = np.dot(self._hom(p), np.transpose(self.P))
        uv[:, 0] /= uv[:, 2]
        uv[:, 1] /= uv[:, 2]
        return uv


# ------------------------------------------------------------------------------------------------------------------ statistics
def _load_stats(stats):
    if isinstance(stats, dict):
        return stats
    with open(stats) as f:
        return json.load(f)


def label_stats(root, split="train", force=False):
    """stat.py get_dataset_stats: mean / population std of the Car heights, widths and lengths of ``<root>/<split>.txt``, written
    to ``<root>/label_stats_<split>.json`` (reused unless ``force``)."""
    if split not in SPLIT_DIRS:
        raise ValueError("split must be one of %s" % sorted(SPLIT_DIRS))
    stat_file = os.path.join(root, "label_stats_%s.json" % split)
    if os.path.isfile(stat_file) and not force:
        with open(stat_file) as f:
            return json.load(f)
    with open(os.path.join(root, "%s.txt" % split)) as f:
        ids = [x.strip() for x in f.readlines()]
    label_dir = os.path.join(root, SPLIT_DIRS[split], "label_2")
    vals = {x: [] for x in STAT_SUBJECTS}
    for i in ids:
        for line in read_label_lines(os.path.join(label_dir, "%s.txt" % i)):
            obj = Object3d(line)
            if obj.cls_type == "Car":
                vals["height"].append(obj.h)
                vals["width"].append(obj.w)
                vals["length"].append(obj.l)
    stats = {x: {"mean": float(np.mean(np.array(vals[x]))), "std": float(np.std(np.array(vals[x])))} for x in STAT_SUBJECTS}
    with open(stat_file, "w") as f:
        json.dump(stats, f, indent=4)
    return stats


class ScaleMap:
    """get_scale_map: ``mapping(obj, ratio)`` -> (1, 3) factors in l, h, w order, ``(x + (dst.mean - src.mean) * ratio) / x``."""

    def __init__(self, src, dst):
        self.src, self.dst = _load_stats(src), _load_stats(dst)

    def _one(self, x, key, ratio):
        return x + (self.dst[key]["mean"] - self.src[key]["mean"]) * ratio

    def __call__(self, obj, ratio):
        return (np.array([self._one(obj.l, "length", ratio), self._one(obj.h, "height", ratio), self._one(obj.w, "width", ratio)])
                / np.array([obj.l, obj.h, obj.w])).reshape(1, 3)


def scale_map(src_stats, dst_stats):
    return ScaleMap(src_stats, dst_stats)


# ------------------------------------------------------------------------------------------------------------ per-object arithmetic
def _rot(ry):
    return np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])


def _align_shifts(obj, lhw):
    """align_front: up to two (dx, dz) shifts (None where the condition fails) for the new size ``lhw`` (list l, h, w)."""
    l, _, w = lhw
    dist = np.linalg.norm(obj.t)
    alpha = np.arctan2(np.sin(obj.alpha), np.cos(obj.alpha))
    out = [None, None]
    if np.abs(np.sin(alpha)) * dist > obj.l / 2.0:
        shift = (obj.l - l) / 2.0
        angle = -obj.ry if 0 < alpha else -obj.ry + np.pi
        out[0] = (shift * np.cos(angle), shift * np.sin(angle))
    if np.abs(np.cos(alpha)) * dist > obj.w / 2.0:
        shift = (obj.w - w) / 2.0
        angle = -obj.ry - np.pi / 2.0 if -np.pi / 2.0 < alpha < np.pi / 2.0 else -obj.ry + np.pi / 2.0
        out[1] = (shift * np.cos(angle), shift * np.sin(angle))
    return out


def _new_size(obj, mapping, ratio):
    return (np.array([obj.l, obj.h, obj.w]) * mapping(obj, ratio).reshape(-1)).tolist()


def _refine(obj, calib, w, h):
    """2-D box = the image-clipped min / max of the projected 3-D corners (norm.py refine / gen_obj_box_ptc)."""
    l, bw, bh = obj.l, obj.w, obj.h
    corners = np.vstack([[l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2],
                         [-bh, -bh, -bh, -bh, 0, 0, 0, 0],
                         [bw / 2, -bw / 2, -bw / 2, bw / 2, bw / 2, -bw / 2, -bw / 2, bw / 2]])
    c3 = np.dot(_rot(obj.ry), corners)
    c3[0, :] = c3[0, :] + obj.t[0]
    c3[1, :] = c3[1, :] + obj.t[1]
    c3[2, :] = c3[2, :] + obj.t[2]
    uv = calib.rect_to_image2(np.transpose(c3))
    bbox = list(chain(np.min(uv, axis=0).tolist()[0:2], np.max(uv, axis=0).tolist()[0:2]))
    obj.box2d = np.array([max(0, bbox[0]), max(0, bbox[1]), min(w, bbox[2]), min(h, bbox[3])])


def paint_rects(objs):
    """The painting rectangles of postprocessing: (y0, y1, x0, x1) = int(round()) (half to even) of the 2-D box, as slice bounds."""
    return [(int(round(o.box2d[1])), int(round(o.box2d[3])), int(round(o.box2d[0])), int(round(o.box2d[2]))) for o in objs]


def paint_occlusion(rects, h, w):
    """Host painter: paint rectangle i with i in turn over an (h, w) int16 map of -1 (slice semantics, negative bounds included);
    -> pixels owned by each rectangle."""
    m = np.full((h, w), -1, dtype=np.int16)
    for i, (y0, y1, x0, x1) in enumerate(rects):
        m[y0:y1, x0:x1] = i
    unique, counts = np.unique(m, return_counts=True)
    out = np.zeros(len(rects), dtype=np.int64)
    for u, c in zip(unique.tolist(), counts.tolist()):
        if u >= 0:
            out[u] = c
    return out


def _resolved(rects, h, w):
    """Slice bounds -> explicit half-open ranges inside the map (what the device painter reads)."""
    out = []
    for y0, y1, x0, x1 in rects:
        a, b, _ = slice(y0, y1).indices(h)
        c, d, _ = slice(x0, x1).indices(w)
        out.append((a, max(a, b), c, max(c, d)))
    return out


def device_paint_occlusion(rects_per_scene, h, w, device="cuda"):
    """paint_occlusion for a batch of scenes in one launch (csrc/stat_norm.hip sn_occlusion_kernel) -> list of int64 arrays."""
    import torch
    n = [len(r) for r in rects_per_scene]
    off = cum(n).astype(np.int32)
    flat = [r for rs in rects_per_scene for r in _resolved(rs, h, w)]
    rects = torch.from_numpy(np.asarray(flat, dtype=np.int32).reshape(-1, 4) if flat else np.zeros((1, 4), np.int32)).to(device)
    offs = torch.from_numpy(off).to(device)
    counts = torch.zeros(max(1, int(off[-1])), dtype=torch.int32, device=device)
    _lib.call("prcnn_stat_norm_occlusion", len(n), int(h), int(w), max(n) if n else 0, offs.data_ptr(), rects.data_ptr(),
              counts.data_ptr(), C.c_void_p(_lib.current_stream(counts)))
    got = counts.cpu().numpy().astype(np.int64)
    return [got[off[i]:off[i + 1]] for i in range(len(n))]


def _labels_stage1(objs, mapping, ratios, calib, w0, h0, align_front, classes):
    """scale_labels up to the painting: new sizes (and shifted centres), refined 2-D boxes, stable sort by depth (far first)."""
    new, cnt = [], 0
    for obj in objs:
        o = copy.deepcopy(obj)
        if obj.cls_type in classes:
            lhw = _new_size(obj, mapping, ratios[cnt])
            if align_front:
                for sh in _align_shifts(obj, lhw):
                    if sh is not None:
                        o.t[0] += sh[0]
                        o.t[2] += sh[1]
            o.l, o.h, o.w = lhw
            cnt += 1
        new.append(o)
    for o in new:
        _refine(o, calib, w0, h0)
    return sorted(new, key=lambda x: x.t[2], reverse=True)


def _labels_stage2(objs, counts, scene):
    """postprocessing after the painting: occlusion = 1 - pixels / box2d area -> the truncation field."""
    lines = []
    for i, o in enumerate(objs):
        c = np.int64(counts[i]) if counts[i] else 0
        with np.errstate(all="ignore"):
            occ = 1.0 - c / (o.box2d[3] - o.box2d[1]) / (o.box2d[2] - o.box2d[0])
        if np.isnan(occ):
            raise ValueError("scene %s: object %d (%s, sorted order) has a zero-area 2-D box and no pixels: its occlusion is "
                             "undefined" % (scene, i, o.cls_type))
        o.trucation = int(np.clip(occ * 4, 0, 3))
        lines.append(o.to_kitti_format())
    return lines


# ------------------------------------------------------------------------------------------------------------------ numpy path
def _rescale_cpu(velo, objs, calib, mapping, avoid_conflict, align_front, classes):
    ptc = calib.velo_to_rect(velo[:, :3])
    patches, ratios, counts = [], [], []
    mask = np.ones(ptc.shape[0], dtype=bool)
    for obj in objs:
        if obj.cls_type not in classes:
            continue
        R = _rot(obj.ry)
        f = np.dot(ptc - obj.t, R)
        box = (f[:, 0] > -obj.l / 2.0) & (f[:, 0] < obj.l / 2.0) & (f[:, 2] > -obj.w / 2.0) & (f[:, 2] < obj.w / 2.0) & \
              (f[:, 1] > -obj.h)
        inside = box & (f[:, 1] < 0)
        n_in = int(np.sum(inside))
        ratio = 0
        if n_in > 0:
            mask[inside] = False
            fin = f[inside]
            if avoid_conflict:
                env0 = int(np.sum(box & (f[:, 1] < -0.5)))
                for ratio in RATIOS:
                    tmp = fin * mapping(obj, ratio)
                    env = (f[:, 0] > np.min(tmp[:, 0])) & (f[:, 0] < np.max(tmp[:, 0])) & \
                          (f[:, 1] > np.min(tmp[:, 1])) & (f[:, 1] < -0.5) & \
                          (f[:, 2] > np.min(tmp[:, 2])) & (f[:, 2] < np.max(tmp[:, 2]))
                    if int(np.sum(env)) - env0 < 10:
                        break
            else:
                ratio = 1
                tmp = fin * mapping(obj, ratio)
            patch = np.dot(tmp, R.T) + obj.t
            if align_front:
                for sh in _align_shifts(obj, _new_size(obj, mapping, ratio)):
                    if sh is not None:
                        patch[:, 0] += sh[0]
                        patch[:, 2] += sh[1]
            patches.append(patch)
        ratios.append(ratio)
        counts.append(n_in)
    out = calib.rect_to_velo(np.concatenate(patches + [ptc[mask]], axis=0))
    cloud = np.concatenate([out, np.ones((out.shape[0], 1), dtype=np.float32)], axis=1).astype(np.float32)
    return cloud, ratios, counts


# ---------------------------------------------------------------------------------------------------------------- device path
_SnBatch = _lib.struct("prcnn_sn_batch")


def _box_record(obj, mapping, avoid_conflict):
    rec = np.zeros(_lib.PRCNN_SN_BOXD)
    rec[_T:_T + 3] = obj.t
    rec[_R:_R + 9] = _rot(obj.ry).reshape(-1)
    rec[_XLO:_XLO + 5] = (-obj.l / 2.0, obj.l / 2.0, -obj.h, -obj.w / 2.0, obj.w / 2.0)        # XLO, XHI, YLO, ZLO, ZHI
    if avoid_conflict:
        rec[_SCALE:_SCALE + 33] = np.concatenate([mapping(obj, r).reshape(-1) for r in RATIOS])
    return rec


def _rescale_device(scenes, mapping, avoid_conflict, align_front, classes, device):
    """scenes: list of (velo (n, 4) f32, objects without DontCare, Calib) -> clouds, ratios, inside counts per scene."""
    import torch
    S = len(scenes)
    boxes = [[o for o in objs if o.cls_type in classes] for _, objs, _ in scenes]
    pk = pack_scenes([v for v, _, _ in scenes], [len(b) for b in boxes])
    nb, box_off, tile_off, bt_off = pk.nb, pk.box_off, pk.tile_off, cum(pk.nb * pk.nt)
    if pk.pt_off[-1] >= 2 ** 31 or bt_off[-1] >= 2 ** 31:
        raise ValueError("stat_norm batch too large: split it")
    nbox = int(box_off[-1])
    flat = [o for b in boxes for o in b]
    boxd = np.stack([_box_record(o, mapping, avoid_conflict) for o in flat]) if flat else np.zeros((1, _lib.PRCNN_SN_BOXD))
    calib = np.stack([np.concatenate([c.V2C.ravel(), c.R0.ravel(), c.R0_inv.ravel(), c.C2V.ravel()]) for _, _, c in scenes])
    dev = to_device(device)
    t_pt, t_tile, t_box = offsets_to_device(pk, dev)
    t_bt, t_velo, t_calib, t_boxd = dev(bt_off), dev(pk.velo), dev(calib), dev(boxd)
    t_boxi = torch.zeros((max(1, nbox), _lib.PRCNN_SN_BOXI), dtype=torch.int32, device=device)
    t_mm = torch.tensor([np.inf] * 3 + [-np.inf] * 3, dtype=torch.float64, device=device).repeat(max(1, nbox), 1)
    t_btc = torch.zeros(max(1, int(bt_off[-1])), dtype=torch.int32, device=device)
    t_rem = torch.zeros(max(1, int(tile_off[-1])), dtype=torch.int32, device=device)
    t_sc = torch.zeros((S, 4), dtype=torch.int32, device=device)
    b = _SnBatch(S, pk.max_tiles, int(nb.max()) if S else 0, int(bool(avoid_conflict)),
                 t_pt.data_ptr(), t_tile.data_ptr(), t_box.data_ptr(), t_bt.data_ptr(), t_velo.data_ptr(), t_calib.data_ptr(),
                 t_boxd.data_ptr(), t_boxi.data_ptr(), t_mm.data_ptr(), t_btc.data_ptr(), t_rem.data_ptr(), t_sc.data_ptr(), None, None)
    stream = C.c_void_p(_lib.current_stream(t_velo))
    _lib.call("prcnn_stat_norm_count", C.byref(b), stream)
    _lib.call("prcnn_stat_norm_choose", C.byref(b), stream)
    small = torch.cat([t_boxi[:, [_lib.PRCNN_SN_CNT, _lib.PRCNN_SN_RIDX]].reshape(-1), t_sc.reshape(-1)]).cpu().numpy()   # the one D2H that sizes
    cnt_ridx = small[:2 * max(1, nbox)].reshape(-1, 2)[:nbox]
    n_out = small[2 * max(1, nbox):].reshape(S, 4)[:, 2].astype(np.int64)
    ratios_flat = []
    for g, obj in enumerate(flat):
        cnt, q = int(cnt_ridx[g, 0]), int(cnt_ridx[g, 1])
        ratio = 0 if cnt == 0 else (RATIOS[q] if avoid_conflict else 1)
        ratios_flat.append(ratio)
        if cnt:
            lhw = None
            boxd[g, _FSCALE:_FSCALE + 3] = mapping(obj, ratio).reshape(-1)
            if align_front:
                lhw = _new_size(obj, mapping, ratio)
                for k, sh in enumerate(_align_shifts(obj, lhw)):
                    if sh is not None:
                        boxd[g, _SHIFT + 2 * k:_SHIFT + 2 * k + 2] = sh
                        boxd[g, _FLAG1 + k] = 1.0
    out_off = cum(n_out)
    t_boxd.copy_(torch.from_numpy(boxd))
    t_off = dev(out_off)
    t_out = torch.empty((max(1, int(out_off[-1])), 4), dtype=torch.float32, device=device)
    b.out_off, b.out = t_off.data_ptr(), t_out.data_ptr()
    _lib.call("prcnn_stat_norm_write", C.byref(b), stream)
    out = t_out.cpu().numpy()
    clouds = [out[out_off[s]:out_off[s + 1]] for s in range(S)]
    ratios = [ratios_flat[box_off[s]:box_off[s + 1]] for s in range(S)]
    counts = [cnt_ridx[box_off[s]:box_off[s + 1], 0].astype(np.int64).tolist() for s in range(S)]
    return clouds, ratios, counts


# -------------------------------------------------------------------------------------------------------------------- public
def rescale_scenes(velos, label_lines, calibs, mapping, avoid_conflict=False, align_front=False, rescaled_classes=("Car", "Van"),
                   image_size=(1242, 375), device="cuda", names=None, details=False):
    """rescale_ptc + scale_labels for a batch of scenes.

    velos: (n, 4) float32 clouds as read from .bin; label_lines: per scene the label file's lines (DontCare lines are dropped);
    calibs: per scene a Calib, a calib file path or the parse_calib dict; mapping: scale_map(); image_size: (w, h).
    -> (clouds, labels): per scene the (n_out, 4) float32 cloud as format_lidar_data writes it and the label lines as save_labels
    writes them; with ``details`` also the per-box ratios and inside-point counts of the rescaled objects."""
    check_device(device)
    classes = tuple(rescaled_classes)
    w0, h0 = image_size
    names = list(names) if names is not None else [str(i) for i in range(len(velos))]
    scenes = []
    for v, lines, c in zip(velos, label_lines, calibs):
        objs = [o for o in (Object3d(line) for line in lines) if o.cls_type != "DontCare"]
        calib = as_calib(c, Calib, Calib.from_file if isinstance(c, str) else Calib)
        scenes.append((np.asarray(v, dtype=np.float32).reshape(-1, 4), objs, calib))
    if device == "cpu":
        res = [_rescale_cpu(v, o, c, mapping, avoid_conflict, align_front, classes) for v, o, c in scenes]
        clouds, ratios, counts = [r[0] for r in res], [r[1] for r in res], [r[2] for r in res]
    else:
        clouds, ratios, counts = _rescale_device(scenes, mapping, avoid_conflict, align_front, classes, device)
    sorted_objs = [_labels_stage1(o, mapping, r, c, w0, h0, align_front, classes) for (_, o, c), r in zip(scenes, ratios)]
    rects = [paint_rects(o) for o in sorted_objs]
    if device == "cpu":
        pix = [paint_occlusion(r, h0, w0) for r in rects]
    else:
        pix = device_paint_occlusion(rects, h0, w0, device)
    labels = [_labels_stage2(o, p, nm) for o, p, nm in zip(sorted_objs, pix, names)]
    if details:
        return clouds, labels, ratios, counts
    return clouds, labels


def convert_tree(src_root, dst_root, src_stats, dst_stats, avoid_conflict=False, align_front=False,
                 rescaled_classes=("Car", "Van"), image_size=None, batch=8, device="cuda", workers=8,
                 image_folder="image_2", calib_folder="calib", label_folder="label_2"):
    """norm.convert for one (source, target) pair: ``dst_root`` gets the split files, training/{velodyne,label_2} with the rescaled
    scenes of trainval.txt and symlinks training/{image_2,calib} to the source.  src_stats / dst_stats: dicts or JSON paths
    (label_stats_train.json or car-sales statistics).  Reads and writes run on a thread pool of ``workers`` (<= 16) while the
    device works on the current batch."""
    mapping = scale_map(src_stats, dst_stats)
    if image_size is None:
        with open(os.path.join(src_root, "train.txt")) as f:
            first = f.readlines()[0].rstrip()
        image_size = png_size(os.path.join(src_root, "training", image_folder, "%s.png" % first))
    w0, h0 = (int(x) for x in image_size)
    os.makedirs(dst_root, exist_ok=True)
    for split in ("train", "val", "trainval"):
        shutil.copyfile(os.path.join(src_root, "%s.txt" % split), os.path.join(dst_root, "%s.txt" % split))
    root = os.path.join(dst_root, "training")
    os.makedirs(root, exist_ok=True)
    for name, folder in (("image_2", image_folder), ("calib", calib_folder)):
        link = os.path.join(root, name)
        if os.path.lexists(link):
            os.remove(link)
        os.symlink(os.path.abspath(os.path.join(src_root, "training", folder)), link)
    os.makedirs(os.path.join(root, "velodyne"), exist_ok=True)
    os.makedirs(os.path.join(root, label_folder), exist_ok=True)
    with open(os.path.join(src_root, "trainval.txt")) as f:
        ids = [x.strip() for x in f.readlines()]
    src_tr = os.path.join(src_root, "training")

    def load(i):
        velo = np.fromfile(os.path.join(src_tr, "velodyne", "%s.bin" % i), dtype=np.float32).reshape(-1, 4)
        return velo, read_label_lines(os.path.join(src_tr, label_folder, "%s.txt" % i)), \
            Calib.from_file(os.path.join(src_tr, calib_folder, "%s.txt" % i))

    def save(i, cloud, lines):
        cloud.reshape(-1).tofile(os.path.join(root, "velodyne", "%s.bin" % i))
        with open(os.path.join(root, label_folder, "%s.txt" % i), "w") as f:
            f.write("\n".join(lines))

    batch = max(1, int(batch))
    groups = [ids[k:k + batch] for k in range(0, len(ids), batch)]
    with cf.ThreadPoolExecutor(max_workers=max(1, min(MAX_IO_WORKERS, int(workers)))) as pool:
        pending = [pool.submit(load, i) for i in groups[0]] if groups else []
        writes = []
        for gi, group in enumerate(groups):
            loaded = [f.result() for f in pending]
            pending = [pool.submit(load, i) for i in groups[gi + 1]] if gi + 1 < len(groups) else []
            clouds, labels = rescale_scenes([x[0] for x in loaded], [x[1] for x in loaded], [x[2] for x in loaded], mapping,
                                            avoid_conflict, align_front, rescaled_classes, (w0, h0), device, names=group)
            writes += [pool.submit(save, i, c, l) for i, c, l in zip(group, clouds, labels)]
        for f in writes:
            f.result()
    return len(ids)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.stat_norm", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("stats", help="car-size statistics of a KITTI-format tree -> ROOT/label_stats_<split>.json")
    s.add_argument("root")
    s.add_argument("--split", default="train", choices=sorted(SPLIT_DIRS))
    s.add_argument("--force", action="store_true")
    c = sub.add_parser("convert", help="rescale a KITTI-format tree toward another domain's car sizes")
    c.add_argument("src")
    c.add_argument("dst")
    c.add_argument("--src_stats", required=True)
    c.add_argument("--dst_stats", required=True)
    c.add_argument("--avoid_conflict", action="store_true")
    c.add_argument("--align_front", action="store_true")
    c.add_argument("--classes", default="Car,Van")
    c.add_argument("--device", default="cuda")
    c.add_argument("--image_size", type=int, nargs=2, metavar=("W", "H"))
    c.add_argument("--batch", type=int, default=8)
    a = ap.parse_args(argv)
    if a.cmd == "stats":
        print(json.dumps(label_stats(a.root, a.split, a.force), indent=4))
    else:
        n = convert_tree(a.src, a.dst, a.src_stats, a.dst_stats, a.avoid_conflict, a.align_front,
                         tuple(x for x in a.classes.split(",") if x), a.image_size, a.batch, a.device)
        print("converted %d scenes into %s" % (n, a.dst))


if __name__ == "__main__":
    main()
