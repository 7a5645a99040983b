"""KITTI label files and annotation dicts of the offline evaluator (evaluate/kitti_common.py:293-360): text rows -> dicts of arrays
and back, the two rotated-box layouts, and the columnar form of an annotation list (SplitSide) that every whole-split launch and
both statistic paths read."""
import os
import pathlib
import re

import numpy as np

CLASS_CODE = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4}      # include/prcnn_hip.h: the split table


def _anno_from_rows(rows):
    """rows: list of token lists (15 or 16 tokens).  dimensions are stored l, h, w (file order h, w, l)."""
    n = len(rows)
    anno = {
        "name": np.array([r[0] for r in rows]),
        "truncated": np.array([float(r[1]) for r in rows]),
        "occluded": np.array([int(r[2]) for r in rows]),
        "alpha": np.array([float(r[3]) for r in rows]),
        "bbox": np.array([[float(v) for v in r[4:8]] for r in rows], dtype=np.float64).reshape(-1, 4),
        "dimensions": np.array([[float(v) for v in r[8:11]] for r in rows], dtype=np.float64).reshape(-1, 3)[:, [2, 0, 1]],
        "location": np.array([[float(v) for v in r[11:14]] for r in rows], dtype=np.float64).reshape(-1, 3),
        "rotation_y": np.array([float(r[14]) for r in rows]).reshape(-1),
    }
    anno["score"] = np.array([float(r[15]) for r in rows]) if n != 0 and len(rows[0]) == 16 else np.zeros([n])
    return anno


def get_label_anno(label_path):
    with open(label_path, "r") as f:
        return _anno_from_rows([line.strip().split(" ") for line in f.readlines()])


def get_label_annos(label_folder, image_ids=None):
    folder = pathlib.Path(label_folder)
    if image_ids is None:
        pat = re.compile(r"^\d{6}.txt$")
        image_ids = sorted(int(p.stem) for p in folder.glob("*.txt") if pat.match(p.name))
    if not isinstance(image_ids, list):
        image_ids = list(range(image_ids))
    return [get_label_anno(folder / ("%06d.txt" % i)) for i in image_ids]


def filter_annos_low_score(annos, thresh):
    out = []
    for a in annos:
        keep = [i for i, s in enumerate(a["score"]) if s >= thresh]
        out.append({k: v[keep] for k, v in a.items()})
    return out


def annos_from_lines(lines):
    """KITTI label lines (strings, as eval_rcnn.save_kitti_format writes them) -> annotation dict."""
    return _anno_from_rows([l.strip().split(" ") for l in lines if l.strip()])


def to_kitti_format(anno, extra=None):
    """Annotation -> the reference's 16-column %.2f text (kitti_common.py:293-304); ``extra``: a 17th column."""
    rows = []
    for i in range(len(anno["name"])):
        row = "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            anno["name"][i], anno["truncated"][i], anno["occluded"][i], anno["alpha"][i],
            anno["bbox"][i, 0], anno["bbox"][i, 1], anno["bbox"][i, 2], anno["bbox"][i, 3],
            anno["dimensions"][i, 1], anno["dimensions"][i, 2], anno["dimensions"][i, 0],
            anno["location"][i, 0], anno["location"][i, 1], anno["location"][i, 2], anno["rotation_y"][i], anno["score"][i])
        rows.append(row if extra is None else row + " %.2f" % extra[i])
    return "\n".join(rows)


def save_labels(annos, folder, ids, extras=None):
    assert len(annos) == len(ids)
    os.makedirs(folder, exist_ok=True)
    for n, (anno, i) in enumerate(zip(annos, ids)):
        with open(os.path.join(folder, "%06d.txt" % i), "w") as f:
            f.write(to_kitti_format(anno, None if extras is None else extras[n]))


def _bev_boxes(anno):
    return np.concatenate([anno["location"][:, [0, 2]], anno["dimensions"][:, [0, 2]], anno["rotation_y"][..., np.newaxis]], axis=1)


def _d3_boxes(anno):
    return np.concatenate([anno["location"], anno["dimensions"], anno["rotation_y"][..., np.newaxis]], axis=1)


def _cat(arrays, width, dtype=np.float64):
    parts = [np.asarray(a, dtype=dtype).reshape((-1, width) if width else (-1,)) for a in arrays]
    return np.ascontiguousarray(np.concatenate(parts, 0) if parts else np.zeros((0, width) if width else (0,), dtype))


class SplitSide:
    """One side (labels or detections) of a split as concatenated columns: ``off`` (n_img + 1) i64 and ``off32``, the same as i32
    (what the segmented launches take), ``code`` i8 class codes of the lower-cased names (lower-casing runs over the UNIQUE names),
    ``is_dc`` (the name is exactly "DontCare"), the f64 columns named by ``keys`` (all of COLUMNS, or the fewer a caller needs and
    its annotations hold, BOX_KEYS among them), ``box3d`` = _d3_boxes and ``bev`` = _bev_boxes in f32.  ``annos``: the list given."""
    COLUMNS = {"occluded": 0, "truncated": 0, "alpha": 0, "bbox": 4, "location": 3, "dimensions": 3, "rotation_y": 0, "score": 0}      # widths
    BOX_KEYS = ("location", "dimensions", "rotation_y")

    def __init__(self, annos, keys=tuple(COLUMNS)):
        self.annos, self.n_img = annos, len(annos)
        nums = np.array([len(a["name"]) for a in annos], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(nums)]).astype(np.int64)
        self.off32 = self.off.astype(np.int32)
        names = np.concatenate([np.asarray(a["name"], dtype=str).reshape(-1) for a in annos]) if self.n_img else np.zeros((0,), dtype=str)
        uniq, inv = np.unique(names, return_inverse=True) if names.size else (np.zeros((0,), dtype=str), np.zeros((0,), dtype=np.int64))
        self.code = np.array([CLASS_CODE.get(u.lower(), -1) for u in uniq], dtype=np.int8)[inv].reshape(-1)
        self.is_dc = np.array([u == "DontCare" for u in uniq], dtype=bool)[inv].reshape(-1)
        for key in keys:
            setattr(self, key, _cat([a[key] for a in annos], self.COLUMNS[key]))
        self.box3d = np.ascontiguousarray(np.concatenate([self.location, self.dimensions, self.rotation_y[:, None]], axis=1))
        self.bev = np.ascontiguousarray(self.box3d[:, [0, 2, 3, 5, 6]].astype(np.float32))

    def __len__(self):
        return int(self.off[-1])


class PreparedGT:
    """The ground-truth half of a split, parsed and tabulated once: pass it wherever ``gt_annos`` goes (both statistic paths take
    its columns) -- a sweep evaluates every checkpoint against the same one."""

    def __init__(self, gt_annos, ids=None):
        self.annos = list(gt_annos)
        self.ids = None if ids is None else list(ids)
        self.side = SplitSide(self.annos)

    def __len__(self):
        return len(self.annos)
