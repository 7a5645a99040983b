"""The reference evaluator's output transformations (evaluate/evaluate.py:17-81, 114-275): grounding on the road planes,
re-scaling, size / front alignment against the best-overlapping ground truth (``device="cuda"``: ``prcnn_eval_align`` of
csrc/eval_match.hip after the fused best-match launch; ``"cpu"``: the reference's statements over numpy's best match), statistical
mapping of the ground-truth sizes, the per-box overlap columns and the result files beside the run folder."""
import json
import os
import pickle

import numpy as np

from . import _lib
from .kitti_annos import SplitSide, save_labels
from .kitti_overlaps import _best_match_device, best_match

ALIGN_MIN_OVERLAP = 0.2          # evaluate.py:196,209: a detection is aligned when its best BEV overlap exceeds this


def read_plane(fname):
    with open(fname) as f:
        return np.array([float(v) for v in f.readlines()[-1].split(" ")])


def annos_to_ground(annos, planes_dir, ids):
    """Drop every box onto its image's ground plane a x + b y + c z + d = 0: the last line of <planes_dir>/<id>.txt (evaluate.py:17-35)."""
    for anno, i in zip(annos, ids):
        plane = read_plane(os.path.join(planes_dir, "%06d.txt" % i))
        anno["location"][:, 1] -= (-plane[3] - plane[0] * anno["location"][:, 0] - plane[2] * anno["location"][:, 2]) / plane[1]
    return annos


def rescale_pred(annos, ratio):
    for anno in annos:
        anno["dimensions"] *= ratio
    return annos


def _align(dt_annos, gt_annos, mode, device, device_id):
    """align_size (mode 0) / align_front (mode 1), in place.  -> per image branch codes (-1 untouched; bits as prcnn_eval_align)."""
    if device == "cuda":
        import torch
        dt, gt = SplitSide(dt_annos, SplitSide.BOX_KEYS + ("alpha",)), SplitSide(gt_annos, SplitSide.BOX_KEYS)
        m = _best_match_device(dt, gt, device_id, columns=False)
        up = lambda column: torch.from_numpy(column).to(m["row_val"].device)
        loc, dim, gdim = up(dt.location), up(dt.dimensions), up(gt.dimensions)
        alpha, ry = up(dt.alpha), up(dt.rotation_y)
        branch = torch.empty_like(m["row_idx"])
        with torch.cuda.device(branch.device):
            _lib.call("prcnn_eval_align", dt.n_img, len(dt), m["box_off"].data_ptr(), m["q_off"].data_ptr(), loc.data_ptr(),
                      dim.data_ptr(), alpha.data_ptr(), ry.data_ptr(), gdim.data_ptr(), m["row_val"].data_ptr(), m["row_idx"].data_ptr(),
                      int(mode), branch.data_ptr(), _lib.current_stream(loc))
        loc, dim, branch, off = loc.cpu().numpy(), dim.cpu().numpy(), branch.cpu().numpy().astype(np.int64), dt.off
        for i, anno in enumerate(dt_annos):
            anno["location"][...] = loc[off[i]:off[i + 1]]
            anno["dimensions"][...] = dim[off[i]:off[i + 1]]
        return [branch[off[i]:off[i + 1]] for i in range(dt.n_img)]
    branches = []
    for dt, gt, (val, idx) in zip(dt_annos, gt_annos, best_match(dt_annos, gt_annos, device, device_id)[0]):
        code = np.full(len(val), -1, dtype=np.int64)
        for j in range(len(val)):
            if val[j] > ALIGN_MIN_OVERLAP:
                code[j] = 0
                if mode == 1:                          # evaluate.py:210-228
                    dist = np.linalg.norm(dt["location"][j, :])
                    alpha = dt["alpha"][j]
                    alpha = np.arctan2(np.sin(alpha), np.cos(alpha))
                    if np.abs(np.sin(alpha)) * dist > dt["dimensions"][j, 2] / 2.0:
                        shift = (dt["dimensions"][j, 2] - gt["dimensions"][idx[j], 2]) / 2.0
                        angle = -dt["rotation_y"][j] if 0 < alpha else -dt["rotation_y"][j] + np.pi
                        code[j] |= 1 | (2 if 0 < alpha else 0)
                        dt["location"][j, 0] += shift * np.cos(angle)
                        dt["location"][j, 2] += shift * np.sin(angle)
                    if np.abs(np.cos(alpha)) * dist > dt["dimensions"][j, 1] / 2.0:
                        shift = (dt["dimensions"][j, 1] - gt["dimensions"][idx[j], 1]) / 2.0
                        inner = -np.pi / 2.0 < alpha < np.pi / 2.0
                        angle = -dt["rotation_y"][j] - np.pi / 2.0 if inner else -dt["rotation_y"][j] + np.pi / 2.0
                        code[j] |= 4 | (8 if inner else 0)
                        dt["location"][j, 0] += shift * np.cos(angle)
                        dt["location"][j, 2] += shift * np.sin(angle)
                dt["dimensions"][j, :] = gt["dimensions"][idx[j], :]
        branches.append(code)
    return branches


def align_size(dt_annos, gt_annos, device="cuda", device_id=0):
    """Every detection whose best BEV overlap exceeds 0.2 takes the size of that ground-truth box (evaluate.py:187-197)."""
    _align(dt_annos, gt_annos, 0, device, device_id)
    return dt_annos


def align_front(dt_annos, gt_annos, device="cuda", device_id=0):
    """... and is first moved so that its faces towards the camera stay where they were (evaluate.py:200-229)."""
    _align(dt_annos, gt_annos, 1, device, device_id)
    return dt_annos


def get_scale_map(src, dst, form="regular"):
    """Map (n,3) dimensions (l, h, w) from the source statistics to the destination's (evaluate.py:58-81).  src / dst: the
    ``label_stats_<split>.json`` dicts of ``stat_norm stats`` (length / height / width -> mean, std)."""
    keys = ("length", "height", "width")
    forms = {"regular": lambda x, s, d: x - s["mean"] + d["mean"], "log": lambda x, s, d: x / s["mean"] * d["mean"],
             "gaussian": lambda x, s, d: (x - s["mean"]) / s["std"] * d["std"] + d["mean"]}
    if form not in forms:
        raise ValueError("scale_map %r is none of regular, gaussian, log" % (form,))
    f = forms[form]
    return lambda x: np.stack([f(x[:, c], src[key], dst[key]) for c, key in enumerate(keys)], axis=1)


def _stats(s):
    if isinstance(s, dict):
        return s
    with open(s) as f:
        return json.load(f)


def reverse_align(gt_annos, src_stats, dst_stats, scale_map="regular"):
    """Statistical normalization applied to the ground-truth sizes (evaluate.py:232-249); statistics as dicts or file names."""
    mapping = get_scale_map(_stats(src_stats), _stats(dst_stats), scale_map)
    for anno in gt_annos:
        if len(anno["name"]) > 0:
            anno["dimensions"] = mapping(anno["dimensions"])
    return gt_annos


def write_with_iou(dt_annos, gt_annos, parent, ids, device="cuda", device_id=0):
    """<parent>/with_iou: the detections with their best BEV overlap as a 17th column; <parent>/with_iou_gt: the ground truth
    with theirs (evaluate.py:130-185)."""
    dt_matches, gt_matches = best_match(dt_annos, gt_annos, device, device_id)
    save_labels(dt_annos, os.path.join(parent, "with_iou"), ids, [v for v, _ in dt_matches])
    save_labels(gt_annos, os.path.join(parent, "with_iou_gt"), ids, [v for v, _ in gt_matches])


def direct_save(result_path, text, result, toground=False, align_size=False, reverse_align=False, adapted=False):
    """Result text and per-class dict beside the run folder: <run>_val20[_ground][_align_size][_reverse_align][_adapted].txt / .pkl
    in the folder that holds <run>/<result folder> (evaluate.py:258-274).  -> the path without extension."""
    run = os.path.dirname(result_path)
    tags = ((toground, "_ground"), (align_size, "_align_size"), (reverse_align, "_reverse_align"), (adapted, "_adapted"))
    base = os.path.join(os.path.dirname(run), os.path.basename(run) + "_val20" + "".join(tag for on, tag in tags if on))
    with open(base + ".pkl", "wb") as f:
        pickle.dump(result, f)
    with open(base + ".txt", "w") as f:
        f.write(text)
    return base
