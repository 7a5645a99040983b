"""Generates tests/golden/g17_eval_transforms_ref.npz: the REFERENCE's own evaluate/evaluate.py::evaluate (old metric, COCO result,
output transformations) on CPU.

RUN IN THE BUILD CONTAINER ONLY (needs /root/reference, read-only):   python tests/golden/make_golden_eval_transforms.py

Same shims as make_golden.py::g10: ``numba.jit`` is the identity, an empty ``skimage`` stand-in serves kitti_common's unused import, and
the evaluator's ``rotate_iou`` dependency is the reference's own evaluate/rotate_iou.py on the numba.cuda interpreter of numba_shim.py
(results are memoised on the input bytes: every configuration pairs the same boxes several times).  For ``reverse_align`` a stand-in
``config_path`` module in sys.modules points the reference at two statistics files of the temporary tree.

The fixture is DATA: input label / detection / plane lines, the two statistics files, ids; per configuration the result text, the AP
arrays and every file the reference wrote (as strings); the per-image (max, argmax) of calculate_iou_partly(..., 1); the in-memory
dimensions / location after align_size and align_front; the old metric's clean_data lists; and the branch counts asserted below.

TWO DEVIATIONS, recorded in the fixture as ``coco_unpatched_error``: get_coco_eval_result raises in both reference modules as shipped.
(1) do_coco_style_eval hands np.linspace a float sample count (eval2.py:617), which the numpy of the reference's day accepted and
today's does not: np.linspace is wrapped to convert the count while the reference runs.  (2) With that out of the way,
do_coco_style_eval (eval2.py:618, eval_old.py:608) calls ``do_eval(gt, dt, classes, min_overlaps, compute_aos)`` -- one argument short
since ``dataset`` was added to do_eval.  The generator first records both errors, then wraps the module's do_eval with an adapter that
accepts the five-argument call and passes the dataset name in the fourth place; everything else (linspace thresholds, the mean over
them, the text) is the reference's own code.
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden as MG  # noqa: E402

REF_EVAL = "/root/reference/evaluate"
SRC_STATS = {"length": {"mean": 3.88, "std": 0.43}, "height": {"mean": 1.53, "std": 0.14}, "width": {"mean": 1.63, "std": 0.10}}
DST_STATS = {"length": {"mean": 4.80, "std": 0.55}, "height": {"mean": 1.78, "std": 0.18}, "width": {"mean": 2.10, "std": 0.16}}
CONFIGS = [
    ("new", {}),
    ("old", {"metric": "old"}),
    ("old_waymo", {"metric": "old", "dataset": "waymo"}),
    ("coco_new", {"coco": True}),
    ("coco_old", {"metric": "old", "coco": True}),
    ("toground", {"toground": True}),
    ("rescale2", {"rescale_pred": 2}),
    ("align_size", {"align_size": True}),
    ("align_front", {"align_front": True}),
    ("reverse_align", {"reverse_align": True}),
    ("size_ground_save", {"align_size": True, "toground": True, "direct_save": True}),
    ("output_iou", {"output_iou": True}),
]


def label_sets():
    """make_golden.synth_label_sets() plus exact duplicates of a ground-truth line in four images (ties for the lowest-index rule);
    image 5, which has no objects, also loses its DontCare regions: a label file without a line, against detections."""
    gts, dts = MG.synth_label_sets()
    gts[5] = []
    assert len(dts[5]) > 0 and len(dts[7]) == 0
    for i in (10, 20, 30, 40):
        cars = [l for l in gts[i] if l.startswith("Car")]
        gts[i] = gts[i] + [cars[0]]
    return gts, dts


def plane_files(n, seed=17):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a, c = rng.normal(0, 0.01, 2)
        out.append("# Plane\nWidth 4\nHeight 1\n%.6e %.6e %.6e %.6e" % (a, -1.0 + rng.normal(0, 1e-3), c, 1.65 + rng.normal(0, 0.05)))
    return out


def write_tree(tmp, gts, dts, planes):
    """<tmp>/src_kitti/training/{label_2,planes}, <tmp>/src_kitti/val.txt, <tmp>/out_waymo/run/data, two statistics folders."""
    lab = os.path.join(tmp, "src_kitti", "training", "label_2")
    pla = os.path.join(tmp, "src_kitti", "training", "planes")
    res = os.path.join(tmp, "out_waymo", "run", "data")
    for d in (lab, pla, res, os.path.join(tmp, "stats_a"), os.path.join(tmp, "stats_b")):
        os.makedirs(d)
    for i in range(len(gts)):
        for d, text in ((lab, "\n".join(gts[i])), (pla, planes[i]), (res, "\n".join(dts[i]))):
            with open(os.path.join(d, "%06d.txt" % i), "w") as f:
                f.write(text)
    with open(os.path.join(tmp, "src_kitti", "val.txt"), "w") as f:
        f.write("\n".join("%06d" % i for i in range(len(gts))))
    for d, s in (("stats_a", SRC_STATS), ("stats_b", DST_STATS)):
        with open(os.path.join(tmp, d, "label_normal_val.json"), "w") as f:
            json.dump(s, f)
    return lab, res


def written_files(tmp):
    """Everything under <tmp>/out_waymo except the input folder: relative names and texts (pickles: name only)."""
    names, texts = [], []
    base = os.path.join(tmp, "out_waymo")
    for root, _, files in sorted(os.walk(base)):
        for fn in sorted(files):
            rel = os.path.relpath(os.path.join(root, fn), base)
            if rel.startswith(os.path.join("run", "data") + os.sep):
                continue
            names.append(rel)
            if fn.endswith(".pkl"):
                texts.append("")
            else:
                with open(os.path.join(root, fn)) as f:
                    texts.append(f.read())
    return np.array(names), np.array(texts)


def ap_arrays(ret):
    """ret['result'][class] -> (n_overlap, 3, n_difficulty) in the order bbox, bev, 3d."""
    return np.stack([np.stack([v["mAPbbox"], v["mAPbev"], v["mAP3d"]], 0) for v in ret["result"][0].values()], 0)


def front_branches(dt, gt, val, idx):
    """Which branch of evaluate.py:209-229 a detection takes: -1 not aligned, else bit 0 first shift, bit 1 its 0 < alpha choice,
    bit 2 second shift, bit 3 its |alpha| < pi / 2 choice."""
    out = np.full(len(val), -1, dtype=np.int64)
    for j in range(len(val)):
        if val[j] > 0.2:
            dist = np.linalg.norm(dt["location"][j, :])
            alpha = dt["alpha"][j]
            alpha = np.arctan2(np.sin(alpha), np.cos(alpha))
            code = 0
            if np.abs(np.sin(alpha)) * dist > dt["dimensions"][j, 2] / 2.0:
                code |= 1 | (2 if 0 < alpha else 0)
            if np.abs(np.cos(alpha)) * dist > dt["dimensions"][j, 1] / 2.0:
                code |= 4 | (8 if -np.pi / 2.0 < alpha < np.pi / 2.0 else 0)
            out[j] = code
    return out


_np_linspace = np.linspace


def _linspace_int_num(start, stop, num=50, *a, **k):
    """numpy of the reference's day accepted a float sample count (class_to_range holds [0.5, 0.95, 10] as one float array)."""
    return _np_linspace(start, stop, int(num), *a, **k)


def main():
    import numba_shim as NS
    riou, cu = NS.import_reference_rotate_iou()
    calls = {"n": 0, "pairs": 0, "undefined": 0, "memo_hits": 0}
    memo = {}
    _ref_eval = riou.rotate_iou_gpu_eval

    def counted(boxes, query_boxes, criterion=-1, device_id=0):
        key = (np.asarray(boxes).tobytes(), np.asarray(query_boxes).tobytes(), np.asarray(boxes).dtype.str, int(criterion))
        if key in memo:
            calls["memo_hits"] += 1
            return memo[key].copy()
        out = _ref_eval(boxes, query_boxes, criterion, device_id)
        calls["n"] += 1
        calls["pairs"] += out.size
        if out.size and cu.last_undefined is not None:
            calls["undefined"] += int(cu.last_undefined.sum())
        memo[key] = out.copy()
        return out
    riou.rotate_iou_gpu_eval = counted
    if "skimage" not in sys.modules:
        sk = types.ModuleType("skimage")
        sk.io = types.ModuleType("skimage.io")
        sys.modules["skimage"], sys.modules["skimage.io"] = sk, sk.io
    sys.path.insert(0, REF_EVAL)
    eval2 = importlib.import_module("eval2")
    eval_old = importlib.import_module("eval_old")
    kc = importlib.import_module("kitti_common")
    ev = importlib.import_module("evaluate")
    assert ev.__file__.startswith(REF_EVAL) and eval_old.__file__.startswith(REF_EVAL)
    assert eval2.rotate_iou_gpu_eval is counted and eval_old.rotate_iou_gpu_eval is counted

    loaded = []
    _get = kc.get_label_annos

    def capturing(folder, ids=None):
        annos = _get(folder, ids)
        loaded.append(annos)                       # evaluate() transforms these lists in place
        return annos
    kc.get_label_annos = capturing

    gts, dts = label_sets()
    planes = plane_files(len(gts))
    n_img = len(gts)
    out = {"gt_lines": np.array(["\n".join(l) for l in gts]), "dt_lines": np.array(["\n".join(l) for l in dts]),
           "plane_lines": np.array(planes), "src_stats": np.array(json.dumps(SRC_STATS)), "dst_stats": np.array(json.dumps(DST_STATS)),
           "configs": np.array([c for c, _ in CONFIGS]), "config_kwargs": np.array([json.dumps(k) for _, k in CONFIGS])}

    # the COCO result as shipped: one argument short
    with tempfile.TemporaryDirectory(prefix="g17_") as tmp:
        lab, res = write_tree(tmp, gts, dts, planes)
        g, d = _get(lab, list(range(n_img))), _get(res, list(range(n_img)))
    errors = []
    for mod in (eval2, eval_old):
        for shim in (False, True):
            np.linspace = _linspace_int_num if shim else _np_linspace
            try:
                mod.get_coco_eval_result(g, d, 0)
                errors.append("no error")
            except Exception as e:                 # noqa: BLE001
                errors.append("%s: %s" % (type(e).__name__, e))
    assert all(e != "no error" for e in errors), errors
    out["coco_unpatched_error"] = np.array(errors)      # [eval2 as shipped, eval2 with the linspace shim, eval_old ..., eval_old ...]
    print("coco as shipped:", errors)

    current = {"dataset": "kitti"}
    for mod in (eval2, eval_old):       # get_official_eval_result calls do_eval with six arguments, do_coco_style_eval with five
        def both(*a, _six=mod.do_eval):
            if len(a) == 5:
                return _six(a[0], a[1], a[2], current["dataset"], a[3], a[4])
            return _six(*a)
        mod.do_eval = both

    np.linspace = _linspace_int_num
    for name, kw in CONFIGS:
        with tempfile.TemporaryDirectory(prefix="g17_") as tmp:
            lab, res = write_tree(tmp, gts, dts, planes)
            cp = types.ModuleType("config_path")
            cp.dataset_paths = {"kitti": os.path.join(tmp, "stats_a"), "waymo": os.path.join(tmp, "stats_b")}
            sys.modules["config_path"] = cp
            current["dataset"] = kw.get("dataset", "kitti")
            del loaded[:]
            r = ev.evaluate(res, dataset_path=os.path.join(tmp, "src_kitti"), **kw)
            sys.modules.pop("config_path", None)
            if kw.get("coco"):
                out["text_" + name] = np.array(r)
                mod = eval_old if kw.get("metric") == "old" else eval2
                rng = np.zeros([3, 3, 1])
                rng[:, :, 0] = np.array([0.5, 0.95, 10])[:, np.newaxis]
                arrs = mod.do_coco_style_eval(loaded[1], loaded[0], [0], rng, True)
                out["ap_" + name] = np.stack(arrs[:3], 0)                 # (3 kinds, 1 class, n_difficulty)
            elif r is not None:
                out["text_" + name] = np.array(r[0])
                out["ap_" + name] = ap_arrays(r[1])
            out["files_%s_names" % name], out["files_%s_texts" % name] = written_files(tmp)
            if name in ("align_size", "align_front"):
                dt_after = loaded[0]
                out["dims_after_" + name] = np.concatenate([a["dimensions"] for a in dt_after], 0)
                out["loc_after_" + name] = np.concatenate([a["location"] for a in dt_after], 0)
            print("g17 %-17s %s | files %d | %s" % (name, (str(out.get("text_" + name, "")).split("\n") + ["", "", "", ""])[2],
                                                   len(out["files_%s_names" % name]), calls))

    # best matches: calculate_iou_partly(dt, gt, 1) as evaluate.py:135,188,201 calls it
    with tempfile.TemporaryDirectory(prefix="g17_") as tmp:
        lab, res = write_tree(tmp, gts, dts, planes)
        gt_annos, dt_annos = _get(lab, list(range(n_img))), _get(res, list(range(n_img)))
    overlaps = eval2.calculate_iou_partly(dt_annos, gt_annos, 1)[0]
    dv, di, gv, gi, br = [], [], [], [], []
    ties = 0
    for i, o in enumerate(overlaps):
        n, k = len(dt_annos[i]["name"]), len(gt_annos[i]["name"])
        assert o.shape == (n, k) and o.dtype == np.float64
        if n > 0 and k > 0:
            dv.append(np.max(o, axis=1)); di.append(np.argmax(o, axis=1))
            gv.append(np.max(o, axis=0)); gi.append(np.argmax(o, axis=0))
            ties += int(np.count_nonzero(((o == dv[-1][:, None]).sum(1) > 1) & (dv[-1] > 0)))
        else:
            dv.append(np.zeros(n)); di.append(np.full(n, -1, dtype=np.int64))
            gv.append(np.zeros(k)); gi.append(np.full(k, -1, dtype=np.int64))
        br.append(front_branches(dt_annos[i], gt_annos[i], dv[-1], di[-1]))
    out["bm_dt_val"], out["bm_dt_idx"] = np.concatenate(dv), np.concatenate(di).astype(np.int64)
    out["bm_gt_val"], out["bm_gt_idx"] = np.concatenate(gv), np.concatenate(gi).astype(np.int64)
    out["front_branch"] = np.concatenate(br)

    # the old metric's per-image bookkeeping for two datasets
    for ds in ("kitti", "waymo"):
        nv, ig, idt = [], [], []
        for diff in (0, 1, 2):
            for i in range(n_img):
                a, b, c, _ = eval_old.clean_data(gt_annos[i], dt_annos[i], 0, ds, diff)
                nv.append(a); ig += list(b); idt += list(c)
        out["old_clean_%s_num_valid" % ds] = np.array(nv, dtype=np.int64)
        out["old_clean_%s_ignored_gt" % ds] = np.array(ig, dtype=np.int64)
        out["old_clean_%s_ignored_dt" % ds] = np.array(idt, dtype=np.int64)

    # the inputs must reach every branch
    val, b = out["bm_dt_val"], out["front_branch"]
    counts = {
        "dt_above": int(np.count_nonzero(val > 0.2)), "dt_at_or_below": int(np.count_nonzero(val <= 0.2)),
        "shift1_alpha_pos": int(np.count_nonzero((b >= 0) & (b & 1 > 0) & (b & 2 > 0))),
        "shift1_alpha_neg": int(np.count_nonzero((b >= 0) & (b & 1 > 0) & (b & 2 == 0))),
        "shift2_inner": int(np.count_nonzero((b >= 0) & (b & 4 > 0) & (b & 8 > 0))),
        "shift2_outer": int(np.count_nonzero((b >= 0) & (b & 4 > 0) & (b & 8 == 0))),
        "img_without_dt": sum(1 for a in dt_annos if len(a["name"]) == 0),
        "img_without_gt": sum(1 for a in gt_annos if len(a["name"]) == 0),
        "exact_ties": ties,
        "old_gt_kitti_vs_waymo": int(np.count_nonzero(out["old_clean_kitti_ignored_gt"] != out["old_clean_waymo_ignored_gt"])),
        "old_dt_kitti_vs_waymo": int(np.count_nonzero(out["old_clean_kitti_ignored_dt"] != out["old_clean_waymo_ignored_dt"])),
    }
    print("g17 counts:", counts)
    assert counts["dt_above"] >= 20 and counts["dt_at_or_below"] >= 5, counts
    assert all(v >= 1 for v in counts.values()), counts
    out["counts"] = np.array(json.dumps(counts))
    assert calls["n"] > 0 and calls["undefined"] == 0, calls
    assert sys.modules["rotate_iou"].__file__.startswith("/root/reference/")
    out["riou_source"] = np.array("reference evaluate/rotate_iou.py via tests/golden/numba_shim.py: %(n)d calls, %(pairs)d pairs" % calls)
    path = os.path.join(HERE, "g17_eval_transforms_ref.npz")
    np.savez_compressed(path, **out)
    print("g17: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
