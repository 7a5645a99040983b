"""Generates tests/golden/g19_aug_scene_ref.npz + g19_aug_scene_ref.json: the augmented scenes as the REFERENCE's own
tools/generate_aug_scene.py writes them for tests/aug_tree.py's fake tree, from the database its own tools/generate_gt_database.py
makes of that tree.

RUN IN THE BUILD CONTAINER ONLY (runs the reference's tools in place, read-only, through ref_harness; needs oracle/_ref):
    python tests/golden/make_golden_aug_scene.py
Both tools run as scripts (runpy), ``Car`` with --aug_times 2 and ``People`` with --aug_times 1, with ``roipool3d_cuda`` =
oracle/_ref/roipool3d_ref.so (the reference's own roipool3d.cpp compiled for the host) and the rotated overlap from the CPU oracle
(ref_harness).  The pickles are NOT kept: the fixture holds data only.

  g19_aug_scene_ref.json   "numpy" (the version that made it: the y shift of the pasted points follows NEP 50), "sample_ids",
                           "tree_seed", and per class name: "db_points" (points per database entry), "bins" (file names), "labels"
                           (file name -> text), "split" (the split file's text), "log" (log_info.txt), "stdout" (the printed lines) --
                           the save directory replaced by <save_dir>, the database's by <db_dir> -- and "cases": what the run
                           contained, counted through wrappers around np.random.randint, boxes_iou3d_gpu and pts_in_boxes3d_cpu
  g19_aug_scene_ref.npz    <class>_<file name without .bin> (n, 4) f32: every rectified_data file
The run must contain at least one of each case the tree was built for (asserted below): change the tree, not the assertion.
"""
import contextlib
import io
import json
import os
import pickle
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402

RUNS = (("Car", 2), ("People", 1))
TRY_TIMES = 50


def run_script(tool, argv_tail, cwd):
    argv, old = sys.argv, os.getcwd()
    sys.argv = [tool] + argv_tail
    buf = io.StringIO()
    try:
        os.chdir(cwd)
        with contextlib.redirect_stdout(buf):
            runpy.run_path(tool, run_name="__main__")
    finally:
        sys.argv = argv
        os.chdir(old)
    return buf.getvalue()


class Watch:
    """Wrappers around the three calls the tool's branches show in."""

    def __init__(self):
        import lib.utils.iou3d.iou3d_utils as iou3d_utils
        import lib.utils.roipool3d.roipool3d_utils as roipool3d_utils
        self.iu, self.ru = iou3d_utils, roipool3d_utils
        self.saved = (np.random.randint, iou3d_utils.boxes_iou3d_gpu, roipool3d_utils.pts_in_boxes3d_cpu)
        self.scenes = []                       # per aug_one_scene call: {"draws": [...], "tests": [...]}
        self.removed = 0

    def __enter__(self):
        randint, iou, inside = self.saved

        def w_randint(*a, **k):
            v = randint(*a, **k)
            if a == (10, 15):
                self.scenes.append({"extra": int(v), "draws": [], "tests": [], "n_orig": None})
            else:
                self.scenes[-1]["draws"].append(int(v))
            return v

        def w_iou(a, b):
            r = iou(a, b)
            cur = self.scenes[-1]
            if cur["n_orig"] is None:
                cur["n_orig"] = int(b.shape[0])
            n0 = cur["n_orig"]
            rn = r.numpy()
            if rn.max() < 1e-8:
                what = "accepted"
            elif rn[0, :n0].max() >= 1e-8:
                what = "original"
            else:
                plain = b[n0:].clone()
                plain[:, 4] -= 0.5
                plain[:, 5] -= 0.5
                what = "enlargement" if iou(a, plain).numpy().max() < 1e-8 else "accepted_box"
            cur["tests"].append(what)
            return r

        def w_inside(pts, boxes):
            masks = inside(pts, boxes)
            self.removed += int(sum(int((m.numpy() == 1).sum()) for m in masks))
            return masks

        np.random.randint, self.iu.boxes_iou3d_gpu, self.ru.pts_in_boxes3d_cpu = w_randint, w_iou, w_inside
        return self

    def __exit__(self, *exc):
        np.random.randint, self.iu.boxes_iou3d_gpu, self.ru.pts_in_boxes3d_cpu = self.saved


def in_scope(centre, class_name):
    scope = ((-40, 40), (-1, 3), (0, 70.4)) if class_name == "Car" else ((-30, 30), (-1, 3), (0, 50))
    return all(lo <= float(v) <= hi for v, (lo, hi) in zip(centre, scope))


def count_cases(watch, db, class_name, n_scene_runs, labels, log):
    """What the run contained.  The exits of a try are recounted from the recorded draws (the loop of aug_one_scene over the entries'
    centres and point counts) and must agree with the number of overlap tests seen."""
    cases = {"accepted": 0, "rejected_original": 0, "rejected_enlargement_only": 0, "rejected_accepted_box": 0, "range_skip": 0,
             "few_points_skip": 0, "break": 0, "draws": 0, "scenes_skipped": n_scene_runs - len(watch.scenes),
             "original_points_removed": watch.removed}
    for sc in watch.scenes:
        cnt = 0
        assert len(db) - 1 not in sc["draws"]
        for idx in sc["draws"]:
            e = db[idx]
            if not in_scope(e["gt_box3d"][0:3], class_name):
                cases["range_skip"] += 1
            elif cnt > sc["extra"]:
                cases["break"] += 1
            elif len(e["points"]) < 5:
                cases["few_points_skip"] += 1
            else:
                cnt += 1
        assert cnt == len(sc["tests"]) and cnt <= 15, (cnt, len(sc["tests"]))
        assert len(sc["draws"]) == TRY_TIMES or cases["break"] > 0
        cases["draws"] += len(sc["draws"])
        for what, key in (("accepted", "accepted"), ("original", "rejected_original"), ("enlargement", "rejected_enlargement_only"),
                          ("accepted_box", "rejected_accepted_box")):
            cases[key] += sc["tests"].count(what)
    new_obj = sum(int(line.split("new_obj: ")[1].split(")")[0]) for line in log.splitlines() if "new_obj" in line)
    written = sum(sum(1 for ln in text.splitlines() if ln.startswith(class_name + " ") and len(ln.split(" ")[3].split(".")[1]) == 4)
                  for text in labels.values())
    assert new_obj == cases["accepted"]
    cases["labels_dropped_by_80_percent_rule"] = new_obj - written
    return cases


def run_class(tree, class_name, aug_times, out, meta, n_scenes):
    tools = os.path.join(H.REF, "tools")
    with tempfile.TemporaryDirectory() as work:
        db_dir, save_dir = os.path.join(work, "db"), os.path.join(work, "aug")
        run_script(os.path.join(tools, "generate_gt_database.py"), ["--root", tree, "--save_dir", db_dir, "--class_name", class_name], work)
        (db_file,) = os.listdir(db_dir)
        with open(os.path.join(db_dir, db_file), "rb") as f:
            db = pickle.load(f)
        with Watch() as watch:
            stdout = run_script(os.path.join(tools, "generate_aug_scene.py"),
                                ["--root", tree, "--save_dir", save_dir, "--class_name", class_name, "--aug_times", str(aug_times),
                                 "--gt_database_dir", os.path.join(db_dir, db_file)], work)
        fix = lambda s: s.replace(save_dir, "<save_dir>").replace(db_dir, "<db_dir>")
        bins = sorted(os.listdir(os.path.join(save_dir, "rectified_data")))
        for name in bins:
            out["%s_%s" % (class_name, name[:-4])] = np.fromfile(os.path.join(save_dir, "rectified_data", name), dtype=np.float32).reshape(-1, 4)
        labels = {}
        for name in sorted(os.listdir(os.path.join(save_dir, "aug_label"))):
            with open(os.path.join(save_dir, "aug_label", name)) as f:
                labels[name] = f.read()
        with open(os.path.join(save_dir, "train_aug.txt")) as f:
            split = f.read()
        with open(os.path.join(save_dir, "log_info.txt")) as f:
            log = fix(f.read())
        cases = count_cases(watch, db, class_name, n_scenes * aug_times, labels, log)
    meta[class_name] = {"aug_times": aug_times, "db_file": db_file, "db_points": [int(len(e["points"])) for e in db], "bins": bins,
                        "labels": labels, "split": split, "log": log, "stdout": fix(stdout).splitlines(), "cases": cases}
    print(class_name, len(db), "entries,", len(bins), "scenes written,", cases)
    return cases


def main():
    H.install()
    from oracle import oracle
    ref = oracle.load_reference_roipool()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    sys.modules["roipool3d_cuda"] = ref
    sys.path.append(os.path.join(H.REF, "tools"))             # the tools' ``import _init_path``
    import aug_tree
    out, meta = {}, {"numpy": np.__version__}
    with tempfile.TemporaryDirectory() as tree:
        meta["sample_ids"] = aug_tree.write_aug_tree(tree)
        meta["tree_seed"] = aug_tree.TREE_SEED
        cases = {c: run_class(tree, c, t, out, meta, len(meta["sample_ids"])) for c, t in RUNS}
    total = {k: sum(c[k] for c in cases.values()) for k in cases["Car"]}
    for key in ("accepted", "rejected_original", "rejected_enlargement_only", "range_skip", "few_points_skip", "break",
                "original_points_removed"):
        assert total[key] > 0, "the run contains no case of: %s" % key
    assert cases["People"]["scenes_skipped"] > 0 and cases["Car"]["scenes_skipped"] == 0
    meta["label_dropped_by_80_percent_rule"] = total["labels_dropped_by_80_percent_rule"] > 0
    path = os.path.join(HERE, "g19_aug_scene_ref.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "g19_aug_scene_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
