"""Generates tests/golden/g18_gt_database_ref.npz + g18_gt_database_ref.json: the GT database as the REFERENCE's own
tools/generate_gt_database.py writes it for tests/gt_tree.py's labelled fake tree.

RUN IN THE BUILD CONTAINER ONLY (runs the reference's tool in place, read-only, through ref_harness; needs oracle/_ref):
    python tests/golden/make_golden_gt_database.py
The tool is run as a script (runpy, ``sys.argv`` = --root <tree> --save_dir <tmp> --class_name <Car | People>), once per class name,
with ``roipool3d_cuda`` = oracle/_ref/roipool3d_ref.so, the reference's own roipool3d.cpp compiled for the host, so that
pts_in_boxes3d_cpu is the reference's.  Its pickle is read back here (the reference's Object3d class is importable in this
process) and is NOT kept: the fixture holds data only.

  g18_gt_database_ref.json   per class name: "file" (the pickle's base name), "stdout" (the printed lines; the save directory is
                             replaced by <save_dir>), "entries": per entry sample_id, cls_type, n (points), and "obj" = the
                             Object3d's __dict__ in its order as [name, type name, value] (arrays as lists, numpy scalars as
                             Python numbers)
  g18_gt_database_ref.npz    <class>_<i>_gt_box3d (7,) f32, <class>_<i>_points (n, 3) f32, <class>_<i>_intensity (n,) f32,
                             <class>_<i>_box2d / _pos: the obj's two arrays in their own dtype
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

CLASS_NAMES = ("Car", "People")


def type_name(v):
    return "%s[%s]" % (type(v).__name__, v.dtype) if isinstance(v, (np.ndarray, np.generic)) else type(v).__name__


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def run_tool(tree, class_name, out, meta):
    tool = os.path.join(H.REF, "tools", "generate_gt_database.py")
    with tempfile.TemporaryDirectory() as save_dir:
        argv, cwd = sys.argv, os.getcwd()
        sys.argv = [tool, "--root", tree, "--save_dir", save_dir, "--class_name", class_name]
        buf = io.StringIO()
        try:
            os.chdir(os.path.dirname(tool))
            with contextlib.redirect_stdout(buf):
                runpy.run_path(tool, run_name="__main__")
        finally:
            sys.argv = argv
            os.chdir(cwd)
        files = os.listdir(save_dir)
        assert len(files) == 1, files
        with open(os.path.join(save_dir, files[0]), "rb") as f:
            db = pickle.load(f)
        stdout = buf.getvalue().replace(save_dir, "<save_dir>").splitlines()
    entries = []
    for i, e in enumerate(db):
        assert sorted(e) == ["cls_type", "gt_box3d", "intensity", "obj", "points", "sample_id"]
        assert type(e["obj"]).__module__ == "lib.utils.object3d" and type(e["obj"]).__name__ == "Object3d"
        key = "%s_%d_" % (class_name, i)
        out[key + "gt_box3d"], out[key + "points"], out[key + "intensity"] = e["gt_box3d"], e["points"], e["intensity"]
        out[key + "box2d"], out[key + "pos"] = e["obj"].box2d, e["obj"].pos
        entries.append({"sample_id": plain(e["sample_id"]), "sample_id_type": type_name(e["sample_id"]), "cls_type": e["cls_type"],
                        "n": int(e["points"].shape[0]),
                        "obj": [[k, type_name(v), plain(v)] for k, v in e["obj"].__dict__.items()]})
    meta[class_name] = {"file": files[0], "stdout": stdout, "entries": entries}
    print(class_name, files[0], len(db), "entries, points per entry", [x["n"] for x in entries])


def main():
    H.install()
    from oracle import oracle
    ref = oracle.load_reference_roipool()
    assert ref is not None, "build oracle/_ref first: make -C oracle ref"
    sys.modules["roipool3d_cuda"] = ref
    sys.path.append(os.path.join(H.REF, "tools"))             # the tool's ``import _init_path``
    import gt_tree
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as tree:
        meta["sample_ids"] = gt_tree.write_gt_tree(tree)
        meta["tree_seed"] = gt_tree.TREE_SEED
        for class_name in CLASS_NAMES:
            run_tool(tree, class_name, out, meta)
    path = os.path.join(HERE, "g18_gt_database_ref.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "g18_gt_database_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
