"""Generates tests/golden/g26_few_shot_ref.json: the few-shot car split and the tree links as the REFERENCE's own scripts make them.

RUN IN THE BUILD CONTAINER ONLY (runs the reference's scripts/gen_car_split.py and pointrcnn/tools/generate_multi_data.py unmodified,
read-only, through runpy):
    python tests/golden/make_golden_car_split.py
It needs numpy only.  The fixture holds recorded data only:

  car1       {"A/train_car1.txt": text, "A/val_car1.txt", "B/train_car1.txt", "B/val_car1.txt"}: the four files gen_car_split.py writes
             for dataset_paths = (A, B) of tests/car_tree.py, in that order
  links      [[path relative to DST, link target relative to SRC]] of generate_multi_data.gen_data(A, DST), sorted by path
             ("." is SRC itself)

Shim: ``config_path`` (the reference's machine-local dataset table) is a stub module in sys.modules whose ``dataset_paths`` is the
ordered pair; nothing else is touched.

Asserted here, on the reference's run: A's train list is not in its input order (the shuffle shows); B's files differ from what a run
over B alone gives (the stream carries over from A); the files outside the device parser's grammar are among the kept ids (the
reference accepts a "\\r" and ``1.0`` in the occluded column).
"""
import json
import os
import runpy
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))

import car_tree


def run_gen_car_split(paths):
    cfg = types.ModuleType("config_path")
    cfg.dataset_paths = dict(paths)                                    # insertion order = the order of the run
    sys.modules["config_path"] = cfg
    try:
        runpy.run_path(os.path.join(REF, "scripts", "gen_car_split.py"), run_name="__main__")
    finally:
        del sys.modules["config_path"]


def main():
    tmp = tempfile.mkdtemp()
    a, b = car_tree.write_roots(os.path.join(tmp, "both"))
    run_gen_car_split([("A", a), ("B", b)])
    car1 = car_tree.car1_texts((a, b))
    alone = car_tree.write_root(os.path.join(tmp, "alone", "B"), "B")
    run_gen_car_split([("B", alone)])
    b_alone = car_tree.car1_texts((alone,), ("B",))

    for root in ("A", "B"):
        for split in car_tree.SPLITS:
            got = car1["%s/%s_car1.txt" % (root, split)].split("\n")
            assert sorted(got) == sorted(car_tree.with_car(root, split)), (root, split, got)
            assert set(car_tree.HOST_DECIDED[root][split]) <= set(got)
    a_train = car1["A/train_car1.txt"].split("\n")
    assert len(a_train) >= 5 and a_train != car_tree.with_car("A", "train"), a_train
    assert all(b_alone[k] != car1[k] for k in b_alone), "the stream did not carry over from A"

    sys.modules["config_path"] = types.ModuleType("config_path")
    sys.modules["config_path"].dataset_paths = {}
    ref = runpy.run_path(os.path.join(REF, "pointrcnn", "tools", "generate_multi_data.py"), run_name="generate_multi_data")
    del sys.modules["config_path"]
    dst = os.path.join(tmp, "linked")
    ref["gen_data"](a, dst)
    links = []
    for base, dirs, files in os.walk(dst):
        for name in dirs + files:
            p = os.path.join(base, name)
            if os.path.islink(p):
                links.append([os.path.relpath(p, dst), os.path.relpath(os.readlink(p), a)])
    links.sort()
    assert ["KITTI/ImageSets", "."] in links and ["KITTI/object/training/label_2", "training/label_2"] in links

    path = os.path.join(HERE, "g26_few_shot_ref.json")
    with open(path, "w") as f:
        json.dump({"car1": car1, "links": links}, f, indent=1, sort_keys=True)
        f.write("\n")
    for k in sorted(car1):
        print(k, car1[k].split("\n"), "| alone:", b_alone.get(k, "").split("\n") if k in b_alone else "-")
    print(links)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
