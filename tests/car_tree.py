"""Two small dataset-layout roots, A and B, for the few-shot car split (tests/golden g26, tests/test_car_split.py,
tests/test_gpu_car_split.py, tests/test_multi_data.py): ROOT/train.txt, ROOT/val.txt and ROOT/training/label_2/<id>.txt from the
literal label lines below.  Nothing here is random; the ids are listed out of sorted order.

The rule under test (scripts/gen_car_split.py is_valid_car): token 0 exactly ``Car``, bbox height y2 - y1 + 1 >= 25, truncated <= 0.5,
occluded <= 2 as floats.  Each scene is there for one edge of it; HOST_DECIDED names the files outside the device parser's grammar
(a "\\r", ``1.0`` in the occluded column), which the device path of car_split hands to the line-by-line restatement.
"""
import os


def line(name, truncated="0.00", occluded="0", y1="100.00", y2="160.00"):
    return "%s %s %s 1.57 300.00 %s 380.00 %s 1.50 1.60 3.90 1.00 1.65 20.00 0.10" % (name, truncated, occluded, y1, y2)


CAR = line("Car")
VAN = line("Van")
PED = line("Pedestrian", y1="90.00", y2="200.00")
DONTCARE = "DontCare -1 -1 -10 500.00 150.00 540.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10"

# root -> split -> [(id, file text, holds a valid car)] in the order of the split file
SCENES = {
    "A": {
        "train": [
            ("000007", CAR + "\n" + PED + "\n", True),                                           # a valid Car on the first line
            ("000002", VAN + "\n" + DONTCARE + "\n" + CAR + "\n", True),                         # ... behind a Van and a DontCare line
            ("000011", line("Car", y1="100.00", y2="124.00") + "\n", True),                      # bbox height exactly 25
            ("000004", line("Car", y1="100.00", y2="123.99") + "\n", False),                     # 24.99
            ("000009", line("Car", truncated="0.50") + "\n", True),
            ("000001", line("Car", truncated="0.51") + "\n" + VAN + "\n", False),
            ("000013", PED + "\n" + line("Car", occluded="2"), True),                            # the last line has no newline
            ("000010", VAN + "\r\n" + CAR + "\r\n", True),                                       # \r\n endings: host-decided
            ("000003", line("Car", occluded="1.0") + "\n", True),                                # a float there: host-decided
        ],
        "val": [
            ("000016", CAR + "\n", True),
            ("000005", line("Car", occluded="3") + "\n", False),
            ("000008", line("car") + "\n" + line("Cars") + "\n", False),                         # not exactly Car
            ("000014", DONTCARE + "\n" + CAR, True),
            ("000006", "", False),                                                               # an empty file
            ("000012", DONTCARE + "\n", False),                                                  # only DontCare
            ("000017", line("Car", truncated="0.25", occluded="1") + "\n", True),
        ],
    },
    "B": {
        "train": [
            ("000021", CAR + "\n", True),
            ("000020", VAN + "\n", False),                                                       # only Van
            ("000025", CAR + "\r\n", True),                                                      # host-decided
            ("000023", line("Car", y1="0.00", y2="24.00") + "\n" + line("Car", occluded="3") + "\n", True),
            ("000022", line("Car", occluded="3") + "\n" + line("Car", occluded="1.0") + "\n", True),   # host-decided
            ("000024", line("Car", truncated="0.51") + "\n", False),
            ("000028", DONTCARE + "\n" + DONTCARE + "\n" + CAR + "\n", True),
            ("000026", PED + "\n" + CAR + "\n" + VAN + "\n", True),
            ("000027", line("Cars") + "\n", False),
        ],
        "val": [
            ("000031", CAR + "\n", True),
            ("000030", "", False),
            ("000033", VAN + "\n" + CAR + "\n", True),
            ("000032", line("Car", occluded="2") + "\n", True),
            ("000034", line("Car", occluded="3"), False),
        ],
    },
}
HOST_DECIDED = {"A": {"train": ["000010", "000003"], "val": []}, "B": {"train": ["000025", "000022"], "val": []}}
SPLITS = ("train", "val")
OTHER_DIRS = {"A": ("velodyne", "calib", "image_2", "planes"), "B": ("velodyne", "calib")}     # empty directories: what multi_data links


def listed(root, split):
    return [i for i, _text, _ok in SCENES[root][split]]


def with_car(root, split):
    """the ids the rule keeps, in list order (before the shuffle)"""
    return [i for i, _text, ok in SCENES[root][split] if ok]


def write_root(path, root):
    """Root ``root`` ("A" or "B") in the dataset layout under ``path``"""
    label_dir = os.path.join(path, "training", "label_2")
    for sub in ("label_2",) + OTHER_DIRS[root]:
        os.makedirs(os.path.join(path, "training", sub), exist_ok=True)
    for split in SPLITS:
        with open(os.path.join(path, split + ".txt"), "w") as f:
            f.write("".join(i + "\n" for i in listed(root, split)))
        for i, text, _ok in SCENES[root][split]:
            with open(os.path.join(label_dir, i + ".txt"), "wb") as f:                           # bytes: the \r\n stay
                f.write(text.encode("ascii"))
    return path


def write_roots(base):
    """-> (path of A, path of B) under ``base``"""
    return tuple(write_root(os.path.join(str(base), name), name) for name in ("A", "B"))


def car1_texts(paths, names=("A", "B")):
    """{"A/train_car1.txt": text, ...} of the roots at ``paths``"""
    out = {}
    for path, name in zip(paths, names):
        for split in SPLITS:
            with open(os.path.join(path, split + "_car1.txt")) as f:
                out["%s/%s_car1.txt" % (name, split)] = f.read()
    return out
