"""The few-shot car split of KITTI-format trees (reference: scripts/gen_car_split.py): for every root, for ``train`` then ``val``, the
ids of ``<split>.txt`` whose label file holds at least one valid car, shuffled, written to ``<split>_car1.txt`` beside the split file
(names joined by "\\n", no trailing newline; an existing file is overwritten).  ``train_car1.txt`` is what --subsample reads
(scene_batch.sample_id_list).

  python -m 3d_adapt_auto_driving_amd.car_split ROOT [ROOT ...] [--layout dataset|pointrcnn] [--parse_device cpu|cuda]

Layouts: ``dataset`` (the reference's, and what ``stat_norm convert`` writes) is ROOT/<split>.txt and ROOT/training/label_2/<id>.txt;
``pointrcnn`` is ROOT/KITTI/ImageSets/<split>.txt and ROOT/KITTI/object/training/label_2.  On a tree that multi_data.py linked the two
name the same files.

A valid line is the reference's is_valid_car, to the letter: the line is strip()ped and split(" "); token 0 is exactly ``Car``;
float(x[7]) - float(x[5]) + 1 >= 25 (f64, in that order); float(x[1]) <= 0.5; float(x[2]) <= 2 (a float: ``1.0`` in the occluded column
is legal HERE, though the label parsers of this package reject it).  A ``Car`` line with fewer than 8 tokens or a token that is no float
makes the reference raise; here it raises ValueError with the file's name, on both paths, before any file is written (every list is
made first, then all are written).

The random stream is the reference's: np.random.seed(19260817) ONCE per run, then one legacy np.random.shuffle per Python list of kept
names, in the order above.  The stream runs on across splits and roots, so the files of the second root depend on how many ids the
first root kept: ``car_split A B`` and ``car_split B`` write different files for B.  (The global legacy stream is seeded and used, as
the reference does; nothing else in this package draws from it.)

Two paths, equal byte for byte.  ``--parse_device cpu`` is the restatement line by line: the checker and the definition.
``--parse_device cuda`` sends each split's label files through kitti_annos.read_texts + parse_texts(texts, "cuda") -- one call per split,
csrc/kitti_parse.hip -- and evaluates the rule in whole-array numpy over the returned columns (off, the name tokens' bytes, truncated,
occluded, bbox).  Inside the parser's regular grammar a line's tokens are those of strip().split(" ") and every value is Python's
float().  A file outside that grammar (a "\\r", a blank line, ``1.0`` in the occluded column, 7 tokens, ...) is decided by the
restatement for that file alone; ``host_files`` counts them.  ``cuda`` without a usable GPU raises kitti_annos.ParseDeviceError; nothing
falls back.  Speed: profiles/car_split_probe.md; on files in the page cache the cuda path is the slower one (its time is read_texts).
"""
import argparse
import io
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SEED = 19260817
SPLITS = ("train", "val")
LAYOUTS = ("dataset", "pointrcnn")
MIN_HEIGHT, MAX_TRUNCATED, MAX_OCCLUDED = 25, 0.5, 2


def layout_dirs(root, layout="dataset"):
    """-> (the directory of the split files, the label directory)"""
    if layout == "dataset":
        return root, os.path.join(root, "training", "label_2")
    if layout == "pointrcnn":
        return os.path.join(root, "KITTI", "ImageSets"), os.path.join(root, "KITTI", "object", "training", "label_2")
    raise ValueError("car_split: --layout %r is neither 'dataset' nor 'pointrcnn'" % (layout,))


def is_valid_car(x):
    """gen_car_split.py:8-14 on the tokens of one line"""
    if x[0] != "Car":
        return False
    height = float(x[7]) - float(x[5]) + 1
    truncated = float(x[1])
    occluded = float(x[2])
    return height >= MIN_HEIGHT and truncated <= MAX_TRUNCATED and occluded <= MAX_OCCLUDED


def has_car(lines, label_file):
    """Does any of a label file's lines (str, as readlines() gives them) hold a valid car?  Every line is looked at, as the reference's
    filter does, so a malformed Car line raises wherever it stands."""
    found = False
    for k, line in enumerate(lines):
        try:
            found = is_valid_car(line.strip().split(" ")) or found
        except (IndexError, ValueError) as e:
            raise ValueError("car_split: %s line %d: %s: %s" % (label_file, k + 1, type(e).__name__, e)) from e
    return found


def _file_lines(label_file):
    with open(label_file) as f:
        return f.readlines()


def _text_lines(blob):
    """the lines open(label_file).readlines() gives for these bytes"""
    return io.TextIOWrapper(io.BytesIO(bytes(blob))).readlines()


def _read_texts(label_dir, names):
    """kitti_annos.read_texts for ids in its own %06d form; any other name the reference would open is read the same way"""
    from . import kitti_annos
    if all(len(x) == 6 and x.isdigit() for x in names):
        return kitti_annos.read_texts(label_dir, [int(x) for x in names])

    def read(name):
        with open(os.path.join(label_dir, name + ".txt"), "rb") as f:
            return f.read()
    with ThreadPoolExecutor(max_workers=16) as pool:
        return list(pool.map(read, names))


def car_mask_columns(side):
    """A parsed side (kitti_annos.parse_texts) -> bool per file: it holds a row that is a valid car.  Whole-array numpy over the columns."""
    text, span = side._text, side._name_span                     # the bytes the name spans point into
    at = lambda k: text[np.minimum(span[:, 0] + k, max(0, len(text) - 1))] if len(text) else np.zeros(len(span), np.uint8)
    is_car = (span[:, 1] == 3) & (at(0) == ord("C")) & (at(1) == ord("a")) & (at(2) == ord("r"))
    valid = is_car & (side.bbox[:, 3] - side.bbox[:, 1] + 1 >= MIN_HEIGHT) & (side.truncated <= MAX_TRUNCATED) & (side.occluded <= MAX_OCCLUDED)
    file_of_row = np.repeat(np.arange(side.n_img), np.diff(side.off))
    return np.bincount(file_of_row[valid], minlength=side.n_img) > 0


def kept_names(root, split, layout="dataset", parse_device="cpu"):
    """-> (the names of <split>.txt, those whose label file has a valid car in list order, the files the restatement decided on the
    device path)"""
    sets, label_dir = layout_dirs(root, layout)
    with open(os.path.join(sets, split + ".txt")) as f:
        names = [x.strip() for x in f.readlines()]
    path = lambda name: os.path.join(label_dir, name + ".txt")
    if parse_device == "cpu":
        return names, [x for x in names if has_car(_file_lines(path(x)), path(x))], 0
    if parse_device != "cuda":
        raise ValueError("car_split: --parse_device %r is neither 'cpu' nor 'cuda'" % (parse_device,))
    from . import kitti_annos
    texts = _read_texts(label_dir, names)
    side = kitti_annos.parse_texts(texts, "cuda", host_anno=lambda text, skip_blank: kitti_annos._anno_from_rows([]))
    keep = car_mask_columns(side)
    for f in sorted(side._host_annos):                           # outside the device grammar: the definition, for that file alone
        keep[f] = has_car(_text_lines(texts[f]), path(names[f]))
    return names, [x for x, k in zip(names, keep) if k], side.parse_stats["host_files"]


def car_split(roots, layout="dataset", parse_device="cpu", log=print):
    """The reference's run over ``roots`` in order -> {output path: text}.  Every list is made before the first file is written."""
    plan = []
    for root in roots:
        for split in SPLITS:
            names, kept, host = kept_names(root, split, layout, parse_device)
            plan.append((root, split, len(names), kept, host))
    np.random.seed(SEED)
    written = {}
    for root, split, listed, kept, host in plan:
        np.random.shuffle(kept)
        out = os.path.join(layout_dirs(root, layout)[0], split + "_car1.txt")
        with open(out, "w") as f:
            f.write("\n".join(kept))
        written[out] = "\n".join(kept)
        log("%s %s: %d listed, %d kept, %d host-decided files" % (root, split, listed, len(kept), host))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m 3d_adapt_auto_driving_amd.car_split", description=__doc__.split("\n")[0])
    ap.add_argument("roots", nargs="+", metavar="ROOT")
    ap.add_argument("--layout", type=str, default="dataset", choices=LAYOUTS)
    ap.add_argument("--parse_device", type=str, default="cpu", choices=("cpu", "cuda"))
    a = ap.parse_args(argv)
    car_split(a.roots, a.layout, a.parse_device)


if __name__ == "__main__":
    main()
