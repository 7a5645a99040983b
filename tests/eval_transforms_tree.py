"""Shared by tests/test_eval_transforms.py and tests/test_gpu_eval_transforms.py: the fixture g17 (tests/golden/
make_golden_eval_transforms.py: the reference's evaluate/evaluate.py on CPU) written back as a tree, and the comparison of one
configuration's outcome with what the reference returned and wrote.  Not a test module."""
import json
import os
import pickle

import numpy as np

from conftest import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
G17 = os.path.join(HERE, "golden", "g17_eval_transforms_ref.npz")


def fixture():
    return np.load(G17)


def configs(z):
    return [(str(n), json.loads(str(k))) for n, k in zip(z["configs"], z["config_kwargs"])]


CONFIG_NAMES = ["new", "old", "old_waymo", "coco_new", "coco_old", "toground", "rescale2", "align_size", "align_front", "reverse_align",
                "size_ground_save", "output_iou"]


def write_tree(z, tmp):
    """-> dict(result, labels, split, dataset, src_stats, dst_stats, ids): the generator's layout under ``tmp``."""
    tmp = str(tmp)
    t = {"dataset": os.path.join(tmp, "src_kitti"), "labels": os.path.join(tmp, "src_kitti", "training", "label_2"),
         "planes": os.path.join(tmp, "src_kitti", "training", "planes"), "result": os.path.join(tmp, "out_waymo", "run", "data"),
         "split": os.path.join(tmp, "src_kitti", "val.txt"), "out": os.path.join(tmp, "out_waymo"),
         "src_stats": os.path.join(tmp, "stats_a", "label_stats_val.json"), "dst_stats": os.path.join(tmp, "stats_b", "label_stats_val.json"),
         "ids": list(range(len(z["gt_lines"])))}
    for d in (t["labels"], t["planes"], t["result"], os.path.dirname(t["src_stats"]), os.path.dirname(t["dst_stats"])):
        os.makedirs(d)
    for i in t["ids"]:
        for d, key in ((t["labels"], "gt_lines"), (t["planes"], "plane_lines"), (t["result"], "dt_lines")):
            with open(os.path.join(d, "%06d.txt" % i), "w") as f:
                f.write(str(z[key][i]))
    with open(t["split"], "w") as f:
        f.write("\n".join("%06d" % i for i in t["ids"]))
    for key in ("src_stats", "dst_stats"):
        with open(t[key], "w") as f:
            f.write(str(z[key]))
    return t


def annos(z):
    KE = pkg("kitti_eval")
    gt = [KE.annos_from_lines(str(s).split("\n")) for s in z["gt_lines"]]
    dt = [KE.annos_from_lines(str(s).split("\n")) for s in z["dt_lines"]]
    return gt, dt


def evaluate_kwargs(t, kw):
    kw = dict(kw)
    if kw.get("reverse_align"):
        kw.update(src_stats=t["src_stats"], dst_stats=t["dst_stats"])
    return kw


def ap_arrays(ret):
    return np.stack([np.stack([v["mAPbbox"], v["mAPbev"], v["mAP3d"]], 0) for v in ret["result"][0].values()], 0)


def written(t):
    names, texts = [], []
    for root, _, files in sorted(os.walk(t["out"])):
        for fn in sorted(files):
            rel = os.path.relpath(os.path.join(root, fn), t["out"])
            if not rel.startswith(os.path.join("run", "data") + os.sep):
                names.append(rel)
                texts.append(open(os.path.join(root, fn)).read() if not fn.endswith(".pkl") else "")
    return names, texts


def check_configuration(z, name, kw, tmp, device):
    """evaluate() on a fresh tree: result text character for character, AP arrays within 1e-9 (the bar of
    test_kitti_eval.check_against_fixture), every written file character for character under the reference's names."""
    KE = pkg("kitti_eval")
    t = write_tree(z, tmp)
    r = KE.evaluate(t["result"], t["labels"], t["ids"], device=device, **evaluate_kwargs(t, kw))
    if kw.get("output_iou"):
        assert r is None
    elif kw.get("coco"):
        assert r == str(z["text_" + name])
    else:
        assert r[0] == str(z["text_" + name])
        np.testing.assert_allclose(ap_arrays(r[1]), z["ap_" + name], rtol=0, atol=1e-9, equal_nan=True)
    names, texts = written(t)
    assert names == [str(n) for n in z["files_%s_names" % name]]
    for n, got, want in zip(names, texts, z["files_%s_texts" % name]):
        if n.endswith(".pkl"):
            with open(os.path.join(t["out"], n), "rb") as f:
                saved = pickle.load(f)
            assert list(saved) == [0] and list(saved[0]) == list(r[1]["result"][0])
            for key, v in saved[0].items():
                for kind in ("mAPbbox", "mAPbev", "mAP3d"):
                    assert np.array_equal(v[kind], r[1]["result"][0][key][kind])
        else:
            assert got == str(want), n
    return t, r
