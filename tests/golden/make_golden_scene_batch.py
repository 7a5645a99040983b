"""Generates tests/golden/g21_scene_batch_ref.npz: what the two valid-point filters of the package returned BEFORE they became one
function (scene_batch.valid_points), on the fake trees of tests/aug_tree.py (g19) and tests/train_tree.py (g20).

RUN AT THE COMMIT BEFORE scene_batch.py EXISTED (28d6e02), from that checkout, with this file and the two tree modules on the path:
    python tests/golden/make_golden_scene_batch.py [package checkout]
  a_<class>_<id>       aug_scene.valid_points(pts, calib, shape, area_scope(class)) for class Car / People and every scene of the g19
                       tree: is_rect False, reduce True
  t_<reduce>_<id>      RpnTrainInput.valid_points(load_scene(id)) with PC_REDUCE_BY_RANGE <reduce> (1 / 0) for every scene of the g20
                       tree, the pre-made aug scene 400007 (is_rect True) included
Each case is recorded as ``record()`` makes it: the number of valid points, the SHA-256 of the rect rows' and of the intensities' bytes,
and every 97th row in full (for a readable failure).
"""
import hashlib
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "3d_adapt_auto_driving_amd"
OUT = os.path.join(HERE, "g21_scene_batch_ref.npz")
STEP = 97


def record(rect, inten):
    """(pts_rect (m, 3) f32, intensity (m,) f32) -> the arrays recorded for the case"""
    assert rect.dtype == np.float32 and inten.dtype == np.float32 and rect.shape == (len(inten), 3)
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)
    return {"n": np.int64(len(inten)), "sha_rect": sha(rect), "sha_intensity": sha(inten),
            "rows": np.concatenate((rect[::STEP], inten[::STEP].reshape(-1, 1)), 1)}


def g19_scene(root, sample_id):
    """-> (pts, calib, image shape) of a scene of the g19 tree"""
    import aug_tree
    kitti_io = importlib.import_module(PKG + ".kitti_io")
    base = os.path.join(root, "KITTI", "object", "training")
    pts = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
    return pts, kitti_io.Calibration(os.path.join(base, "calib", "%06d.txt" % sample_id)), aug_tree.IMG_SHAPE


def g20_source(root, reduce):
    """-> an RpnTrainInput over the g20 tree (no GT-aug: only its scene loader is used)"""
    import train_tree
    cfg = importlib.import_module(PKG + ".config").make_cfg()
    cfg["GT_AUG_ENABLED"], cfg["PC_REDUCE_BY_RANGE"] = False, bool(reduce)
    return importlib.import_module(PKG + ".train_input").RpnTrainInput(root, cfg, None, split=train_tree.SPLIT, device="cpu")


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    sys.path.insert(0, os.path.dirname(HERE))
    import aug_tree
    import train_tree
    A = importlib.import_module(PKG + ".aug_scene")
    assert not os.path.exists(os.path.join(os.path.dirname(A.__file__), "scene_batch.py")), "run this at the commit before the fold"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        g19, g20 = os.path.join(tmp, "g19"), os.path.join(tmp, "g20")
        aug_tree.write_aug_tree(g19)
        train_tree.write_train_tree(g20)
        for class_name in ("Car", "People"):
            for sid in aug_tree.SAMPLE_IDS:
                pts, calib, shape = g19_scene(g19, sid)
                for k, v in record(*A.valid_points(pts, calib, shape, A.area_scope(class_name))).items():
                    out["a_%s_%d_%s" % (class_name, sid, k)] = v
        for reduce in (1, 0):
            src = g20_source(g20, reduce)
            for sid in train_tree.SAMPLE_IDS:
                for k, v in record(*src.valid_points(src.load_scene(sid))).items():
                    out["t_%d_%d_%s" % (reduce, sid, k)] = v
    out["numpy"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases" % (OUT, sum(k.endswith("_n") for k in out)))


if __name__ == "__main__":
    main()
