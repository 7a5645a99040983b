"""Throughput of statistical normalization: rescale_scenes on the device (csrc/stat_norm.hip) against the numpy path, for
120 k-point scenes with 30 cars and 180 k-point scenes with 60 cars, avoid_conflict off and on; then whole-tree convert_tree
(reads, device work, writes) on a synthetic tree.  One JSON line per measurement (also collected into --json PATH).

    python profiles/stat_norm_probe.py [--batch 8] [--reps 5] [--tree 48] [--json PATH]
"""
import argparse
import importlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SN = importlib.import_module("3d_adapt_auto_driving_amd.stat_norm")
MAPPING = {"src": {"height": {"mean": 1.52}, "width": {"mean": 1.63}, "length": {"mean": 3.88}},
           "dst": {"height": {"mean": 1.77}, "width": {"mean": 1.93}, "length": {"mean": 4.91}}}
CALIB = {"P2": np.array([707.0493, 0, 604.0814, 45.75831, 0, 707.0493, 180.5066, -0.3454157, 0, 0, 1, 0.004981016]),
         "R0_rect": np.array([0.9999239, 0.00983776, -0.007445048, -0.009869795, 0.9999421, -0.004278459, 0.007402527, 0.004351614,
                              0.9999631]),
         "Tr_velo_to_cam": np.array([0.007533745, -0.9999714, -0.000616602, -0.004069766, 0.01480249, 0.0007280733, -0.9998902,
                                     -0.07631618, 0.9998621, 0.00752379, 0.01480755, -0.2717806])}


def scene(rng, calib, n, n_cars):
    """A LiDAR-like cloud (rect frame: ground, cars standing on it, clutter) and its Car / Pedestrian labels."""
    xyz = np.stack([rng.uniform(-30, 30, n), rng.uniform(1.4, 1.7, n), rng.uniform(3, 70, n)], 1)      # ground
    lines = []
    for k in range(n_cars):
        x, z, ry = rng.uniform(-20, 20), rng.uniform(5, 60), rng.uniform(-np.pi, np.pi)
        h, w, l = rng.normal(1.52, 0.08), rng.normal(1.63, 0.06), rng.normal(3.9, 0.3)
        m = int(n * 0.4 / n_cars)
        loc = np.stack([rng.uniform(-l / 2, l / 2, m), rng.uniform(-h, 0, m), rng.uniform(-w / 2, w / 2, m)], 1)
        c, s = np.cos(ry), np.sin(ry)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        xyz[rng.integers(0, n, m)] = loc @ R.T + [x, 1.65, z]
        lines.append("%s 0.00 0 %.2f 100 100 200 200 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            "Car" if k % 8 else "Pedestrian", rng.uniform(-3, 3), h, w, l, x, 1.65, z, ry))
    velo = calib.rect_to_velo(xyz).astype(np.float32)
    return np.concatenate([velo, rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1), lines


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", type=int, default=48)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    calib = SN.Calib(CALIB)
    mapping = SN.scale_map(MAPPING["src"], MAPPING["dst"])
    out = []
    for n, cars in ((120_000, 30), (180_000, 60)):
        sc = [scene(rng, calib, n, cars) for _ in range(a.batch)]
        args = ([s[0] for s in sc], [s[1] for s in sc], [calib] * a.batch, mapping)
        for ac in (False, True):
            gpu = timed(lambda: SN.rescale_scenes(*args, avoid_conflict=ac, device="cuda"), a.reps)
            t0 = time.perf_counter()
            SN.rescale_scenes([sc[0][0]], [sc[0][1]], [calib], mapping, avoid_conflict=ac, device="cpu")     # one scene
            cpu = time.perf_counter() - t0
            rec = {"probe": "rescale_scenes", "points": n, "cars": cars, "avoid_conflict": ac, "batch": a.batch,
                   "gpu_ms_per_scene": 1e3 * gpu / a.batch, "gpu_scenes_per_s": a.batch / gpu,
                   "numpy_ms_per_scene": 1e3 * cpu, "numpy_scenes_per_s": 1.0 / cpu}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    # whole tree: 120 k x 30 scenes
    tmp = tempfile.mkdtemp(prefix="sn_probe_")
    try:
        src = os.path.join(tmp, "src")
        tr = os.path.join(src, "training")
        for d in ("velodyne", "label_2", "calib", "image_2"):
            os.makedirs(os.path.join(tr, d))
        calib_text = "\n".join("%s: %s" % (k, " ".join("%.12e" % x for x in v)) for k, v in CALIB.items()) + \
            "\nP3: " + " ".join("%.12e" % x for x in CALIB["P2"]) + "\n"
        ids = ["%06d" % i for i in range(a.tree)]
        base = [scene(rng, calib, 120_000, 30) for _ in range(8)]
        for k, i in enumerate(ids):
            v, lines = base[k % 8]
            v.tofile(os.path.join(tr, "velodyne", i + ".bin"))
            with open(os.path.join(tr, "label_2", i + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
            with open(os.path.join(tr, "calib", i + ".txt"), "w") as f:
                f.write(calib_text)
        for split in ("train", "val", "trainval"):
            with open(os.path.join(src, split + ".txt"), "w") as f:
                f.write("\n".join(ids) + "\n")
        for dev in ("cuda", "cpu"):
            for ac in (False, True):
                if dev == "cpu" and a.tree > 8:
                    with open(os.path.join(src, "trainval.txt"), "w") as f:
                        f.write("\n".join(ids[:8]) + "\n")
                t0 = time.perf_counter()
                n = SN.convert_tree(src, os.path.join(tmp, "dst_%s_%d" % (dev, ac)), MAPPING["src"], MAPPING["dst"], avoid_conflict=ac,
                                    image_size=(1242, 375), batch=a.batch, device=dev)
                dt = time.perf_counter() - t0
                rec = {"probe": "convert_tree", "device": dev, "avoid_conflict": ac, "scenes": n, "points": 120_000, "cars": 30,
                       "s": dt, "scenes_per_s": n / dt}
                print(json.dumps(rec), flush=True)
                out.append(rec)
            with open(os.path.join(src, "trainval.txt"), "w") as f:
                f.write("\n".join(ids) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
