"""Times GT-database extraction (3d_adapt_auto_driving_amd/gt_database.py) at two scene sizes, batch 8:
  extract   extract_objects on the device, uploads and downloads inside the timed call (median of REPS after a warm-up)
  cpu       the same module's cpu path on the same scenes (one run)
  tool      generate_gt_database on a synthetic tree with file I/O, device and cpu (40k-point scenes: a tree small enough to write)

Every measurement is a child process of its own under ``timeout``; its exit status is checked and a failure ends the run.
    python profiles/gt_database_probe.py            # all steps, one JSON line each
    python profiles/gt_database_probe.py STEP ARGS  # one step (what the parent starts)
"""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((120000, 30), (180000, 60))
BATCH, REPS = 8, 7
CALIB = {"P2": np.eye(3, 4), "R0": np.eye(3), "Tr_velo2cam": np.array([[0.0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]])}


def scenes(n, g, batch=BATCH):
    synth = importlib.import_module("3d_adapt_auto_driving_amd.synth")
    out = []
    for s in range(batch):
        rng = np.random.default_rng(1700 + s)
        rect = synth.dense_scene(1700 + s, n)[:, :3].astype(np.float64)
        boxes = np.zeros((g, 7), dtype=np.float32)
        at = rect[rng.integers(0, len(rect), g)]
        boxes[:, 0], boxes[:, 2], boxes[:, 1] = at[:, 0], at[:, 2], at[:, 1] + 0.8
        boxes[:, 3:6] = rng.uniform((1.3, 1.4, 3.2), (1.8, 1.9, 4.6), (g, 3))
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, g)
        velo = (rect - CALIB["Tr_velo2cam"][:, 3]) @ CALIB["Tr_velo2cam"][:, :3]
        out.append((np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32), CALIB, boxes))
    return out


def step_extract(device, n, g):
    G = importlib.import_module("3d_adapt_auto_driving_amd.gt_database")
    sc = scenes(n, g)
    times, reps = [], (REPS if device != "cpu" else 1)
    G.extract_objects(sc if device != "cpu" else sc[:1], device)        # warm-up: imports, library load, allocator
    for _ in range(reps):
        t0 = time.perf_counter()
        res = G.extract_objects(sc, device)                             # ends with the download: synchronous
        times.append(time.perf_counter() - t0)
    pts = sum(len(p) for a in res for p, _ in a)
    print(json.dumps({"step": "extract", "device": device, "points": n, "boxes": g, "batch": BATCH, "object_points": pts,
                      "ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times), "reps": reps}))


def step_tool(device, n, g, n_scenes=16):
    G = importlib.import_module("3d_adapt_auto_driving_amd.gt_database")
    with tempfile.TemporaryDirectory() as root:
        base = os.path.join(root, "KITTI", "object", "training")
        for sub in ("velodyne", "calib", "label_2"):
            os.makedirs(os.path.join(base, sub))
        os.makedirs(os.path.join(root, "KITTI", "ImageSets"))
        eye34 = " ".join("%.12e" % v for v in np.eye(3, 4).reshape(-1))
        for s, (velo, cal, boxes) in enumerate(scenes(n, g, n_scenes)):
            velo.tofile(os.path.join(base, "velodyne", "%06d.bin" % s))
            with open(os.path.join(base, "calib", "%06d.txt" % s), "w") as f:
                f.write("P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\n" % (
                    eye34, eye34, eye34, eye34, " ".join("%.12e" % v for v in np.eye(3).reshape(-1)),
                    " ".join("%.12e" % v for v in cal["Tr_velo2cam"].reshape(-1))))
            with open(os.path.join(base, "label_2", "%06d.txt" % s), "w") as f:
                for x, y, z, h, w, l, ry in boxes:
                    f.write("Car 0.00 0 0.00 100.00 100.00 200.00 160.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (h, w, l, x, y, z, ry))
        with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
            f.write("".join("%06d\n" % s for s in range(n_scenes)))
        times = []
        for _ in range(2):                                              # the first run carries the imports and the library load
            t0 = time.perf_counter()
            db = G.generate_gt_database(root, save_dir=os.path.join(root, "db"), device=device, batch_size=BATCH, log=lambda s: None)
            times.append(time.perf_counter() - t0)
    print(json.dumps({"step": "tool", "device": device, "points": n, "boxes": g, "scenes": n_scenes, "entries": len(db),
                      "s_first": times[0], "s_last": times[-1]}))


def main():
    if len(sys.argv) > 1:
        step, device, n, g = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        {"extract": step_extract, "tool": step_tool}[step](device, n, g)
        return
    jobs = [("extract", d, n, g, 300) for n, g in SIZES for d in ("cuda", "cpu")]
    jobs += [("tool", d, 40000, 30, 300) for d in ("cuda", "cpu")]
    for step, device, n, g, limit in jobs:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step, device, str(n), str(g)])
        if rc != 0:
            sys.exit("step %s %s %d %d ended with status %d: nothing more is started" % (step, device, n, g, rc))


if __name__ == "__main__":
    main()
