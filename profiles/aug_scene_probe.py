"""Times augmented-scene generation (3d_adapt_auto_driving_amd/aug_scene.py), batch 8 scenes x 4 epochs, a 2000-entry synthetic database:
  place     place_candidates on the device, uploads and downloads inside the timed call (median of REPS after a warm-up; the database
            is resident, as in the tool)
  cpu       the same module's cpu path on the same scenes and candidate lists (one run)
  tool      generate_aug_scene on a synthetic 16-scene tree with file I/O, device and cpu (40k-point scenes: a tree small enough to
            write; its database is made by generate_gt_database first)

Every measurement is a child process of its own under ``timeout``; its exit status is checked and a failure ends the run.
    python profiles/aug_scene_probe.py            # all steps, one JSON line each
    python profiles/aug_scene_probe.py STEP ARGS  # one step (what the parent starts)
"""
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((120000, 30), (180000, 60))
BATCH, EPOCHS, REPS, DB_ENTRIES = 8, 4, 7, 2000
SHAPE = (375, 1242)
CALIB = {"P2": np.array([[707.0, 0, 604.0, 45.0], [0, 707.0, 180.0, 0.2], [0, 0, 1.0, 0.003]]), "R0": np.eye(3),
         "Tr_velo2cam": np.array([[0.0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]])}
PLANE = np.array([0.002, -1.0, 0.004, 1.65])


def scenes(n, g, batch=BATCH):
    synth = importlib.import_module("3d_adapt_auto_driving_amd.synth")
    out = []
    for s in range(batch):
        rng = np.random.default_rng(1900 + s)
        rect = synth.dense_scene(1900 + s, n)[:, :3].astype(np.float64)
        boxes = np.zeros((g, 7), dtype=np.float32)
        at = rect[rng.integers(0, len(rect), g)]
        boxes[:, 0], boxes[:, 2], boxes[:, 1] = at[:, 0], at[:, 2], 1.7
        boxes[:, 3:6] = rng.uniform((1.3, 1.4, 3.2), (1.8, 1.9, 4.6), (g, 3))
        boxes[:, 6] = rng.uniform(-np.pi, np.pi, g)
        velo = (rect - CALIB["Tr_velo2cam"][:, 3]) @ CALIB["Tr_velo2cam"][:, :3]
        out.append((np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32), CALIB, SHAPE, boxes, PLANE / np.linalg.norm(PLANE[:3])))
    return out


def database(entries=DB_ENTRIES):
    rng = np.random.default_rng(1899)
    db = []
    for _ in range(entries):
        n = int(rng.integers(0, 600))
        hwl = rng.uniform((1.3, 1.4, 3.2), (1.8, 1.9, 4.6))
        box = np.array([rng.uniform(-42, 42), 1.7, rng.uniform(2, 74), hwl[0], hwl[1], hwl[2], rng.uniform(-np.pi, np.pi)], dtype=np.float32)
        loc = rng.uniform(-0.5, 0.5, (n, 3)) * [hwl[2], hwl[0], hwl[1]]
        c, s = np.cos(box[6]), np.sin(box[6])
        pts = np.stack([box[0] + loc[:, 0] * c + loc[:, 2] * s, box[1] - hwl[0] / 2 + loc[:, 1], box[2] - loc[:, 0] * s + loc[:, 2] * c], 1)
        db.append({"gt_box3d": box, "points": pts.astype(np.float32), "intensity": rng.random(n).astype(np.float32)})
    return db


def step_place(device, n, g):
    A = importlib.import_module("3d_adapt_auto_driving_amd.aug_scene")
    sc, db = scenes(n, g), database()
    rng = A.new_rng()
    jobs = [(s, A.replay_candidates(rng, db, A.area_scope("Car"))) for _ in range(EPOCHS) for s in range(BATCH)]
    placer = A.AugPlacer(db, device) if device != "cpu" else None          # the resident database: uploaded once per run of the tool
    run = lambda j: A.place_candidates(sc, j, db, device=device, placer=placer)
    times, reps = [], (REPS if device != "cpu" else 1)
    run(jobs if device != "cpu" else jobs[:1])                               # warm-up: imports, library load, allocator
    for _ in range(reps):
        t0 = time.perf_counter()
        res = run(jobs)                                                      # ends with the download: synchronous
        times.append(time.perf_counter() - t0)
    print(json.dumps({"step": "place", "device": device, "points": n, "boxes": g, "batch": BATCH, "epochs": EPOCHS, "db": len(db),
                      "candidates": sum(len(c) for _, c in jobs), "accepted": sum(len(a) for _, a in res),
                      "rows": sum(len(r) for r, _ in res), "ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * min(times),
                      "ms_max": 1e3 * max(times), "reps": reps}))


def png_header(path, width, height):
    """the signature and the IHDR chunk: what the tool reads of an image"""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + struct.pack(">I", 13) + b"IHDR" + ihdr + struct.pack(">I", zlib.crc32(b"IHDR" + ihdr)))


def step_tool(device, n, g, n_scenes=16):
    A = importlib.import_module("3d_adapt_auto_driving_amd.aug_scene")
    G = importlib.import_module("3d_adapt_auto_driving_amd.gt_database")
    with tempfile.TemporaryDirectory() as root:
        base = os.path.join(root, "KITTI", "object", "training")
        for sub in ("velodyne", "calib", "label_2", "planes", "image_2"):
            os.makedirs(os.path.join(base, sub))
        os.makedirs(os.path.join(root, "KITTI", "ImageSets"))
        row = lambda a: " ".join("%.12e" % v for v in np.asarray(a).reshape(-1))
        for s, (velo, cal, shape, boxes, plane) in enumerate(scenes(n, g, n_scenes)):
            velo.tofile(os.path.join(base, "velodyne", "%06d.bin" % s))
            with open(os.path.join(base, "calib", "%06d.txt" % s), "w") as f:
                f.write("P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\n" % (
                    row(cal["P2"]), row(cal["P2"]), row(cal["P2"]), row(cal["P2"]), row(cal["R0"]), row(cal["Tr_velo2cam"])))
            with open(os.path.join(base, "label_2", "%06d.txt" % s), "w") as f:
                for x, y, z, h, w, l, ry in boxes:
                    f.write("Car 0.00 0 0.00 100.00 100.00 200.00 160.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n" % (h, w, l, x, y, z, ry))
            with open(os.path.join(base, "planes", "%06d.txt" % s), "w") as f:
                f.write("# Plane\nWidth 4\nHeight 1\n%s\n" % row(plane))
            png_header(os.path.join(base, "image_2", "%06d.png" % s), shape[1], shape[0])
        with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
            f.write("".join("%06d\n" % s for s in range(n_scenes)))
        db = G.generate_gt_database(root, save_dir=os.path.join(root, "db"), device="cuda" if device != "cpu" else "cpu", batch_size=BATCH,
                                    log=lambda s: None)
        times = []
        for k in range(2 if device != "cpu" else 1):                        # the first run carries the imports and the library load
            t0 = time.perf_counter()
            ids = A.generate_aug_scene(root, db, os.path.join(root, "aug%d" % k), aug_times=EPOCHS, device=device, batch_size=BATCH,
                                       log=lambda s: None)
            times.append(time.perf_counter() - t0)
    print(json.dumps({"step": "tool", "device": device, "points": n, "boxes": g, "scenes": n_scenes, "epochs": EPOCHS, "db": len(db),
                      "written": len(ids) - n_scenes, "s_first": times[0], "s_last": times[-1]}))


def main():
    if len(sys.argv) > 1:
        step, device, n, g = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        {"place": step_place, "tool": step_tool}[step](device, n, g)
        return
    jobs = [("place", d, n, g, 420) for n, g in SIZES for d in ("cuda", "cpu")]
    jobs += [("tool", d, 40000, 30, 420) for d in ("cuda", "cpu")]
    for step, device, n, g, limit in jobs:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step, device, str(n), str(g)])
        if rc != 0:
            sys.exit("step %s %s %d %d ended with status %d: nothing more is started" % (step, device, n, g, rc))


if __name__ == "__main__":
    main()
