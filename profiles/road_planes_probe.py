"""Times road-plane estimation (3d_adapt_auto_driving_amd/road_planes.py) at two sweep sizes, batch 8, iters 512:
  estimate  estimate_planes on the device, upload and the one download inside the timed call (median of REPS after a warm-up)
  cpu       the same module's cpu path on the same scenes (one run)
  tool      generate_planes on a synthetic tree with file I/O, device and cpu (16 scenes of 40k points: a tree small enough to write)

The sweeps: a tilted ground with 2 cm noise over x in +-40, z in -10..70 (about half of the points are candidates of the default
range), a third of the rows lifted above it.  Every measurement is a child process of its own under ``timeout``; its exit status is
checked and a failure ends the run.
    python profiles/road_planes_probe.py            # all steps, one JSON line each
    python profiles/road_planes_probe.py STEP ARGS  # one step (what the parent starts)
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
SIZES = (120000, 180000)
BATCH, REPS = 8, 7
TR = np.array([[0.0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]])
CALIB = {"P2": np.eye(3, 4), "R0": np.eye(3), "Tr_velo2cam": TR}


def scenes(n, batch=BATCH):
    out = []
    for s in range(batch):
        rng = np.random.default_rng(2400 + s)
        x, z = rng.uniform(-40, 40, n), rng.uniform(-10, 70, n)
        y = 1.7 + 0.03 * x - 0.02 * z + rng.normal(0, 0.02, n)
        y[: n // 3] -= rng.uniform(0.3, 3.0, n // 3)
        rect = np.stack([x, y, z], 1)[rng.permutation(n)]
        velo = (rect - TR[:, 3]) @ TR[:, :3]
        out.append((np.concatenate([velo, rng.random((n, 1))], 1).astype(np.float32), CALIB))
    return out


def step_estimate(device, n):
    R = importlib.import_module("3d_adapt_auto_driving_amd.road_planes")
    sc = scenes(n)
    times, reps = [], (REPS if device != "cpu" else 1)
    R.estimate_planes(sc if device != "cpu" else sc[:1], device, iters=8 if device == "cpu" else 512)   # warm-up: imports, library load
    for _ in range(reps):
        t0 = time.perf_counter()
        planes, infos = R.estimate_planes(sc, device)                       # ends with the download: synchronous
        times.append(time.perf_counter() - t0)
    print(json.dumps({"step": "estimate", "device": device, "points": n, "batch": BATCH, "iters": 512,
                      "candidates": int(np.mean([i["candidates"] for i in infos])), "fallbacks": sum(i["fallback"] is not None for i in infos),
                      "ms_median": 1e3 * float(np.median(times)), "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times), "reps": reps}))


def step_tool(device, n, n_scenes=16):
    R = importlib.import_module("3d_adapt_auto_driving_amd.road_planes")
    with tempfile.TemporaryDirectory() as root:
        base = os.path.join(root, "KITTI", "object", "training")
        for sub in ("velodyne", "calib"):
            os.makedirs(os.path.join(base, sub))
        os.makedirs(os.path.join(root, "KITTI", "ImageSets"))
        eye34 = " ".join("%.12e" % v for v in np.eye(3, 4).reshape(-1))
        for s, (velo, _) in enumerate(scenes(n, n_scenes)):
            velo.tofile(os.path.join(base, "velodyne", "%06d.bin" % s))
            with open(os.path.join(base, "calib", "%06d.txt" % s), "w") as f:
                f.write("P0: %s\nP1: %s\nP2: %s\nP3: %s\nR0_rect: %s\nTr_velo_to_cam: %s\n" % (
                    eye34, eye34, eye34, eye34, " ".join("%.12e" % v for v in np.eye(3).reshape(-1)), " ".join("%.12e" % v for v in TR.reshape(-1))))
        with open(os.path.join(root, "KITTI", "ImageSets", "train.txt"), "w") as f:
            f.write("".join("%06d\n" % s for s in range(n_scenes)))
        times = []
        for _ in range(2):                                                  # the first run carries the imports and the library load
            t0 = time.perf_counter()
            got = R.generate_planes(root, device=device, batch=BATCH, overwrite=True, log=lambda s: None)
            times.append(time.perf_counter() - t0)
    print(json.dumps({"step": "tool", "device": device, "points": n, "scenes": n_scenes, "fallbacks": sum(g[2]["fallback"] is not None for g in got),
                      "s_first": times[0], "s_last": times[-1]}))


def main():
    if len(sys.argv) > 1:
        {"estimate": step_estimate, "tool": step_tool}[sys.argv[1]](sys.argv[2], int(sys.argv[3]))
        return
    jobs = [("estimate", d, n, 300) for n in SIZES for d in ("cuda", "cpu")] + [("tool", d, 40000, 300) for d in ("cuda", "cpu")]
    for step, device, n, limit in jobs:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step, device, str(n)])
        if rc != 0:
            sys.exit("step %s %s %d ended with status %d: nothing more is started" % (step, device, n, rc))


if __name__ == "__main__":
    main()
