"""Times random object scaling (object_scale.py, csrc/object_scale.hip) and writes profiles/object_scale_probe.md.
  python profiles/object_scale_probe.py [--out FILE]

1. The operator alone, object_scale.scale_objects(device="cuda") with ``extra`` of 4 channels, between device events (the small uploads
   of boxes, counts, trig and factors are inside): 3 warm-up rounds, median (min - max) of 9, at B = 16, N = 16384, G = 30 and G = 60
   and at B = 8, N = 16384, G = 30.  The points are restored from a resident copy before every round (outside the events).
2. RpnTrainInput.batch() at the shape of profiles/train_input_probe.py (8 scenes x 16384 points from 120 k-point clouds with 30 labels),
   with obj_scale off and on: two sources with the same seed, alternating call by call in one process, wall time with a synchronize
   behind every call, 3 warm-up rounds, median (min - max) of 9.
The numpy path is a definition, not a competitor: it is not timed."""
import argparse
import importlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
PKG = "3d_adapt_auto_driving_amd"
WARM, ROUNDS = 3, 9


def fmt(ms):
    return "%.3f (%.3f - %.3f)" % (np.median(ms), min(ms), max(ms))


def operator_rows():
    import torch
    import object_scale_scenes as scenes
    OS = importlib.import_module(PKG + ".object_scale")
    rows = []
    for B, N, G in ((16, 16384, 30), (16, 16384, 60), (8, 16384, 30)):
        pts, gts, factors = scenes.isolated_scenes(7, B, N, G, 0.8, 1.2)
        gt = np.stack(gts)
        counts = np.full(B, G, dtype=np.int32)
        keep = torch.from_numpy(np.concatenate((pts, np.zeros((B, N, 1), np.float32)), axis=2)).cuda()
        t_pts, t_in = keep[:, :, :3].contiguous(), keep.clone()
        ms, hits = [], None
        for k in range(WARM + ROUNDS):
            t_pts.copy_(keep[:, :, :3])
            t_in.copy_(keep)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, _, hits = OS.scale_objects(t_pts, gt, counts, factors, device="cuda", extra=t_in)
            e1.record()
            torch.cuda.synchronize()
            if k >= WARM:
                ms.append(e0.elapsed_time(e1))
        owned = int(hits.cpu().numpy().astype(np.int64).sum())
        rows.append("| %d | %d | %d | %d of %d | %s |" % (B, N, G, owned, B * N, fmt(ms)))
    return rows


def batch_rows():
    import torch
    import train_input_probe
    T = importlib.import_module(PKG + ".train_input")
    G = importlib.import_module(PKG + ".gt_database")
    cfg = importlib.import_module(PKG + ".config").make_cfg()
    cfg["GT_AUG_ENABLED"], cfg["GT_AUG_RAND_NUM"], cfg["GT_AUG_APPLY_PROB"] = True, True, 1.0
    with tempfile.TemporaryDirectory() as root:
        train_input_probe.write_tree(root)
        G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cuda", log=lambda *a: None)
        db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
        srcs = {"off": T.RpnTrainInput(root, cfg, db, npoints=16384, seed=1, device="cuda"),
                "on": T.RpnTrainInput(root, cfg, db, npoints=16384, seed=1, device="cuda", obj_scale=(0.8, 1.2))}
        ms = {"off": [], "on": []}
        for k in range(WARM + ROUNDS):
            for name in ("off", "on") if k % 2 == 0 else ("on", "off"):
                t0 = time.perf_counter()
                srcs[name].batch(range(8))
                torch.cuda.synchronize()
                if k >= WARM:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        boxes = len(srcs["on"].last_scaled)
        owned = sum(rec[3] for rec in srcs["on"].last_scaled)
    add = np.median(ms["on"]) - np.median(ms["off"])
    return ["| off | %s | |" % fmt(ms["off"]),
            "| on (0.8, 1.2), %d boxes, %d owned points in the last batch | %s | %+.3f ms, %+.1f %% of the medians |" %
            (boxes, owned, fmt(ms["on"]), add, 100.0 * add / np.median(ms["off"]))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "object_scale_probe.md"))
    a = ap.parse_args()
    import torch
    lines = ["# Random object scaling: the operator and what it adds to a training batch", "",
             "Written by `python profiles/object_scale_probe.py` on one %s device.  Milliseconds, median (min - max) of %d after %d warm-up rounds." %
             (getattr(torch.cuda.get_device_properties(0), "gcnArchName", "").split(":")[0] or torch.cuda.get_device_name(0), ROUNDS, WARM), "",
             "## The operator alone (`scale_objects(device=\"cuda\")`, `extra` of 4 channels; device events, small uploads inside)", "",
             "| B | N | G | owned points | ms |", "|---|---|---|---|---|"] + operator_rows()
    lines += ["", "## `RpnTrainInput.batch()`, 8 scenes x 16384 points from 120 k-point clouds with 30 labels (wall time, alternating)", "",
              "| obj_scale | ms per batch() | added by the option |", "|---|---|---|"] + batch_rows()
    lines += ["", "The option adds one launch over 8 x 16384 x (3 + 4) floats, four small uploads (boxes, counts, trig, factors) and one "
              "blocking read of the hit counts per batch."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
