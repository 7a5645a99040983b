"""Nested sampling levels of the RPN backbone, standalone: 32 clouds (a geometry group) at 4096 -> 1024, 1024 -> 256, 256 -> 64.

Per level and scene kind (uniform | lidar), launches back to back on one stream, device events around 20 calls, median of 5:
  plain     prcnn_fps_new_xyz                                   (what the levels ran before)
  nested    prcnn_fps_new_xyz_nested on the level's real input  (check + skipped sampling launches)
  check     prcnn_fps_prefix_check alone
  miss      prcnn_fps_new_xyz_nested on lattice clouds          (check + full sampling: the price of a rejected cloud) against
  miss0     prcnn_fps_new_xyz on the same lattice clouds
and the share of clouds the check accepts at each level.  Level 1 (16384 -> 4096, no flag) is timed too: it must not move against the
parent commit -- `--lib PATH` runs the plain entries only, against another build of libprcnn_hip.so.
`--accept G`: no timing; G geometry groups of 32 clouds per scene kind, drawn with the seeds bench.py draws its batches with, through
the four sampling levels: clouds accepted per nested level, and the groups in which EVERY cloud of a level is accepted."""
import argparse, importlib, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser(); ap.add_argument("--lib"); ap.add_argument("--clouds", type=int, default=32); ap.add_argument("--accept", type=int, default=0)
args = ap.parse_args()
L = importlib.import_module("3d_adapt_auto_driving_amd._lib")
NEW = ("prcnn_fps_new_xyz_nested", "prcnn_fps_nested_supported", "prcnn_fps_prefix_check")
if args.lib:
    L.LIB_PATH = os.path.abspath(args.lib)
    for k in NEW:
        L.SIGNATURES.pop(k, None)
pkg = importlib.import_module("3d_adapt_auto_driving_amd"); sys.path.insert(0, pkg.DROPIN_DIR)
import pointnet2_cuda as P
synth = importlib.import_module("3d_adapt_auto_driving_amd.synth")
dev = torch.device("cuda", 0)
B = args.clouds


def timed(fn, calls=20, reps=5):
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return statistics.median(out), min(out), max(out)


def row(tag, t):
    print("  %-7s %8.1f us   (min %.1f, max %.1f)" % (tag, t[0], t[1], t[2]), flush=True)


if args.accept:
    for kind, seed0 in (("uniform", 0), ("lidar", 70000)):            # bench.py: seed0 = slot * BATCH / 70000 + slot * BATCH
        make = synth.lidar_scenes if kind == "lidar" else synth.scenes
        acc, whole = {}, {}
        for grp in range(args.accept):
            cur = P.fps_new_xyz_wrapper(torch.from_numpy(make(B, 16384, seed0=seed0 + grp * B)).to(dev), 4096)[1]
            for m in (1024, 256, 64):
                rej = int(P.fps_prefix_check_wrapper(cur, m).sum())
                acc[m] = acc.get(m, 0) + B - rej
                whole[m] = whole.get(m, 0) + (rej == 0)
                cur = P.fps_new_xyz_wrapper(cur, m)[1]
        for m in (1024, 256, 64):
            print("%-7s %4d -> %4d: %d of %d clouds accepted (%.1f %%), %d of %d groups whole" % (
                kind, 4 * m, m, acc[m], args.accept * B, 100.0 * acc[m] / (args.accept * B), whole[m], args.accept), flush=True)
    sys.exit(0)
g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
print("library: %s, %d clouds" % (L.LIB_PATH, B))
for kind in ("uniform", "lidar"):
    xyz = torch.from_numpy((synth.lidar_scenes if kind == "lidar" else synth.scenes)(B, 16384, seed0=0)).to(dev)
    print("== %s scenes" % kind)
    print("16384 -> 4096 (level 1, plain entry, no flag)")
    row("plain", timed(lambda: P.fps_new_xyz_wrapper(xyz, 4096), calls=5))
    cur = P.fps_new_xyz_wrapper(xyz, 4096)[1]
    for n, m in ((4096, 1024), (1024, 256), (256, 64)):
        print("%d -> %d" % (n, m))
        row("plain", timed(lambda: P.fps_new_xyz_wrapper(cur, m)))
        if not args.lib:
            row("nested", timed(lambda: P.fps_new_xyz_nested_wrapper(cur, m)))
            row("check", timed(lambda: P.fps_prefix_check_wrapper(cur, m)))
            lat = torch.from_numpy(np.stack([np.resize(g[np.random.default_rng(c).permutation(len(g))], (n, 3)) for c in range(B)]).astype(np.float32)).to(dev)
            row("miss", timed(lambda: P.fps_new_xyz_nested_wrapper(lat, m)))
            row("miss0", timed(lambda: P.fps_new_xyz_wrapper(lat, m)))
            rej = P.fps_prefix_check_wrapper(cur, m)
            print("  accepted %d of %d clouds" % (B - int(rej.sum()), B), flush=True)
        cur = P.fps_new_xyz_wrapper(cur, m)[1]
