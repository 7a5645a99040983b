"""The BEV renderer, device against the numpy checker (bev.render_scenes, csrc/bev_render.hip), in one process: writes
profiles/bev_render_probe.md.  Workload: 8 scenes x 120 k points x 30 boxes at 800 x 800 (the default view), labels outlined.  The paths
alternate, 3 warm-up rounds, then median (min to max) of 7; host time in ms.  The device call holds its uploads (clouds, box records,
layer bytes, segments) and its one download (the images and the stats); it ends when the download has arrived.  The checker is the
definition, not a tuned host renderer: the table says what one call costs on each path, it claims no speed-up.

  python profiles/bev_render_probe.py [--scenes 8] [--points 120000] [--boxes 30] [--rounds 7] [--warmup 3] [--out profiles/bev_render_probe.md]"""
import argparse, importlib, os, statistics, sys, time
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
B = importlib.import_module("3d_adapt_auto_driving_amd.bev")
SN = importlib.import_module("3d_adapt_auto_driving_amd.stat_norm")

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8); ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--boxes", type=int, default=30)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", type=str, default=os.path.join(HERE, "bev_render_probe.md"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
clock = time.perf_counter

calib = SN.Calib({"P2": np.zeros(12), "R0_rect": np.array([9.999239e-01, 9.837760e-03, -7.445048e-03, -9.869795e-03, 9.999421e-01, -4.278459e-03,
                                                           7.402527e-03, 4.351614e-03, 9.999631e-01]),
                  "Tr_velo_to_cam": np.array([7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03, 1.480249e-02, 7.280733e-04,
                                              -9.998902e-01, -7.631618e-02, 9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01])})
rng = np.random.default_rng(0)
view = B.View()
scenes = []
for s in range(a.scenes):
    xyz = np.stack([rng.uniform(-45, 45, a.points), rng.uniform(-2.5, 1.8, a.points), rng.uniform(-2, 85, a.points)], 1)
    velo = np.concatenate([calib.rect_to_velo(xyz), rng.uniform(0, 1, (a.points, 1))], 1).astype(np.float32)
    boxes = np.stack([np.concatenate([xyz[rng.integers(a.points)] + [0, 0.8, 0], [rng.normal(1.6, 0.1), rng.normal(1.7, 0.1), rng.normal(4.0, 0.4),
                                                                                 rng.uniform(-np.pi, np.pi)]]) for _ in range(a.boxes)])
    scenes.append(B.Scene([B.Cloud(velo, calib, boxes, 0, 1)], [(0, boxes)]))


def run(device):
    if device != "cpu":
        torch.cuda.synchronize(dev)
    t0 = clock()
    img, st = B.render_scenes(scenes, view, device=device)
    return clock() - t0, img, st


rows, answers = {"cpu": [], "cuda": []}, {}
for rnd in range(a.warmup + a.rounds):
    for name in ("cpu", "cuda") if rnd % 2 == 0 else ("cuda", "cpu"):
        t, img, st = run(name)
        answers[name] = (img, st)
        if rnd >= a.warmup:
            rows[name].append(1e3 * t)
    assert answers["cpu"][0].tobytes() == answers["cuda"][0].tobytes(), "the two paths disagree on a pixel"
    assert all(np.array_equal(answers["cpu"][1][k], answers["cuda"][1][k]) for k in answers["cpu"][1])
    print("round %d done" % rnd, file=sys.stderr, flush=True)
cell = lambda v: "%.1f (%.1f-%.1f)" % (statistics.median(v), min(v), max(v))
st = answers["cpu"][1]
out = ["# The BEV renderer, device against the numpy checker (profiles/bev_render_probe.py)", "",
       "%s, torch %s; ms of host time per render_scenes call, median (min-max) of %d rounds after %d warm-up rounds, paths alternating in "
       "one process.  The device call includes its uploads and its one download." %
       (torch.cuda.get_device_name(dev), torch.__version__, a.rounds, a.warmup), "",
       "| scenes | points per scene | boxes per scene | image | binned points | dropped points | checker (cpu) | device (cuda) |",
       "|---|---|---|---|---|---|---|---|",
       "| %d | %d | %d | %d x %d | %d | %d | %s | %s |" % (a.scenes, a.points, a.boxes, view.width, view.height, int(st["binned"].sum()),
                                                         int(st["dropped"].sum()), cell(rows["cpu"]), cell(rows["cuda"])), "",
       "Both paths give the same images and stats, byte for byte (asserted every round).  The checker is the definition, written for "
       "clarity; no speed is claimed from this table."]
print("\n".join(out))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(out) + "\n")
