"""What a checkpoint costs in a sweep, two ways, in one process on synthetic scenes (profiles/eval_sweep.md):
  (a) as a loop over `eval_rcnn --ckpt` pays inside the process: a new engine and a new runner (graphs captured again) per checkpoint;
  (b) `--eval_all`: one engine and runner, load_state_dict -> runner.reload_weights() per checkpoint.
Per checkpoint, host seconds that end in a device synchronise: load (torch.load + load_state_dict), build (a) / reload (b), the first
batch (with (a): the warm-up and the captures), the remaining batches, the AP.  The clouds are on the device before the clock starts
(loader and writer processes are the same for both ways and are not what this probe is about); a new process per checkpoint -- the
interpreter, the imports, the HIP runtime -- comes on top of (a) and is NOT in its column.

--ap_stats_device cuda runs the AP phase with its statistics on the device (kitti_eval's stats_device) against the labels' table
built once before the clock starts, as the sweep does.

  python profiles/eval_sweep_probe.py [--ckpts 4] [--scenes 512] [--batch_size 8] [--reps 3] [--ap_stats_device cpu|cuda] [--out FILE.json]"""
import argparse, gc, importlib, json, os, statistics, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
PKG = "3d_adapt_auto_driving_amd"
C = importlib.import_module(PKG + ".config"); E = importlib.import_module(PKG + ".eval_rcnn"); K = importlib.import_module(PKG + ".kitti_io")
G = importlib.import_module(PKG + ".gather")
import helpers

ap = argparse.ArgumentParser()
ap.add_argument("--ckpts", type=int, default=4); ap.add_argument("--scenes", type=int, default=512); ap.add_argument("--batch_size", type=int, default=8)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--out", type=str, default=None)
ap.add_argument("--ap_stats_device", type=str, default="cpu", choices=["cpu", "cuda"])
a = ap.parse_args()
dev = torch.device("cuda", 0); cfg = C.default_eval_cfg(); model = E.build_model(cfg, dev, seed=0)
src = K.SyntheticSource(cfg, a.scenes)
ids = list(src.ids)
B = a.batch_size
batches = [torch.from_numpy(np.stack([src.load(i)[0] for i in ids[s:s + B]], 0)).to(dev) for s in range(0, len(ids) - B + 1, B)]
ids = ids[:len(batches) * B]
M = cfg.TEST.RPN_POST_NMS_TOP_N
tmp = tempfile.mkdtemp()
files = []
for k in range(a.ckpts):
    model.load_state_dict(helpers.seeded_state_dict(model.state_dict(), 1 + k)[0])
    files.append(os.path.join(tmp, "checkpoint_epoch_%d.pth" % k))
    torch.save({"model_state": model.state_dict(), "epoch": k, "it": 0}, files[-1])
clock = time.perf_counter
prepared_gt = E.prepare_gt(src, sorted(ids)) if a.ap_stats_device == "cuda" else None


def sync():
    torch.cuda.synchronize(dev)
    return clock()


def run(runner, part):
    """-> the host copies (boxes, scores, num) of the batches `part` (indices), in order"""
    outs = []

    def take(det):
        if det is not None:
            with torch.cuda.stream(det["stream"]):
                outs.append(tuple(det[k].clone() for k in ("boxes", "scores", "num")))      # (the slot is reused a few submits later)
    for n, i in enumerate(part):
        take(runner.submit(batches[i], [batches[j] for j in part[n + 1:n + 1 + runner.depth]]))
    while True:
        det = runner.flush()
        if det is None:
            break
        take(det)
    return outs


def one(path, runner):
    """one checkpoint; runner None: way (a).  -> (seconds by phase, runner, detections)"""
    t = {}
    t0 = sync()
    E.load_checkpoint(model, path)
    t1 = sync(); t["load"] = t1 - t0
    if runner is None:
        runner = E.make_runner(model, cfg, dev)
    else:
        runner.reload_weights()
    t2 = sync(); t["build_or_reload"] = t2 - t1
    dets = run(runner, [0])
    t3 = sync(); t["first_batch"] = t3 - t2
    dets += run(runner, list(range(1, len(batches))))
    torch.cuda.synchronize(dev)
    dets = [tuple(x.cpu() for x in d) for d in dets]
    t4 = sync(); t["inference"] = t4 - t3
    table, counts = G.pack_detections(ids, dets, M)
    E.evaluate_detections(table, counts, src, stats_device=a.ap_stats_device, prepared_gt=prepared_gt)
    t["ap"] = clock() - t4
    return t, runner, dets


rows = {"a": [], "b": []}
check = {}
for rep in range(a.reps):
    for way in ("a", "b") if rep % 2 == 0 else ("b", "a"):          # alternating: other people's work shares the machine
        runner = None
        for k, path in enumerate(files):
            t, r, dets = one(path, None if way == "a" else runner)
            if way == "b":
                runner = r
            warm = way == "b" and k > 0
            rows[way].append(dict(t, ckpt=k, rep=rep, warm=warm))
            key = (k, len(dets))
            sig = [float(sum(d[1].double().sum() for d in dets)), int(sum(int(d[2].sum()) for d in dets))]
            assert check.setdefault(key, sig) == sig, "checkpoint %d: the two ways disagree (%s vs %s)" % (k, check[key], sig)
            del r
            if way == "a":                                              # (the graphs' memory pools go back before the next build)
                gc.collect(); torch.cuda.empty_cache()
        del runner
        gc.collect(); torch.cuda.empty_cache()


def column(sel, key):
    v = [r[key] for r in sel]
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


phases = ("load", "build_or_reload", "first_batch", "inference", "ap")
report = {"scenes": len(ids), "batch_size": B, "ckpts": a.ckpts, "reps": a.reps, "ap_stats_device": a.ap_stats_device,
          "a_new_engine_per_ckpt": {p: column(rows["a"], p) for p in phases},
          "b_reload_warm": {p: column([r for r in rows["b"] if r["warm"]], p) for p in phases},
          "b_first_ckpt_of_a_sweep": {p: column([r for r in rows["b"] if not r["warm"]], p) for p in phases}}
for name in ("a_new_engine_per_ckpt", "b_reload_warm"):
    report[name]["total_median"] = round(sum(report[name][p]["median"] for p in phases), 4)
print(json.dumps(report, indent=1))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"report": report, "rows": rows}, f, indent=1)
