"""The label / result text parser, host against device (kitti_annos.parse_texts, csrc/kitti_parse.hip), in one process on the synthetic
annotations of profiles/kitti_ap_probe.py (about 10 labels x 12 detections per image): writes profiles/kitti_parse_probe.md.  Per
image count the paths alternate, 3 warm-up rounds, then median (min to max) of 7; all times are host time in ms, the device paths end in
a device synchronise.

  parser     : both sides' text -> the columns of both SplitSides.  host: annos_from_lines per image (one float() per token), then
               SplitSide over the dicts.  device: parse_texts(texts, "cuda"): upload, scan, small read, parse, read.
  whole call : parse + get_official_eval_result(..., stats_device="cuda"), host-parsed dicts against device-parsed sides; the two texts
               are asserted equal.

The host parser is the code every earlier revision ran: it is its own baseline.

  python profiles/kitti_parse_probe.py [--images 512 3769] [--rounds 7] [--warmup 3] [--out profiles/kitti_parse_probe.md]"""
import argparse, ast, importlib, os, statistics, sys, time
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
KE = importlib.import_module("3d_adapt_auto_driving_amd.kitti_eval")

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, nargs="*", default=[512, 3769])
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", type=str, default=os.path.join(HERE, "kitti_parse_probe.md"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
clock = time.perf_counter


def synthetic_lines_of_the_ap_probe():
    """kitti_ap_probe.synthetic_lines, taken from its source (the probe runs on import)"""
    with open(os.path.join(HERE, "kitti_ap_probe.py")) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "synthetic_lines"]
    scope = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "kitti_ap_probe.py", "exec"), scope)
    return scope["synthetic_lines"]


def sync():
    torch.cuda.synchronize(dev)
    return clock()


def host_parse(gl, dl, gt_texts, dt_texts):
    t0 = clock()
    gt, dt = [KE.annos_from_lines(x) for x in gl], [KE.annos_from_lines(x) for x in dl]
    t1 = clock()
    sides = KE.SplitSide(gt), KE.SplitSide(dt)
    return {"lines -> dicts": t1 - t0, "dicts -> columns": clock() - t1, "total": clock() - t0}, sides


def device_parse(gl, dl, gt_texts, dt_texts):
    t0 = sync()
    sides = KE.parse_texts(gt_texts, "cuda"), KE.parse_texts(dt_texts, "cuda")
    return {"total": sync() - t0}, sides


def host_call(gl, dl, gt_texts, dt_texts):
    t0 = sync()
    gt, dt = [KE.annos_from_lines(x) for x in gl], [KE.annos_from_lines(x) for x in dl]
    text, _ = KE.get_official_eval_result(gt, dt, 0, "kitti", stats_device="cuda")
    return {"total": sync() - t0}, text


def device_call(gl, dl, gt_texts, dt_texts):
    t0 = sync()
    gt, dt = KE.parse_texts(gt_texts, "cuda"), KE.parse_texts(dt_texts, "cuda")
    text, _ = KE.get_official_eval_result(gt, dt, 0, "kitti", stats_device="cuda")
    return {"total": sync() - t0}, text


def cell(rows, key):
    v = [1e3 * r[key] for r in rows]
    return "%.1f (%.1f-%.1f)" % (statistics.median(v), min(v), max(v))


synthetic_lines = synthetic_lines_of_the_ap_probe()
out = ["# The text parser, host against device (profiles/kitti_parse_probe.py)", "",
       "%s, torch %s; ms of host time, median (min-max) of %d rounds after %d warm-up rounds, paths alternating in one process." %
       (torch.cuda.get_device_name(dev), torch.__version__, a.rounds, a.warmup), "",
       "| images | labels | detections | bytes | host: lines -> dicts | host: dicts -> columns | host parser | device parser | "
       "whole call, host parser | whole call, device parser |", "|---|---|---|---|---|---|---|---|---|---|"]
for n_img in a.images:
    gl, dl = synthetic_lines(n_img)
    args = (gl, dl, ["\n".join(x) + "\n" for x in gl], ["\n".join(x) + "\n" for x in dl])
    paths = (("host", host_parse), ("device", device_parse), ("host call", host_call), ("device call", device_call))
    rows, answers = {name: [] for name, _ in paths}, {}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in paths if rnd % 2 == 0 else paths[::-1]:
            t, answers[name] = fn(*args)
            if rnd >= a.warmup:
                rows[name].append(t)
        print("images=%d round %d done" % (n_img, rnd), file=sys.stderr, flush=True)
        for h, d in zip(answers["host"], answers["device"]):
            assert d.parse_stats["host_files"] == 0
            assert all(getattr(h, k).tobytes() == getattr(d, k).tobytes() for k in list(KE.SplitSide.COLUMNS) + ["off", "code", "is_dc"])
        assert answers["host call"] == answers["device call"], "the two paths disagree on the text"
    out.append("| %d | %d | %d | %d | %s | %s | %s | %s | %s | %s |" %
               (n_img, sum(len(x) for x in gl), sum(len(x) for x in dl), sum(len(x) for x in args[2] + args[3]),
                cell(rows["host"], "lines -> dicts"), cell(rows["host"], "dicts -> columns"), cell(rows["host"], "total"),
                cell(rows["device"], "total"), cell(rows["host call"], "total"), cell(rows["device call"], "total")))
out += ["", "Both parsers give the same columns, bit for bit, and both whole calls the same result text (asserted every round)."]
print("\n".join(out))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(out) + "\n")
