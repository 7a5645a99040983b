"""car_split.py, --parse_device cpu against cuda, in one process on the synthetic label files of profiles/kitti_ap_probe.py (about 10
label lines per file, six of them cars): writes profiles/car_split_probe.md.  Per file count a dataset-layout tree is written once
(train.txt lists the files, val.txt the first 64 of them), then the two paths alternate: warm-up rounds, then median (min to max) of the
timed ones.  All times are host time in ms around the whole car_split() call -- split files read, label files read (from the page
cache: the tree was just written), the rule, the shuffles, the two files written; the cuda path ends in a device synchronise.  The
cuda path's own read of the label files (kitti_annos.read_texts, 16 threads) is timed inside it by wrapping the function.

  python profiles/car_split_probe.py [--files 3769 50000] [--rounds 5] [--warmup 2] [--out profiles/car_split_probe.md]"""
import argparse, ast, importlib, os, shutil, statistics, sys, tempfile, time
import numpy as np, torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
CS = importlib.import_module("3d_adapt_auto_driving_amd.car_split")
KA = importlib.import_module("3d_adapt_auto_driving_amd.kitti_annos")

ap = argparse.ArgumentParser()
ap.add_argument("--files", type=int, nargs="*", default=[3769, 50000])
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", type=str, default=os.path.join(HERE, "car_split_probe.md"))
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


def write_tree(root, labels):
    os.makedirs(os.path.join(root, "training", "label_2"))
    for i, lines in enumerate(labels):
        with open(os.path.join(root, "training", "label_2", "%06d.txt" % i), "w") as f:
            f.write("\n".join(lines) + "\n")
    for split, n in (("train", len(labels)), ("val", min(64, len(labels)))):
        with open(os.path.join(root, split + ".txt"), "w") as f:
            f.write("".join("%06d\n" % i for i in range(n)))


read_seconds = [0.0]
real_read = KA.read_texts


def timed_read(folder, ids):
    t0 = clock()
    out = real_read(folder, ids)
    read_seconds[0] += clock() - t0
    return out


KA.read_texts = timed_read


def run(root, device):
    read_seconds[0] = 0.0
    torch.cuda.synchronize(dev)
    t0 = clock()
    written = CS.car_split([root], parse_device=device, log=lambda *x: None)
    torch.cuda.synchronize(dev)
    return {"total": clock() - t0, "read": read_seconds[0]}, written


def cell(rows, key):
    v = [1e3 * r[key] for r in rows]
    return "%.1f (%.1f-%.1f)" % (statistics.median(v), min(v), max(v))


synthetic_lines = synthetic_lines_of_the_ap_probe()
out = ["# car_split, --parse_device cpu against cuda (profiles/car_split_probe.py)", "",
       "%s, torch %s; ms of host time around the whole call (file reads from the page cache included), median (min-max) of %d rounds "
       "after %d warm-up rounds, paths alternating in one process." % (torch.cuda.get_device_name(dev), torch.__version__, a.rounds, a.warmup), "",
       "| label files | lines | bytes | kept (train) | cpu | cuda | of it: reading the files (16 threads) | host-decided files |", "|---|---|---|---|---|---|---|---|"]
for n in a.files:
    labels, _ = synthetic_lines(n)
    root = tempfile.mkdtemp(prefix="car_split_probe_")
    try:
        write_tree(root, labels)
        rows, answers = {"cpu": [], "cuda": []}, {}
        for rnd in range(a.warmup + a.rounds):
            for device in ("cpu", "cuda") if rnd % 2 == 0 else ("cuda", "cpu"):
                t, answers[device] = run(root, device)
                if rnd >= a.warmup:
                    rows[device].append(t)
            assert answers["cpu"] == answers["cuda"], "the two paths disagree"
            print("files=%d round %d done" % (n, rnd), file=sys.stderr, flush=True)
        kept = len(answers["cuda"][os.path.join(root, "train_car1.txt")].split("\n"))
        host = CS.kept_names(root, "train", parse_device="cuda")[2]
        out.append("| %d | %d | %d | %d | %s | %s | %s | %d |" % (n, sum(len(x) for x in labels), sum(len("\n".join(x)) + 1 for x in labels), kept,
                                                             cell(rows["cpu"], "total"), cell(rows["cuda"], "total"), cell(rows["cuda"], "read"), host))
    finally:
        shutil.rmtree(root, ignore_errors=True)
out += ["", "Both paths write the same bytes (asserted every round).  The files are synthetic and sit in the page cache; a cold tree on a disk "
        "or a network file system was not measured, and there the reads, which both paths do, are the larger part."]
print("\n".join(out))
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(out) + "\n")
