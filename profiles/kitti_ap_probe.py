"""Where the KITTI AP evaluation spends its time, host path against device path (stats_device "cpu" / "cuda"), in one process on
synthetic annotations (profiles/kitti_ap_probe.md): per configuration both paths alternate, 3 warm-up rounds, then median (min to max)
of 7.  Every stage is host time; the device path's stages end in a device synchronise (so its total carries six synchronises the
uninstrumented call does not make; the last rows give the uninstrumented calls).

  host stages   : parse (both sides' lines -> annotations), table + flags (SplitTable, HostStats's columns, split_flags of the six
                  difficulties), overlaps, pass 1, thresholds, pass 2, rest (curves, mAP, text)
  device stages : parse (the same), table (SplitTable + uploads + the host-made cosine terms), flags, overlaps, pass 1,
                  sort + thresholds, pass 2, read (+ curves, mAP, text)

  python profiles/kitti_ap_probe.py [--images 512 3769] [--dense 512] [--rounds 7] [--warmup 3] [--out FILE.json]"""
import argparse, importlib, json, os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = "3d_adapt_auto_driving_amd"
KE = importlib.import_module(PKG + ".kitti_eval")

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, nargs="*", default=[512, 3769]); ap.add_argument("--dense", type=int, nargs="*", default=[512])
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
clock = time.perf_counter


def sync():
    torch.cuda.synchronize(dev)
    return clock()


def synthetic_lines(n_img, seed=0):
    """about 10 labels x 12 detections per image, as text: cars and pedestrians over 4..68 m, a Van, a DontCare region, detections
    on most labels with graded noise and some clutter"""
    rng = np.random.RandomState(seed)
    dims = {"Car": (1.5, 1.6, 3.9), "Pedestrian": (1.7, 0.6, 0.8), "Van": (2.0, 1.9, 5.0)}

    def bbox(x, y, z, h, w, l):
        half = 700.0 * max(l, w) / z / 2
        return (600 + 700.0 * x / z - half, 180 + 700.0 * (y - h) / z, 600 + 700.0 * x / z + half, 180 + 700.0 * y / z)
    gts, dts = [], []
    for _ in range(n_img):
        gt, dt = [], []
        for k in range(9):
            name = "Van" if k == 8 else ("Car" if k < 6 else "Pedestrian")
            h, w, l = dims[name]
            x, z, ry = rng.uniform(-20, 20), rng.uniform(4, 68), rng.uniform(-3.1, 3.1)
            gt.append("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" %
                      ((name, rng.choice([0.0, 0.1, 0.3]), rng.randint(0, 3), ry * 0.5) + bbox(x, 1.6, z, h, w, l) + (h, w, l, x, 1.6, z, ry)))
            if k != 5:
                s = rng.choice([0.02, 0.05, 0.15, 0.4])
                x, z, ry = x + rng.normal(0, s), z + rng.normal(0, s), ry + rng.normal(0, s / 3)
                dt.append("%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" %
                          (("Car" if name == "Van" else name, ry * 0.5) + bbox(x, 1.6, z, h, w, l) + (h, w, l, x, 1.6, z, ry, rng.uniform(-1, 4))))
        gt.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10" % (100, 120, 400, 260))
        for k in range(4):
            h, w, l = dims["Car"]
            x, z, ry = rng.uniform(-20, 20), rng.uniform(4, 75), rng.uniform(-3.1, 3.1)
            dt.append("Car -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" %
                      ((ry * 0.5,) + bbox(x, 1.6, z, h, w, l) + (h, w, l, x, 1.6, z, ry, rng.uniform(-2, 2))))
        gts.append(gt); dts.append(dt)
    return gts, dts


def min_overlaps(dense):
    o7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5]] * 3)
    o5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25], [0.5, 0.25, 0.25, 0.5, 0.25]])
    extra = []
    if dense:
        for i in range(101):
            t = np.zeros((3, 5)); t[:, 0] = i / 100.0; extra.append(t)
    return np.stack([o7, o5] + extra, 0)[:, :, [0]]


DIFFS = [0, 1, 2, 3, 4, 5]


def host_path(gl, dl, dense):
    t, t0 = {k: 0.0 for k in ("parse", "table + flags", "overlaps", "pass 1", "thresholds", "pass 2")}, clock()
    gt, dt = [KE.annos_from_lines(x) for x in gl], [KE.annos_from_lines(x) for x in dl]
    t1 = clock(); t["parse"] = t1 - t0
    hs = KE.HostStats(KE.SplitTable(gt, dt))
    flags = hs.flags(0, "kitti", DIFFS, "new")
    t["table + flags"] = clock() - t1
    mo = min_overlaps(dense)
    curves = []
    for kind in (0, 1, 2):
        s = clock()
        ov, lev = hs.overlaps(kind), mo[:, kind, 0]
        s1 = clock(); t["overlaps"] += s1 - s
        scores = hs.scores(flags, ov, kind, lev)
        s2 = clock(); t["pass 1"] += s2 - s1
        thr = hs.thresholds(scores, flags[2])
        s3 = clock(); t["thresholds"] += s3 - s2
        pr = hs.pr(flags, ov, kind, lev, thr, kind == 0)
        t["pass 2"] += clock() - s3
        shape = [1, 6, len(mo), 41]
        prec, rec, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        for g, rows in enumerate(pr):
            l, k = divmod(g, len(mo))
            KE._fill_curves(prec[0, l, k], rec[0, l, k], aos[0, l, k], rows, kind == 0)
        curves.append((prec, aos))
    t["total"] = clock() - t0
    t["rest"] = t["total"] - sum(v for k, v in t.items() if k != "total")
    return t, [KE.get_mAP(c[0]) for c in curves] + [KE.get_mAP(curves[0][1])]


def device_path(gl, dl, dense):
    t, t0 = {k: 0.0 for k in ("parse", "table", "flags", "overlaps", "pass 1", "sort + thresholds", "pass 2", "read")}, sync()
    gt, dt = [KE.annos_from_lines(x) for x in gl], [KE.annos_from_lines(x) for x in dl]
    t1 = clock(); t["parse"] = t1 - t0
    ds = KE.DeviceStats(KE.SplitTable(gt, dt))
    ds.pair_cos()
    t2 = sync(); t["table"] = t2 - t1
    flags = ds.flags(0, "kitti", DIFFS, "new")
    t3 = sync(); t["flags"] = t3 - t2
    mo = min_overlaps(dense)
    n_lev, width = len(mo), 4 * 41
    step = ds.level_chunk(6, n_lev)
    outs = []
    for kind in (0, 1, 2):
        s = sync()
        ov = ds.overlaps(kind)
        s1 = sync(); t["overlaps"] += s1 - s
        out = torch.zeros((6, n_lev, width + 1), dtype=torch.float64, device=dev)
        levels = ds._up(np.ascontiguousarray(mo[:, kind, 0]))
        for k0 in range(0, n_lev, step):
            s = sync()
            lev = levels[k0:k0 + step]
            scores, valid = ds.scores(flags, ov, kind, lev)
            s1 = sync(); t["pass 1"] += s1 - s
            _, _, thr, n_thr = ds.thresholds(scores, valid, flags[2])
            s2 = sync(); t["sort + thresholds"] += s2 - s1
            pr = ds.pr(flags, ov, kind, lev, thr, n_thr, kind == 0)
            out[:, k0:k0 + step, :width] = pr.view(6, lev.shape[0], width)
            out[:, k0:k0 + step, width] = n_thr.view(6, lev.shape[0]).double()
            t["pass 2"] += sync() - s2
        outs.append(out)
    s = sync()
    res = []
    for kind, out in enumerate(outs):
        host = out.cpu().numpy()
        n_thr, pr = host[..., width].astype(np.int64), host[..., :width].reshape(6, n_lev, 41, 4)
        shape = [1, 6, n_lev, 41]
        prec, rec, aos = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        for l in range(6):
            for k in range(n_lev):
                KE._fill_curves(prec[0, l, k], rec[0, l, k], aos[0, l, k], pr[l, k, :n_thr[l, k]], kind == 0)
        res.append((prec, aos))
    t["read"] = clock() - s
    t["total"] = clock() - t0
    return t, [KE.get_mAP(c[0]) for c in res] + [KE.get_mAP(res[0][1])]


def whole(gl, dl, dense, stats_device):
    """the public call, uninstrumented: parse + get_official_eval_result"""
    t0 = sync()
    gt, dt = [KE.annos_from_lines(x) for x in gl], [KE.annos_from_lines(x) for x in dl]
    text, _ = KE.get_official_eval_result(gt, dt, 0, "kitti", dense_sample=dense, stats_device=stats_device)
    return {"total": clock() - t0}, text


def column(rows, key):
    v = [1e3 * r[key] for r in rows]
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


report = []
for n_img, dense in [(n, False) for n in a.images] + [(n, True) for n in a.dense]:
    gl, dl = synthetic_lines(n_img)
    rows = {"host": [], "device": [], "host call": [], "device call": []}
    paths = (("host", lambda: host_path(gl, dl, dense)), ("device", lambda: device_path(gl, dl, dense)))
    if not dense:                                    # (the dense host call alone is tens of seconds a round: its staged run stands for it)
        paths += (("host call", lambda: whole(gl, dl, dense, "cpu")), ("device call", lambda: whole(gl, dl, dense, "cuda")))
    answers = {}
    for rnd in range(a.warmup + a.rounds):
        for name, fn in paths if rnd % 2 == 0 else paths[::-1]:
            t, ans = fn()
            if rnd >= a.warmup:
                rows[name].append(t)
            answers[name] = ans
        print("images=%d dense=%s round %d done" % (n_img, dense, rnd), file=sys.stderr, flush=True)
        assert all(np.array_equal(x, y) for x, y in zip(answers["host"], answers["device"])), "the two paths disagree on the mAPs"
        assert answers.get("host call") == answers.get("device call"), "the two paths disagree on the text"
    n_box = (sum(len(x) for x in gl), sum(len(x) for x in dl))
    report.append({"images": n_img, "dense_sample": dense, "labels": n_box[0], "detections": n_box[1], "rounds": a.rounds,
                   **{name: {k: column(r, k) for k in r[0]} for name, r in rows.items() if r}})
print(json.dumps(report, indent=1))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
