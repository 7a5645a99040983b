"""A small adversarial split for the AP statistics, as KITTI label / result lines (helper of test_kitti_ap_table.py and
test_gpu_kitti_ap.py; no test lives here).  Seeded; every image is written for a reason, named in IMAGES:

  * an image with no labels, one with no detections, one with neither;
  * DontCare boxes over detections that match nothing; siblings (Van under a Car detection, Person_sitting under a Pedestrian);
  * ground truth failing each cap (occlusion, truncation, distance band, bbox height) and detections outside the band;
  * equal scores inside an image and across images; duplicated detections (equal overlaps); a score that prints as -0.0000;
  * image-box overlaps that EQUAL a level of min_overlaps (0.7 for Car, 0.5 for Pedestrian): the comparison is a strict >;
  * images with 1, 31, 32, 33, 64, 65, 129 and 300 detections (the kernels keep 128 per image in registers);
  * 48 cyclists within 30 m, each detected a few centimetres off (coincident rotated boxes are a degenerate case of the overlap
    kernel, not this split's subject): those groups take all 41 thresholds; none beyond 30 m: groups with no valid ground truth
    and no threshold;
  * a valid Car at 29.9 m whose only overlapping detection stands at 30.1 m (ignored in the 0-30 m band).
"""
import numpy as np

FOCAL = 2000.0
DIMS = {"Car": (1.5, 1.6, 3.9), "Van": (2.0, 1.9, 5.0), "Pedestrian": (1.7, 0.6, 0.8), "Person_sitting": (1.2, 0.6, 0.8),
        "Cyclist": (1.7, 0.6, 1.8)}
N_DT_SIZES = (1, 31, 32, 33, 64, 65, 129, 300)
IMAGES = {}                                          # name -> image index, filled by make_split


def bbox_of(x, y, z, h, w, l):
    zz = max(z, 0.5)
    half = FOCAL * max(l, w) / zz / 2
    cx = 960 + FOCAL * x / zz
    return [cx - half, 400 + FOCAL * (y - h) / zz, cx + half, 400 + FOCAL * y / zz]


def gt_line(name, x, z, ry=0.0, occ=0, trunc=0.0, y=1.6, bbox=None, alpha=None, dims=None):
    h, w, l = dims or DIMS.get(name, (1.5, 1.6, 3.9))
    b = bbox or bbox_of(x, y, z, h, w, l)
    alpha = ry * 0.5 if alpha is None else alpha
    return "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (name, trunc, occ, alpha, b[0], b[1], b[2], b[3],
                                                                                   h, w, l, x, y, z, ry)


def dt_line(name, x, z, score, ry=0.0, y=1.6, bbox=None, alpha=None, dims=None):
    h, w, l = dims or DIMS.get(name, (1.5, 1.6, 3.9))
    b = bbox or bbox_of(x, y, z, h, w, l)
    alpha = ry * 0.5 + 0.1 if alpha is None else alpha
    return "%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f" % (name, alpha, b[0], b[1], b[2], b[3], h, w, l,
                                                                                       x, y, z, ry, score)


def make_split(seed=0):
    """-> (gt_lines, dt_lines): per image a list of lines"""
    rng = np.random.RandomState(seed)
    gts, dts = [], []

    def image(name, gt, dt):
        IMAGES[name] = len(gts)
        gts.append(gt)
        dts.append(dt)

    def scene(n_car, n_ped, n_dt, tie=None):
        """n_car + n_ped labels at random places, detections on them with graded noise, then clutter up to n_dt"""
        gt, dt = [], []
        for k in range(n_car + n_ped):
            name = "Car" if k < n_car else "Pedestrian"
            x, z, ry = rng.uniform(-15, 15), rng.uniform(4, 68), rng.uniform(-3, 3)
            gt.append(gt_line(name, x, z, ry, occ=int(rng.randint(0, 3)), trunc=float(rng.choice([0.0, 0.1, 0.25, 0.45]))))
            if len(dt) < n_dt:
                s = float(rng.choice([0.0, 0.03, 0.1, 0.3]))
                score = tie if tie is not None and k % 2 == 0 else rng.uniform(-1, 4)
                dt.append(dt_line(name, x + rng.normal(0, s), z + rng.normal(0, s), score, ry + rng.normal(0, s / 3)))
        while len(dt) < n_dt:
            name = "Car" if rng.rand() < 0.7 else ("Pedestrian" if rng.rand() < 0.7 else "Cyclist")
            dt.append(dt_line(name, rng.uniform(-20, 20), rng.uniform(2, 75), round(rng.uniform(-2, 3), int(rng.randint(1, 5))),
                              rng.uniform(-3, 3)))
        return gt, dt

    image("no_labels", [], scene(0, 0, 3)[1])
    image("no_detections", scene(3, 1, 0)[0], [])
    image("neither", [], [])
    # two Car detections inside a DontCare region match nothing; one Pedestrian detection likewise
    image("dontcare", [gt_line("Car", 0.0, 12.0), gt_line("DontCare", -1000, -1000, y=-1000, bbox=[100, 100, 700, 500], dims=(-1, -1, -1)),
                       gt_line("DontCare", -1000, -1000, y=-1000, bbox=[1500, 50, 1900, 300], dims=(-1, -1, -1))],
          [dt_line("Car", 0.02, 12.01, 2.5), dt_line("Car", -9.0, 25.0, 1.5, bbox=[200, 200, 300, 260]),
           dt_line("Car", -8.0, 20.0, 0.5, bbox=[400, 150, 520, 230]), dt_line("Pedestrian", 9.0, 18.0, 1.0, bbox=[1600, 100, 1640, 200]),
           dt_line("Car", 9.0, 40.0, 0.7)])
    image("siblings", [gt_line("Van", 3.0, 15.0), gt_line("Person_sitting", -4.0, 10.0), gt_line("Car", -8.0, 22.0), gt_line("Tram", 10.0, 30.0)],
          [dt_line("Car", 3.0, 15.0, 1.9, dims=DIMS["Van"]), dt_line("Pedestrian", -4.0, 10.0, 1.2, dims=DIMS["Person_sitting"]),
           dt_line("Car", -8.05, 22.0, 2.2)])
    caps_gt, caps_dt = [], []
    for k, (occ, trunc, z, hpx) in enumerate([(0, 0.0, 10, 200), (1, 0.0, 10, 200), (2, 0.0, 10, 200), (3, 0.0, 10, 200), (0, 0.2, 12, 150),
                                              (0, 0.4, 12, 150), (0, 0.6, 12, 150), (0, 0.0, 35, 100), (0, 0.0, 55, 80), (0, 0.0, 75, 60),
                                              (0, 0.0, 20, 117.09), (0, 0.0, 20, 73.18), (0, 0.0, 20, 30), (0, 0.0, 30.0, 120),
                                              (0, 0.0, 50.0, 90), (0, 0.15, 8, 180), (0, 0.3, 8, 180), (0, 0.5, 8, 180)]):
        x = -17.0 + 2.0 * k
        box = [500 + 60 * k, 300.0, 540 + 60 * k, 300.0 + hpx]
        for name in ("Car", "Pedestrian"):
            caps_gt.append(gt_line(name, x, float(z) + (0.0 if name == "Car" else 1.5), occ=occ, trunc=trunc, bbox=box))
            caps_dt.append(dt_line(name, x, float(z) + (0.0 if name == "Car" else 1.5), 3.0 - 0.1 * k, bbox=box))
    image("caps", caps_gt, caps_dt)
    image("out_of_band", [gt_line("Car", 0.0, 20.0), gt_line("Pedestrian", 5.0, 45.0)],
          [dt_line("Car", 0.0, 80.0, 2.0), dt_line("Car", 1.0, -5.0, 1.0), dt_line("Car", 0.0, 20.0, 0.9, bbox=[10, 10, 30, 20]),
           dt_line("Pedestrian", 5.0, 45.0, 0.4), dt_line("Car", 0.0, 70.0, 0.3), dt_line("Car", 0.0, 30.0, 0.2)])
    image("ties_a", *scene(5, 3, 8, tie=1.25))
    image("ties_b", *scene(4, 4, 8, tie=1.25))
    image("duplicates", [gt_line("Car", 2.0, 14.0), gt_line("Pedestrian", -3.0, 9.0)],
          [dt_line("Car", 2.03, 14.0, 1.0), dt_line("Car", 2.03, 14.0, 1.0), dt_line("Car", 2.03, 14.0, 2.0),
           dt_line("Pedestrian", -3.0, 9.02, 0.5), dt_line("Pedestrian", -3.0, 9.02, 0.5), dt_line("Car", 6.0, 30.0, -0.00001)])
    # image-box overlap exactly 0.7 (Car) and exactly 0.5 (Pedestrian): no match at those levels in the image-box kind
    image("exact_level", [gt_line("Car", 0.0, 10.0, bbox=[0, 0, 100, 100]), gt_line("Pedestrian", 6.0, 10.0, bbox=[300, 0, 400, 100])],
          [dt_line("Car", 0.0, 10.0, 1.7, bbox=[0, 0, 100, 70]), dt_line("Pedestrian", 6.0, 10.0, 1.1, bbox=[300, 0, 400, 50])])
    for n in N_DT_SIZES:
        image("n_dt_%d" % n, *scene(6, 3, n))
    for part in range(6):                            # 48 cyclists within 30 m, each detected closely, distinct scores
        ks = range(part * 8, part * 8 + 8)
        image("cyclists_%d" % part, [gt_line("Cyclist", -14.0 + 4.0 * (k % 8), 5.0 + 0.45 * k, 0.1 * k) for k in ks],
              [dt_line("Cyclist", -13.97 + 4.0 * (k % 8), 5.02 + 0.45 * k, 0.5 + 0.05 * k, 0.1 * k + 0.01, alpha=0.05 * k - 1.0) for k in ks])
    image("ignored_only", [gt_line("Car", 0.0, 29.9)], [dt_line("Car", 0.0, 30.1, 1.4, bbox=bbox_of(0.0, 1.6, 29.9, *DIMS["Car"]))])
    for k in range(4):
        image("plain_%d" % k, *scene(7, 4, 12))
    return gts, dts


def as_annos(KE, lines):
    return [KE.annos_from_lines(l) for l in lines]


def _p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def host_stages(KE, gt, dt, current_class, kind, levels, difficultys, overlaps, dataset="kitti", metric="new", compute_aos=False):
    """The host path of eval_class, stage by stage (KE.HostStats), for one class: per (difficulty index, level index) a dict with the
    pass-1 scores sorted descending, num_valid_gt, the thresholds, pr (n_thresholds, 4) and the two flag vectors."""
    hs = KE.HostStats(KE.SplitTable(gt, dt))
    flat = np.ascontiguousarray(np.concatenate([np.asarray(o, dtype=np.float64).reshape(-1) for o in overlaps]), dtype=np.float64)
    levels = np.asarray(levels, dtype=np.float64)
    flags = hs.flags(current_class, dataset, difficultys, metric)
    scores = hs.scores(flags, flat, kind, levels)
    thr = hs.thresholds(scores, flags[2])
    pr = hs.pr(flags, flat, kind, levels, thr, compute_aos)
    out = {}
    for l in range(len(difficultys)):
        for k in range(len(levels)):
            g = l * len(levels) + k
            out[(l, k)] = {"scores": np.sort(scores[g])[::-1], "num_valid_gt": int(flags[2][l]), "thresholds": thr[g], "pr": pr[g],
                           "ignored_gt": flags[0][l], "ignored_dt": flags[1][l]}
    return out


def image_stats(KE, gt_anno, dt_anno, overlap, current_class, difficulty, kind, level, thresh, compute_fp, compute_aos=False,
                dataset="kitti", metric="new"):
    """prcnn_kitti_image_stats of one image -> (tp, fp, fn, similarity, num_valid_gt)"""
    import ctypes
    nv, ig, idt, dc = KE.clean_data(gt_anno, dt_anno, current_class, dataset, difficulty, metric)
    gtd = np.ascontiguousarray(np.concatenate([gt_anno["bbox"], gt_anno["alpha"][..., None]], 1), dtype=np.float64).reshape(-1, 5)
    dtd = np.ascontiguousarray(np.concatenate([dt_anno["bbox"], dt_anno["alpha"][..., None], dt_anno["score"][..., None]], 1),
                               dtype=np.float64).reshape(-1, 6)
    dcb = np.ascontiguousarray(dc, dtype=np.float64).reshape(-1, 4)
    o = np.ascontiguousarray(overlap, dtype=np.float64)
    tpfpfn, thr = np.zeros(3, np.int64), np.zeros(max(1, len(ig)), np.float64)
    sim, nth = ctypes.c_double(0), ctypes.c_int(0)
    KE._lib.call("prcnn_kitti_image_stats", len(ig), len(idt), len(dcb), _p(o), _p(gtd), _p(dtd), _p(ig), _p(idt), _p(dcb), int(kind),
                 float(level), float(thresh), int(compute_fp), int(compute_aos), _p(tpfpfn), ctypes.cast(ctypes.pointer(sim), ctypes.c_void_p),
                 _p(thr), ctypes.cast(ctypes.pointer(nth), ctypes.c_void_p))
    return int(tpfpfn[0]), int(tpfpfn[1]), int(tpfpfn[2]), sim.value, nv
