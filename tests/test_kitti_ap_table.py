"""The split table of both AP paths and its two numpy definitions (kitti_eval.SplitTable, split_flags, thresholds_loop), the
pair-cosine host entry, the host path on that table (HostStats: its columns, its pr rows against the per-image definition, its
eval_class against its own recorded output, PreparedGT), and -- with the host entries only -- that the helper split (ap_split.py)
reaches every branch the GPU test is meant to pin: a GPU test shows nothing about a branch no input takes.  CPU; needs the built
library."""
import functools
import os

import numpy as np
import pytest

from conftest import pkg
import ap_split

HERE = os.path.dirname(os.path.abspath(__file__))
G10 = os.path.join(HERE, "golden", "g10_ap_eval_ref.npz")


@functools.lru_cache(maxsize=None)
def helper_split():
    KE = pkg("kitti_eval")
    gl, dl = ap_split.make_split(0)
    return ap_split.as_annos(KE, gl), ap_split.as_annos(KE, dl)


@functools.lru_cache(maxsize=None)
def fixture_split():
    KE = pkg("kitti_eval")
    z = np.load(G10)
    return ([KE.annos_from_lines(str(s).split("\n")) for s in z["gt_lines"]], [KE.annos_from_lines(str(s).split("\n")) for s in z["dt_lines"]])


@pytest.mark.parametrize("which", ["g10", "helper"])
def test_split_flags_equal_clean_data(which):
    KE = pkg("kitti_eval")
    gt, dt = fixture_split() if which == "g10" else helper_split()
    table = KE.SplitTable(gt, dt)
    assert table.n_img == len(gt) and table.pair_off[-1] == sum(len(g["name"]) * len(d["name"]) for g, d in zip(gt, dt))
    for metric, dataset, levels in (("new", "kitti", range(6)), ("old", "waymo", range(3))):
        for cls in (0, 1, 2):
            for difficulty in levels:
                ig, idt, nv, dc = KE.split_flags(table, cls, dataset, difficulty, metric)
                want = [KE.clean_data(g, d, cls, dataset, difficulty, metric) for g, d in zip(gt, dt)]
                assert nv == sum(w[0] for w in want)
                for i, w in enumerate(want):
                    assert np.array_equal(ig[table.gt_off[i]:table.gt_off[i + 1]], w[1]), (which, metric, cls, difficulty, i)
                    assert np.array_equal(idt[table.dt_off[i]:table.dt_off[i + 1]], w[2]), (which, metric, cls, difficulty, i)
                    assert np.array_equal(dc[table.dc_off[i]:table.dc_off[i + 1]], np.asarray(w[3]).reshape(-1, 4))
    assert ig.dtype == np.int64 and idt.dtype == np.int64


def test_prepared_gt_is_the_gt_half():
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    a, b = KE.SplitTable(gt, dt), KE.SplitTable(KE.PreparedGT(gt), dt)
    for key in ("off", "code", "is_dc", "occluded", "truncated", "bbox", "alpha", "location", "dimensions", "rotation_y", "score"):
        assert np.array_equal(getattr(a.gt, key), getattr(b.gt, key)), key
    assert np.array_equal(a.pair_off, b.pair_off) and np.array_equal(a.dc_bbox, b.dc_bbox)


def test_thresholds_loop_equals_closed_form():
    KE = pkg("kitti_eval")
    rng = np.random.RandomState(3)
    cases = [(1, 1), (1, 7), (5, 5), (41, 41), (42, 42), (48, 48), (100, 100), (100, 250), (300, 301), (40, 41)]
    cases += [(int(n), int(n + rng.randint(0, 60))) for n in rng.randint(1, 200, size=40)]
    counts = set()
    for case, (n, num_gt) in enumerate(cases):
        scores = rng.uniform(-2, 5, size=n)
        if case % 3 == 0:
            scores = np.round(scores, 1)            # ties
        s = np.sort(scores)[::-1]
        got, want = KE.thresholds_loop(s, num_gt), KE.get_thresholds(scores, num_gt)
        assert len(got) == len(want) and np.array_equal(np.array(got), np.array(want)), (n, num_gt)
        counts.add(len(got))
    assert KE.thresholds_loop(np.zeros((0,)), 5) == [] and 41 in counts and 1 in counts


def test_pair_cos_is_what_image_stats_sums():
    """The similarity of an image whose detection k matches ground-truth box k is the table's diagonal, added in order from 0.0."""
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    table = KE.SplitTable(gt, dt)
    cosv = KE.pair_cos(table)
    delta = np.concatenate([(g["alpha"][None, :] - d["alpha"][:, None]).reshape(-1) for g, d in zip(gt, dt)])
    assert cosv.shape == delta.shape and np.allclose(cosv, (1 + np.cos(delta)) / 2, rtol=0, atol=1e-15)
    i = ap_split.IMAGES["cyclists_2"]
    n = len(gt[i]["name"])
    ov = KE.image_box_overlap(dt[i]["bbox"], gt[i]["bbox"])
    tp, fp, fn, sim, nv = ap_split.image_stats(KE, gt[i], dt[i], ov, 2, 0, 0, 0.5, -1.0, 1, compute_aos=True)
    assert (tp, fp, fn, nv) == (n, 0, 0, n)
    s = 0.0
    for k in range(n):
        s += cosv[table.pair_off[i] + k * n + k]
    assert s == sim and 0 < sim < n


@functools.lru_cache(maxsize=None)
def host_curves(drop=None):
    """Host eval_class of the helper split for the image-box kind (no rotated IoU needed), optionally without some label names"""
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    if drop:
        gt = [{k: v[~np.isin(g["name"], drop)] for k, v in g.items()} if len(g["name"]) else g for g in gt]
    levels = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])
    return KE.eval_class(gt, dt, [0, 1, 2], "kitti", [0, 1, 2, 3, 4, 5], 0, levels, compute_aos=True)


def test_helper_split_reaches_what_it_claims(oracle):
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    table = KE.SplitTable(gt, dt)
    base = host_curves()
    # the rotated kinds too have a group with all 41 thresholds and one with none (overlaps from the CPU oracle of the IoU kernel)
    ext_cpu = __import__("oracle.ext_cpu", fromlist=["x"])
    for kind in (1, 2):
        with ext_cpu.patch_package():
            rot = KE.calculate_iou(dt, gt, kind)
        st = ap_split.host_stages(KE, gt, dt, 2, kind, [0.5, 0.25], [0, 5], rot)
        assert [len(st[key]["thresholds"]) for key in ((0, 0), (0, 1), (1, 0))] == [41, 41, 0], kind
    # DontCare rows exempt false positives; siblings absorb detections
    no_dc = host_curves(("DontCare",))
    assert np.array_equal(no_dc["recall"], base["recall"]) and not np.array_equal(no_dc["precision"], base["precision"])
    no_sib = host_curves(("Van", "Person_sitting"))
    assert not np.array_equal(no_sib["precision"][0], base["precision"][0]) and not np.array_equal(no_sib["precision"][1], base["precision"][1])
    # a group with all 41 thresholds, one with none, one class/difficulty without valid ground truth
    ov = [KE.image_box_overlap(d["bbox"], g["bbox"]) for g, d in zip(gt, dt)]
    st = ap_split.host_stages(KE, gt, dt, 2, 0, [0.5], [0, 4], ov)
    assert len(st[(0, 0)]["thresholds"]) == 41 and st[(0, 0)]["num_valid_gt"] == 48
    assert len(st[(1, 0)]["thresholds"]) == 0 and st[(1, 0)]["num_valid_gt"] == 0
    # images beyond the register bound of the kernels, and the sizes around a 64-bit word
    assert set(ap_split.N_DT_SIZES) <= set(table.dt_nums.tolist()) and table.max_dt == 300 > KE.REG_DETS and table.n_big == 2
    assert table.ws_slot[ap_split.IMAGES["n_dt_129"]] == 0 and table.ws_slot[ap_split.IMAGES["n_dt_300"]] == 1 and (table.ws_slot >= 0).sum() == 2
    # images with an empty side
    for name, (ng, nd) in (("no_labels", (0, 3)), ("no_detections", (4, 0)), ("neither", (0, 0))):
        i = ap_split.IMAGES[name]
        assert (table.gt_nums[i], table.dt_nums[i]) == (ng, nd)
    # the assigned_ignored_det branch: a valid box whose only overlapping detection is ignored is neither a hit nor a miss
    i = ap_split.IMAGES["ignored_only"]
    tp, fp, fn, _, nv = ap_split.image_stats(KE, gt[i], dt[i], ov[i], 0, 0, 0, 0.7, -1.0, 1)
    assert nv == 1 and (tp, fp, fn) == (0, 0, 0) and ov[i][0, 0] > 0.7
    assert KE.clean_data(gt[i], dt[i], 0, "kitti", 0)[2].tolist() == [1]
    # overlaps that EQUAL a level: strict >, so no match there, a match just below
    i = ap_split.IMAGES["exact_level"]
    assert ov[i][0, 0] == 0.7 and ov[i][1, 1] == 0.5
    assert ap_split.image_stats(KE, gt[i], dt[i], ov[i], 0, 0, 0, 0.7, -1.0, 1)[:3] == (0, 1, 1)
    assert ap_split.image_stats(KE, gt[i], dt[i], ov[i], 0, 0, 0, 0.6999, -1.0, 1)[:3] == (1, 0, 0)
    assert ap_split.image_stats(KE, gt[i], dt[i], ov[i], 1, 0, 0, 0.5, -1.0, 1)[:3] == (0, 1, 1)
    # ties inside an image and across images; a score that prints as -0.0000; every cap fails somewhere
    a, b = dt[ap_split.IMAGES["ties_a"]]["score"], dt[ap_split.IMAGES["ties_b"]]["score"]
    assert (a == 1.25).sum() > 1 and (b == 1.25).sum() > 1
    assert any("-0.0000" in line for line in ap_split.make_split(0)[1][ap_split.IMAGES["duplicates"]])
    caps = ap_split.IMAGES["caps"]
    for metric, dataset, levels in (("new", "kitti", range(6)), ("old", "waymo", range(3))):
        flags = [KE.clean_data(gt[caps], dt[caps], 0, dataset, d, metric) for d in levels]
        assert len({f[0] for f in flags}) > 1 and all((f[1] == 1).any() and (f[1] == 0).any() for f in flags)
        assert any((f[2] == 1).any() for f in flags)


def test_stats_device_cuda_without_a_device_raises_by_name(monkeypatch):
    import torch
    KE, R = pkg("kitti_eval"), pkg("results")
    gt, dt = helper_split()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(KE.StatsDeviceError, match="stats_device='cuda'"):
        KE.get_official_eval_result(gt[:4], dt[:4], 0, stats_device="cuda")
    with pytest.raises(KE.StatsDeviceError):
        KE.eval_class(gt[:4], dt[:4], [0], "kitti", [0], 0, np.full((1, 3, 1), 0.5), stats_device="cuda")
    with pytest.raises(ValueError, match="stats_device"):
        KE.get_official_eval_result(gt[:4], dt[:4], 0, stats_device="gpu")
    assert "stats_device" in R.evaluate_detections.__code__.co_varnames and "prepared_gt" in R.evaluate_detections.__code__.co_varnames


# ---------------------------------------------------------------------------------------------------
# the host path on the shared table (kitti_ap.HostStats)
# ---------------------------------------------------------------------------------------------------
def test_host_pr_is_the_image_order_sum_of_the_per_image_definition():
    """Row t of a group's pr is the sum, in image order, of prcnn_kitti_image_stats at threshold t with the columns and flags that
    ap_split.image_stats builds PER IMAGE from clean_data -- the check that does not go through the shared table.  tp / fp / fn are
    added as doubles, the similarity only where it is not -1 (the rule of the library's pass-2 entry)."""
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    hs = KE.HostStats(KE.SplitTable(gt, dt))
    ov = [KE.image_box_overlap(d["bbox"], g["bbox"]) for g, d in zip(gt, dt)]
    diffs, n_thr = [0, 1, 5], {}
    for cls, level in ((0, 0.7), (1, 0.5), (2, 0.5)):
        flags, lev = hs.flags(cls, "kitti", diffs, "new"), np.array([level])
        thr = hs.thresholds(hs.scores(flags, hs.overlaps(0), 0, lev), flags[2])
        pr = hs.pr(flags, hs.overlaps(0), 0, lev, thr, True)
        for g, difficulty in enumerate(diffs):
            want = np.zeros((len(thr[g]), 4))
            for t, thresh in enumerate(thr[g]):
                for i in range(len(gt)):
                    tp, fp, fn, sim, _ = ap_split.image_stats(KE, gt[i], dt[i], ov[i], cls, difficulty, 0, level, thresh, 1, compute_aos=True)
                    want[t, 0] += float(tp)
                    want[t, 1] += float(fp)
                    want[t, 2] += float(fn)
                    if sim != -1:
                        want[t, 3] += sim
            assert pr[g].shape == want.shape and np.array_equal(pr[g], want), (cls, difficulty)
            n_thr[(cls, difficulty)] = len(thr[g])
    assert len(n_thr) == 9 and n_thr[(2, 0)] == 41 and n_thr[(2, 5)] == 0


@pytest.mark.parametrize("which", ["g10", "helper"])
def test_host_columns_are_the_per_image_concatenation(which):
    KE = pkg("kitti_eval")
    gt, dt = fixture_split() if which == "g10" else helper_split()
    hs = KE.HostStats(KE.SplitTable(gt, dt))
    cat = lambda parts, w: np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, w) for p in parts], 0)
    want_gt = cat([np.concatenate([g["bbox"], g["alpha"][..., None]], 1) for g in gt], 5)                       # as image_stats builds them
    want_dt = cat([np.concatenate([d["bbox"], d["alpha"][..., None], d["score"][..., None]], 1) for d in dt], 6)
    dcs = [KE.clean_data(g, d, 0, "kitti", 0)[3] for g, d in zip(gt, dt)]
    for got, want in ((hs.gt_datas, want_gt), (hs.dt_datas, want_dt), (hs.dontcares, cat(dcs, 4))):
        assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and got.shape == want.shape and np.array_equal(got, want)
    for got, want in ((hs.gt_nums, [len(g["name"]) for g in gt]), (hs.dt_nums, [len(d["name"]) for d in dt]), (hs.dc_nums, [len(x) for x in dcs])):
        assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and got.tolist() == want
    for annos in (gt, dt):
        side = KE.SplitSide(annos)
        bev = np.concatenate([KE._bev_boxes(a) for a in annos], 0).astype(np.float32)
        assert side.bev.dtype == np.float32 and np.array_equal(side.bev, bev)
        assert side.box3d.dtype == np.float64 and np.array_equal(side.box3d, np.concatenate([KE._d3_boxes(a) for a in annos], 0))
        assert side.off32.dtype == np.int32 and np.array_equal(side.off32, side.off)


@pytest.mark.parametrize("which", ["g10", "helper"])
def test_host_eval_class_is_what_it_was(which, oracle):
    """Against this project's own host output recorded before the host path moved onto the table (golden/make_golden_ap_host.py)"""
    KE = pkg("kitti_eval")
    gt, dt = fixture_split() if which == "g10" else helper_split()
    z = np.load(os.path.join(HERE, "golden", "g25_ap_host_ref.npz"))
    levels = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])
    ext_cpu = __import__("oracle.ext_cpu", fromlist=["x"])
    for rule, dataset, diffs in (("new", "kitti", [0, 1, 2, 3, 4, 5]), ("old", "waymo", [0, 1, 2])):
        for kind in (0, 1, 2):
            with ext_cpu.patch_package():
                r = KE.eval_class(gt, dt, [0, 1, 2], dataset, diffs, kind, levels, compute_aos=(kind == 0), difficulty_metric=rule)
                assert KE.calculate_iou(dt[:2], gt[:2], 1)[0].dtype == np.float64                    # the rotated IoU runs without a GPU in here
            want = z["%s_%s_%d" % (which, rule, kind)]
            for c, key in enumerate(("precision", "recall", "orientation")):
                assert r[key].shape == want[c].shape and np.array_equal(r[key], want[c], equal_nan=True), (rule, kind, key)
            assert np.count_nonzero(want[0]) > 0


def test_prepared_gt_serves_the_host_path(oracle):
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    ext_cpu = __import__("oracle.ext_cpu", fromlist=["x"])
    with ext_cpu.patch_package():
        for kw in ({"metric": "new"}, {"metric": "old", "dataset": "waymo"}):
            want, _ = KE.get_official_eval_result(gt, dt, [0, 1, 2], **kw)
            text, _ = KE.get_official_eval_result(KE.PreparedGT(gt), dt, [0, 1, 2], **kw)
            assert text == want and "aos" in want
