"""The AP statistics on the device (csrc/kitti_ap.hip through kitti_eval's stats_device="cuda") against the host path: the
reference's own run (fixture g10) character for character, and the adversarial split of ap_split.py stage by stage, bit for bit.
No tolerance anywhere: flags are comparisons, overlaps the same IEEE operations in the same order, counts integers, and the
orientation similarity adds host-made terms in the host's order."""
import contextlib
import functools
import io
import os

import numpy as np
import pytest

from conftest import pkg
import ap_split

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G10 = os.path.join(HERE, "golden", "g10_ap_eval_ref.npz")
LEVELS = np.array([[[0.7, 0.5, 0.5]] * 3, [[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]])       # [level, kind, class]
DIFFS = [0, 1, 2, 3, 4, 5]


@functools.lru_cache(maxsize=None)
def helper_split():
    KE = pkg("kitti_eval")
    gl, dl = ap_split.make_split(0)
    return ap_split.as_annos(KE, gl), ap_split.as_annos(KE, dl)


@functools.lru_cache(maxsize=None)
def host_overlaps(kind):
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    return KE.calculate_iou(dt, gt, kind)


@functools.lru_cache(maxsize=None)
def device_split():
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    return KE.DeviceStats(KE.SplitTable(gt, dt))


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_fixture_g10_text_and_curves(oracle):
    KE = pkg("kitti_eval")
    z = np.load(G10)
    gt = [KE.annos_from_lines(str(s).split("\n")) for s in z["gt_lines"]]
    dt = [KE.annos_from_lines(str(s).split("\n")) for s in z["dt_lines"]]
    text, ret = KE.get_official_eval_result(gt, dt, 0, "kitti", stats_device="cuda")
    assert text == str(z["result_text"])
    for metric in (0, 1, 2):
        host = KE.eval_class(gt, dt, [0, 1], "kitti", DIFFS, metric, LEVELS[:, :, :2], compute_aos=(metric == 0))
        dev = KE.eval_class(gt, dt, [0, 1], "kitti", DIFFS, metric, LEVELS[:, :, :2], compute_aos=(metric == 0), stats_device="cuda")
        for key in ("precision", "recall", "orientation"):
            assert same(dev[key], host[key]), (metric, key)
        assert np.count_nonzero(host["precision"]) > 0
    # a caller's overlap blocks are taken as they are
    ov = KE.calculate_iou(dt, gt, 2)
    host = KE.eval_class(gt, dt, [0], "kitti", DIFFS, 2, LEVELS[:, :, :1], overlaps=ov)
    dev = KE.eval_class(gt, dt, [0], "kitti", DIFFS, 2, LEVELS[:, :, :1], overlaps=ov, stats_device="cuda")
    assert same(dev["precision"], host["precision"]) and same(dev["recall"], host["recall"])


@pytest.mark.parametrize("metric,dataset", [("new", "kitti"), ("old", "waymo")])
def test_helper_flags(metric, dataset):
    KE = pkg("kitti_eval")
    ds = device_split()
    levels = DIFFS if metric == "new" else [0, 1, 2]
    for cls in (0, 1, 2):
        ig, idt, nv = (t.cpu().numpy() for t in ds.flags(cls, dataset, levels, metric))
        for l, d in enumerate(levels):
            w_ig, w_idt, w_nv, _ = KE.split_flags(ds.table, cls, dataset, d, metric)
            assert np.array_equal(ig[l], w_ig) and np.array_equal(idt[l], w_idt) and nv[l] == w_nv, (metric, cls, d)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_helper_overlaps_bit_equal(kind):
    ds = device_split()
    got = ds.overlaps(kind).cpu().numpy()
    want = np.concatenate([o.reshape(-1) for o in host_overlaps(kind)])
    assert got.dtype == np.float64 and same(got, want)
    assert np.count_nonzero(want) > 100


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_helper_stages(kind, cls):
    """pass-1 scores, thresholds and pr of every (difficulty, level) group against the host entries"""
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    ds = device_split()
    levels = LEVELS[:, kind, cls]
    aos = kind == 0
    host = ap_split.host_stages(KE, gt, dt, cls, kind, levels, DIFFS, host_overlaps(kind), compute_aos=aos)
    flags = ds.flags(cls, "kitti", DIFFS, "new")
    lev = ds._up(np.ascontiguousarray(levels))
    ov = ds.overlaps(kind)
    scores, valid = ds.scores(flags, ov, kind, lev)
    ordered, count, thr, n_thr = ds.thresholds(scores, valid, flags[2])
    pr = ds.pr(flags, ov, kind, lev, thr, n_thr, aos).cpu().numpy()
    ordered, count, thr, n_thr = (t.cpu().numpy() for t in (ordered, count, thr, n_thr))
    scores, valid = scores.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(np.isfinite(scores), valid == 1)
    seen = set()
    for (l, k), h in host.items():
        g = l * len(levels) + k
        assert count[g] == len(h["scores"]) and np.array_equal(ordered[g, :count[g]], h["scores"]), (l, k)
        assert n_thr[g] == len(h["thresholds"]) and np.array_equal(thr[g, :n_thr[g]], h["thresholds"]), (l, k)
        assert np.array_equal(pr[g, :n_thr[g]], h["pr"]), (l, k, pr[g, :n_thr[g]] - h["pr"])
        assert not pr[g, n_thr[g]:].any()
        seen.add(int(n_thr[g]))
    if cls == 2:
        assert 41 in seen and 0 in seen


def _text(fn, *args, **kw):
    out = fn(*args, **kw)
    return out if isinstance(out, str) else out[0]


def test_helper_texts():
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    for kw in ({"metric": "new"}, {"metric": "old", "dataset": "waymo"}):
        want = _text(KE.get_official_eval_result, gt, dt, [0, 1, 2], **kw)
        assert _text(KE.get_official_eval_result, gt, dt, [0, 1, 2], stats_device="cuda", **kw) == want
        assert "aos" in want
    assert KE.get_coco_eval_result(gt, dt, [0, 1, 2], stats_device="cuda") == KE.get_coco_eval_result(gt, dt, [0, 1, 2])
    assert KE.get_coco_eval_result(gt, dt, [1], metric="old", dataset="waymo", stats_device="cuda") == \
        KE.get_coco_eval_result(gt, dt, [1], metric="old", dataset="waymo")


def test_helper_dense_sample_in_chunks(monkeypatch):
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    want = _text(KE.get_official_eval_result, gt, dt, 0, dense_sample=True)
    assert _text(KE.get_official_eval_result, gt, dt, 0, dense_sample=True, stats_device="cuda") == want
    monkeypatch.setattr(KE.DeviceStats, "CHUNK_BYTES", 1 << 20)                  # several chunks of overlap levels
    ds = KE.DeviceStats(KE.SplitTable(gt, dt))
    assert 1 < ds.level_chunk(6, 103) < 103
    assert _text(KE.get_official_eval_result, gt, dt, 0, dense_sample=True, stats_device="cuda") == want


def test_same_bits_twice_and_on_a_side_stream():
    import torch
    KE = pkg("kitti_eval")
    gt, dt = helper_split()
    run = lambda: KE.eval_class(gt, dt, [0, 1, 2], "kitti", DIFFS, 0, LEVELS, compute_aos=True, stats_device="cuda")
    a, b = run(), run()
    junk = [torch.randn(1000 + 37 * i, device="cuda") for i in range(20)]       # unrelated allocations shift every address
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run()
    side.synchronize()
    del junk
    for key in ("precision", "recall", "orientation"):
        assert same(a[key], b[key]) and same(a[key], c[key]), key
    assert np.count_nonzero(a["orientation"]) > 0


def test_evaluate_detections_and_prepared_gt(oracle):
    from test_kitti_eval import synthetic_perfect_table
    KE, R = pkg("kitti_eval"), pkg("results")
    E, src, table, counts = synthetic_perfect_table(16, drop_every=3)
    want_text, want = E.evaluate_detections(table, counts, src)
    text, ret = E.evaluate_detections(table, counts, src, stats_device="cuda")
    assert text == want_text and all(np.array_equal(ret[k], want[k]) for k in want if k != "result")
    prepared = R.prepare_gt(src, sorted(src.ids))
    for stats_device in ("cuda", "cpu"):
        text, _ = E.evaluate_detections(table, counts, src, stats_device=stats_device, prepared_gt=prepared)
        assert text == want_text
    with pytest.raises(ValueError, match="prepared_gt"):
        E.evaluate_detections(table, counts, src, prepared_gt=R.prepare_gt(src, sorted(src.ids)[:-1]))


def test_command_line_stats_device(tmp_path):
    KE = pkg("kitti_eval")
    gl, dl = ap_split.make_split(0)
    ids = list(range(12)) + [ap_split.IMAGES["n_dt_129"], ap_split.IMAGES["cyclists_0"]]
    for sub, lines in (("label_2", gl), ("pred", dl)):
        os.makedirs(tmp_path / sub)
        for i in ids:
            (tmp_path / sub / ("%06d.txt" % i)).write_text("\n".join(lines[i]))
    (tmp_path / "val.txt").write_text("".join("%d\n" % i for i in ids))
    argv = ["--result_path", str(tmp_path / "pred"), "--label_split_file", str(tmp_path / "val.txt"), "--label_path", str(tmp_path / "label_2")]
    texts = []
    for extra in ([], ["--stats_device", "cuda"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            KE.main(argv + extra)
        texts.append(buf.getvalue())
    assert texts[0] == texts[1] and texts[0].startswith("Car AP@0.70, 0.70, 0.70:")
