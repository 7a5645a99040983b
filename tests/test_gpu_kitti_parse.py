"""The label / result text parser on the device (csrc/kitti_parse.hip through kitti_annos.parse_texts(device="cuda")) against its
Python checker (device="cpu") and the definition, the host parser: bit for bit on every column, no tolerance -- a regular token's
value is ONE correctly rounded f64 multiplication or division of two exact operands, which is what these tests confirm of the
device's arithmetic."""
import contextlib
import io
import os

import numpy as np
import pytest

from conftest import pkg
import ap_split
import kitti_parse_cases as cases

pytestmark = pytest.mark.gpu


def KA():
    return pkg("kitti_annos")


def three_ways(texts, skip_blank=False, what=""):
    dev = KA().parse_texts(texts, "cuda", skip_blank=skip_blank)
    cpu = KA().parse_texts(texts, "cpu", skip_blank=skip_blank)
    cases.assert_same_side(dev, cpu, what)
    cases.assert_same_side(dev, cases.host_side(KA(), texts, skip_blank), what)
    assert dev.parse_stats == dict(cpu.parse_stats, device="cuda")
    return dev


@pytest.mark.parametrize("name", sorted(cases.regular_sides()))
def test_regular_sides(name):
    texts = cases.regular_sides()[name]
    dev = three_ways(texts, what=name)
    assert dev.parse_stats["host_files"] == 0
    cases.assert_same_annos(dev.annos, [KA()._host_anno(t, False) for t in texts], name)


def test_every_sweep_token_is_pythons_float():
    toks = cases.sweep_tokens()
    side = KA().parse_texts(cases.regular_sides()["sweep"], "cuda")
    assert side.parse_stats["host_files"] == 0 and len(side) * cases.FLOAT_SLOTS == len(toks) >= 2000
    table = np.concatenate([side.truncated[:, None], side.alpha[:, None], side.bbox, side.dimensions[:, [1, 2, 0]], side.location,
                            side.rotation_y[:, None], side.score[:, None]], axis=1)
    want = np.array([float(t) for t in toks])
    wrong = np.flatnonzero(table.reshape(-1).view(np.int64) != want.view(np.int64))
    assert wrong.size == 0, [(toks[i], table.reshape(-1)[i].hex(), want[i].hex()) for i in wrong[:8]]


@pytest.mark.parametrize("name", sorted(cases.boundary_sides()))
def test_boundary_shapes(name):
    texts, skip_blank = cases.boundary_sides()[name]
    dev = three_ways(texts, skip_blank, name)
    assert dev.parse_stats["host_files"] == 0


def test_lines_mode():
    for lines in cases.g10_lines() + ap_split.make_split(0):
        three_ways([cases.text_of(l, False) for l in lines], True)
    dev = three_ways(cases.BLANKS_DROPPED, True)
    assert dev.off.tolist() == [0, 2, 2, 2, 4] and dev.parse_stats["host_files"] == 0


def test_regular_and_irregular_files_interleaved():
    """order is kept and parse_stats counts the files sent back; a file the host parser rejects raises its exception"""
    parsable, rejected = [], []
    for name in sorted(cases.IRREGULAR):
        text, skip_blank = cases.IRREGULAR[name]
        if not skip_blank:
            try:
                KA()._host_anno(text, False)
                parsable.append(text)
            except (ValueError, IndexError):
                rejected.append(text)
    assert len(parsable) >= 10 and len(rejected) >= 10
    regular = cases.regular_sides()["split_dt"]
    texts = []
    for i, text in enumerate(parsable):
        texts += [regular[i % len(regular)], text] + ([""] if i % 3 == 0 else [])
    dev = three_ways(texts)
    assert dev.parse_stats["host_files"] == len(parsable) and dev.parse_stats["files"] == len(texts)
    cases.assert_same_annos(dev.annos, [KA()._host_anno(t, False) for t in texts])
    for text in rejected:
        with pytest.raises((ValueError, IndexError)) as want:
            KA()._host_anno(text, False)
        with pytest.raises(type(want.value)) as got:
            KA().parse_texts([regular[3], text, regular[4]], "cuda")
        assert str(got.value) == str(want.value)
    for name in ("skip_blank_but_nan", "skip_blank_but_14"):
        text = cases.IRREGULAR[name][0]
        try:
            want = cases.host_side(KA(), [regular[0], text], True)
        except IndexError:
            with pytest.raises(IndexError):
                KA().parse_texts([regular[0], text], "cuda", skip_blank=True)
        else:
            dev = KA().parse_texts([regular[0], text], "cuda", skip_blank=True)
            cases.assert_same_side(dev, want)
            assert dev.parse_stats["host_files"] == 1


def test_two_calls_and_a_side_stream_give_the_same_bytes():
    import torch
    texts = cases.regular_sides()["split_dt"] + cases.boundary_sides()["chunk_edges"][0]
    a = KA().parse_texts(texts, "cuda")
    junk = torch.full((1 << 22,), 0xff, dtype=torch.uint8, device="cuda")            # what the allocator hands out next is not zero
    del junk
    b = KA().parse_texts(texts, "cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c = KA().parse_texts(texts, "cuda")
    stream.synchronize()
    cases.assert_same_side(a, b)
    cases.assert_same_side(a, c)
    assert a._name_span.tobytes() == b._name_span.tobytes() == c._name_span.tobytes()


def test_several_calls_per_side(monkeypatch):
    texts = cases.regular_sides()["split_dt"]
    want = KA().parse_texts(texts, "cuda")
    monkeypatch.setattr(KA(), "PARSE_MAX_BYTES", 20000)
    side = KA().parse_texts(texts, "cuda")
    assert side.parse_stats["calls"] > 2 and side.parse_stats["host_files"] == 1
    cases.assert_same_side(side, want)
    cases.assert_same_annos(side.annos, want.annos)


def test_g10_end_to_end_on_the_device(oracle):
    KE = pkg("kitti_eval")
    z = np.load(cases.G10)
    gt = KE.parse_texts([str(s) for s in z["gt_lines"]], "cuda")
    dt = KE.parse_texts([str(s) for s in z["dt_lines"]], "cuda")
    assert gt.parse_stats["host_files"] == 0 == dt.parse_stats["host_files"]
    text, _ = KE.get_official_eval_result(gt, dt, 0, "kitti", stats_device="cuda")
    assert text == str(z["result_text"])                                 # character for character
    assert KE.get_official_eval_result(KE.PreparedGT(gt), dt, 0, "kitti", stats_device="cuda")[0] == text
    assert KE.get_official_eval_result(gt, dt, 0, "kitti")[0] == text    # the host statistics read the dicts built from the columns
    texts = [str(s) for s in z["gt_lines"]], [str(s) for s in z["dt_lines"]]
    assert KE.get_official_eval_result(*texts, 0, "kitti", stats_device="cuda", parse_device="cuda")[0] == text
    assert KE.get_coco_eval_result(*texts, 0, stats_device="cuda", parse_device="cuda") == KE.get_coco_eval_result(gt.annos, dt.annos, 0)


def test_evaluate_detections_parse_device(oracle):
    from test_kitti_eval import synthetic_perfect_table
    R = pkg("results")
    E, src, table, counts = synthetic_perfect_table(16, drop_every=3)
    want, _ = E.evaluate_detections(table, counts, src)
    for stats_device in ("cpu", "cuda"):
        assert E.evaluate_detections(table, counts, src, stats_device=stats_device, parse_device="cuda")[0] == want
    prepared = R.prepare_gt(src, sorted(src.ids), parse_device="cuda")
    assert E.evaluate_detections(table, counts, src, stats_device="cuda", prepared_gt=prepared, parse_device="cuda")[0] == want


def test_command_line_parse_device(tmp_path):
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
    for extra in ([], ["--parse_device", "cuda"], ["--parse_device", "cuda", "--stats_device", "cuda"], ["--parse_device", "cpu"]):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            KE.main(argv + extra)
        texts.append(buf.getvalue())
    assert texts[0] == texts[1] == texts[2] == texts[3] and texts[0].startswith("Car AP@0.70, 0.70, 0.70:")
