"""car_split.py on the host path against the reference's own run (tests/golden g26 over tests/car_tree.py): byte for byte."""
import json
import os

import pytest

from conftest import pkg
import car_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_few_shot_ref.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def CS():
    return pkg("car_split")


def test_cpu_path_writes_the_references_files(tmp_path, capsys):
    a, b = car_tree.write_roots(tmp_path)
    CS().main([a, b, "--parse_device", "cpu"])
    got = car_tree.car1_texts((a, b))
    assert got == golden()["car1"]
    assert not any(t.endswith("\n") for t in got.values())
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 4 and lines[0] == "%s train: 9 listed, 7 kept, 0 host-decided files" % a
    CS().main([a, b])                                                    # cpu is the default; an existing file is overwritten, equal
    assert car_tree.car1_texts((a, b)) == got


def test_the_stream_runs_on_across_roots(tmp_path):
    a, b = car_tree.write_roots(tmp_path)
    CS().car_split([b, a], log=lambda *x: None)
    got, want = car_tree.car1_texts((a, b)), golden()["car1"]
    assert got != want and {k: sorted(v.split("\n")) for k, v in got.items()} == {k: sorted(v.split("\n")) for k, v in want.items()}
    CS().car_split([b], log=lambda *x: None)
    assert car_tree.car1_texts((b,), ("B",))["B/train_car1.txt"] != want["B/train_car1.txt"]


def test_pointrcnn_layout_on_a_linked_copy(tmp_path):
    a, b = car_tree.write_roots(tmp_path / "src")
    linked = [str(tmp_path / "linked" / name) for name in ("A", "B")]
    for src, dst in zip((a, b), linked):
        pkg("multi_data").gen_data(src, dst)
    written = CS().car_split(linked, layout="pointrcnn", log=lambda *x: None)
    assert sorted(written) == sorted(os.path.join(d, "KITTI", "ImageSets", s + "_car1.txt") for d in linked for s in car_tree.SPLITS)
    assert car_tree.car1_texts((a, b)) == golden()["car1"]               # through the ImageSets link: the same files
    assert list(written.values()) == [golden()["car1"]["%s/%s_car1.txt" % (r, s)] for r in "AB" for s in car_tree.SPLITS]


def test_is_valid_car_to_the_letter():
    ok = CS().is_valid_car
    assert ok(car_tree.CAR.split(" ")) and not ok(car_tree.VAN.split(" ")) and not ok(["car"]) and not ok(["Cars"]) and not ok([""])
    assert ok(car_tree.line("Car", y1="100.00", y2="124.00").split(" ")) and not ok(car_tree.line("Car", y1="100.00", y2="123.99").split(" "))
    assert ok(car_tree.line("Car", occluded="2.0").split(" ")) and not ok(car_tree.line("Car", occluded="2.5").split(" "))
    assert ok(car_tree.line("Car", truncated="5e-1").split(" ")) and not ok(car_tree.line("Car", truncated="nan").split(" "))


@pytest.mark.parametrize("bad", ["Car 0.00 0 1.57 300.00 100.00 380.00", car_tree.line("Car", truncated="0.x0")])
def test_a_line_the_reference_raises_on_raises_before_any_file_is_written(tmp_path, bad):
    a, b = car_tree.write_roots(tmp_path)
    victim = os.path.join(b, "training", "label_2", "000033.txt")        # B's val split: the last list of the run
    with open(victim, "a") as f:
        f.write(bad + "\n")
    with pytest.raises(ValueError, match="000033.txt"):
        CS().main([a, b, "--parse_device", "cpu"])
    assert not [n for r in (a, b) for n in os.listdir(r) if n.endswith("_car1.txt")]


def test_cuda_without_a_device_raises_by_name(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a, b = car_tree.write_roots(tmp_path)
    with pytest.raises(pkg("kitti_annos").ParseDeviceError):
        CS().main([a, b, "--parse_device", "cuda"])
    assert not [n for r in (a, b) for n in os.listdir(r) if n.endswith("_car1.txt")]


def test_column_rule_over_the_python_checker_of_the_device_grammar(tmp_path, monkeypatch):
    """The whole-array rule and the hand-over of the files outside the grammar, with the parser's Python restatement (device "cpu" of
    parse_texts) standing in for the kernels: the same kept lists as line by line."""
    KA = pkg("kitti_annos")
    real, calls = KA.parse_texts, []

    def on_cpu(texts, device, **kw):
        calls.append(len(texts))
        return real(texts, "cpu", **kw)
    monkeypatch.setattr(KA, "parse_texts", on_cpu)
    a, b = car_tree.write_roots(tmp_path)
    for path, root in ((a, "A"), (b, "B")):
        for split in car_tree.SPLITS:
            names, kept, host = CS().kept_names(path, split, parse_device="cuda")
            assert names == car_tree.listed(root, split) and kept == car_tree.with_car(root, split)
            assert kept == CS().kept_names(path, split, parse_device="cpu")[1]
            assert host == len(car_tree.HOST_DECIDED[root][split])
    assert calls == [9, 7, 9, 5]                                         # one call per root and split
