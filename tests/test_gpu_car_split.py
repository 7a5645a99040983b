"""car_split.py with --parse_device cuda (csrc/kitti_parse.hip through kitti_annos.parse_texts) against the reference's run (tests/golden
g26) and the line-by-line path: byte for byte."""
import json
import os

import pytest

from conftest import pkg
import car_tree

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_few_shot_ref.json")


def test_device_path_writes_the_references_files(tmp_path, monkeypatch):
    KA, CS = pkg("kitti_annos"), pkg("car_split")
    with open(GOLDEN) as f:
        want = json.load(f)["car1"]
    real, calls = KA.parse_texts, []

    def counted(texts, device, **kw):
        side = real(texts, device, **kw)
        calls.append((device, len(texts), sorted(side._host_annos), side.parse_stats["host_files"]))
        return side
    monkeypatch.setattr(KA, "parse_texts", counted)
    a, b = car_tree.write_roots(tmp_path / "cuda")
    lines = []
    CS.car_split([a, b], parse_device="cuda", log=lines.append)
    got = car_tree.car1_texts((a, b))
    assert got == want                                                          # the reference's bytes
    order = [(root, split) for root in "AB" for split in car_tree.SPLITS]
    assert len(calls) == 4                                                      # one call per root and split, not per file
    for (device, n, host, n_host), (root, split) in zip(calls, order):
        ids = car_tree.listed(root, split)
        assert device == "cuda" and n == len(ids)
        assert [ids[f] for f in host] == sorted(car_tree.HOST_DECIDED[root][split], key=ids.index) and n_host == len(host)
    assert lines == ["%s %s: %d listed, %d kept, %d host-decided files" %
                     (path, split, len(car_tree.listed(root, split)), len(car_tree.with_car(root, split)), len(car_tree.HOST_DECIDED[root][split]))
                     for path, root in ((a, "A"), (b, "B")) for split in car_tree.SPLITS]
    assert sum(len(car_tree.HOST_DECIDED[r][s]) for r, s in order if r == "A") == 2 == sum(len(car_tree.HOST_DECIDED[r][s]) for r, s in order if r == "B")

    monkeypatch.setattr(KA, "parse_texts", real)
    c, d = car_tree.write_roots(tmp_path / "cpu")
    CS.main([c, d, "--parse_device", "cpu"])
    assert car_tree.car1_texts((c, d)) == got                                   # the line-by-line path's bytes


def test_device_path_raises_where_the_reference_raises(tmp_path):
    a, b = car_tree.write_roots(tmp_path)
    with open(os.path.join(b, "training", "label_2", "000033.txt"), "a") as f:
        f.write("Car 0.00 0 1.57 300.00 100.00 380.00\n")                       # 7 tokens: outside the grammar, then the restatement raises
    with pytest.raises(ValueError, match="000033.txt"):
        pkg("car_split").main([a, b, "--parse_device", "cuda"])
    assert not [n for r in (a, b) for n in os.listdir(r) if n.endswith("_car1.txt")]
