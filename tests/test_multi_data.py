"""multi_data.py (symbolic links from the dataset layout to the PointRCNN layout) against the reference's gen_data (tests/golden g26)."""
import json
import os
import shutil

from conftest import pkg
import car_tree

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_few_shot_ref.json")


def links_of(dst, src):
    out = []
    for base, dirs, files in os.walk(dst):
        for name in dirs + files:
            p = os.path.join(base, name)
            if os.path.islink(p):
                assert os.path.isabs(os.readlink(p))
                out.append([os.path.relpath(p, dst), os.path.relpath(os.readlink(p), src)])
    return sorted(out)


def test_links_are_the_references(tmp_path, monkeypatch):
    with open(GOLDEN) as f:
        want = json.load(f)["links"]
    a, _b = car_tree.write_roots(tmp_path / "src")
    dst = str(tmp_path / "dst")
    monkeypatch.chdir(tmp_path)
    made = pkg("multi_data").gen_data(os.path.relpath(a), dst)           # a relative SRC: the targets are absolute all the same
    assert links_of(dst, a) == want and sorted(made) == [p for p, _t in want]
    assert len(want) == 6 and os.path.isdir(os.path.join(dst, "KITTI", "object", "training")) and not os.path.islink(os.path.join(dst, "KITTI", "object", "training"))
    with open(os.path.join(dst, "KITTI", "ImageSets", "train.txt")) as f:
        assert f.read().split() == car_tree.listed("A", "train")
    assert sorted(os.listdir(os.path.join(dst, "KITTI", "object", "training", "label_2"))) == sorted(os.listdir(os.path.join(a, "training", "label_2")))


def test_a_second_call_changes_nothing(tmp_path):
    a, _b = car_tree.write_roots(tmp_path / "src")
    dst = str(tmp_path / "dst")
    pkg("multi_data").main([a, dst])
    before = links_of(dst, a)
    assert pkg("multi_data").gen_data(a, dst) == [] and links_of(dst, a) == before


def test_no_planes_no_link_and_a_later_one_is_added(tmp_path):
    a, b = car_tree.write_roots(tmp_path / "src")
    shutil.rmtree(os.path.join(a, "training", "planes"))
    dst = str(tmp_path / "dst")
    pkg("multi_data").gen_data(a, dst)
    assert "planes" not in os.listdir(os.path.join(dst, "KITTI", "object", "training"))
    os.makedirs(os.path.join(a, "training", "planes"))
    assert pkg("multi_data").gen_data(a, dst) == [os.path.join("KITTI", "object", "training", "planes")]
    dst_b = str(tmp_path / "dst_b")
    pkg("multi_data").gen_data(b, dst_b)                                 # B never had planes/ or image_2/
    assert sorted(os.listdir(os.path.join(dst_b, "KITTI", "object", "training"))) == ["calib", "label_2", "velodyne"]
