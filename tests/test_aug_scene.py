"""Augmented-scene generation (3d_adapt_auto_driving_amd/aug_scene.py), host side: the cpu path against the REFERENCE tool's own output
on tests/aug_tree.py's tree (tests/golden g19, tests/golden/make_golden_aug_scene.py), the host replay of the random stream against
the try-by-try run, the scene without a label, the command line."""
import importlib
import json
import os

import numpy as np
import pytest

import aug_tree

PKG = "3d_adapt_auto_driving_amd"
A = importlib.import_module(PKG + ".aug_scene")
G = importlib.import_module(PKG + ".gt_database")
kitti_io = importlib.import_module(PKG + ".kitti_io")
HERE = os.path.dirname(os.path.abspath(__file__))
G19 = os.path.join(HERE, "golden", "g19_aug_scene_ref")
RUNS = (("Car", 2), ("People", 1))
quiet = lambda s: None


def g19():
    with open(G19 + ".json") as f:
        return json.load(f), np.load(G19 + ".npz")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("aug_tree"))
    aug_tree.write_aug_tree(root)
    return root


@pytest.fixture(scope="module")
def databases(tree, tmp_path_factory, oracle):
    """class name -> (pickle path, list), made by this package's cpu path and checked against the recorded point counts"""
    meta, _ = g19()
    out = {}
    for class_name, _ in RUNS:
        db_dir = str(tmp_path_factory.mktemp("db_" + class_name))
        db = G.generate_gt_database(tree, class_name=class_name, save_dir=db_dir, device="cpu", log=quiet)
        assert [len(e["points"]) for e in db] == meta[class_name]["db_points"]
        assert os.path.basename(G.database_file_name(db_dir, "train", class_name)) == meta[class_name]["db_file"]
        out[class_name] = (G.database_file_name(db_dir, "train", class_name), db)
    return out


def check_against_g19(class_name, root, db_path, save_dir, lines):
    """bins byte for byte, labels, split file and log character for character, the printed lines"""
    meta, z = g19()
    m = meta[class_name]
    fix = lambda s: s.replace(save_dir, "<save_dir>").replace(os.path.dirname(db_path), "<db_dir>").replace(
        os.path.join(root, "KITTI/ImageSets/"), "../data/KITTI/ImageSets/")       # the reference's hard-coded copy target
    assert sorted(os.listdir(os.path.join(save_dir, "rectified_data"))) == m["bins"]
    for name in m["bins"]:
        with open(os.path.join(save_dir, "rectified_data", name), "rb") as f:
            assert f.read() == z["%s_%s" % (class_name, name[:-4])].tobytes(), (class_name, name)
    assert sorted(os.listdir(os.path.join(save_dir, "aug_label"))) == sorted(m["labels"])
    for name, text in m["labels"].items():
        with open(os.path.join(save_dir, "aug_label", name)) as f:
            assert f.read() == text, (class_name, name)
    with open(os.path.join(save_dir, "train_aug.txt")) as f:
        split = f.read()
    assert split == m["split"] and not split.endswith("\n")
    with open(os.path.join(root, "KITTI", "ImageSets", "train_aug.txt")) as f:
        assert f.read() == split
    with open(os.path.join(save_dir, "log_info.txt")) as f:
        assert fix(f.read()) == m["log"]
    assert [fix(x) for x in lines] == m["stdout"]
    return m


@pytest.mark.parametrize("class_name,aug_times", RUNS)
def test_cpu_path_equals_reference_tool(tree, databases, tmp_path, class_name, aug_times):
    save_dir, lines = str(tmp_path / "aug"), []
    got = A.generate_aug_scene(tree, databases[class_name][0], save_dir, class_name=class_name, aug_times=aug_times, device="cpu",
                               log=lines.append)
    m = check_against_g19(class_name, tree, databases[class_name][0], save_dir, lines)
    assert got == m["split"].split("\n")


def test_fixture_covers_the_cases():
    """What the tree was built to provoke is in the reference's run (the generator asserts it; the counts are recorded)."""
    meta, z = g19()
    assert int(meta["numpy"].split(".")[0]) >= 2                                 # NEP 50: the f64 y shift of the pasted points
    car, people = meta["Car"]["cases"], meta["People"]["cases"]
    for key in ("accepted", "rejected_original", "rejected_enlargement_only", "range_skip", "few_points_skip", "break",
                "original_points_removed"):
        assert car[key] + people[key] > 0, key
    assert people["scenes_skipped"] == 1 and len(meta["People"]["bins"]) == 5 and "400030" not in meta["People"]["split"]
    assert meta["label_dropped_by_80_percent_rule"] is True and car["labels_dropped_by_80_percent_rule"] > 0
    assert meta["Car"]["split"].split("\n")[:6] == ["%06d" % i for i in aug_tree.SAMPLE_IDS]
    assert meta["Car"]["split"].split("\n")[6] == "400002" and meta["Car"]["split"].split("\n")[-1] == "800030"
    assert any(line.startswith("People ") for text in meta["People"]["labels"].values() for line in text.splitlines())


def scene_inputs(tree, sample_id):
    base = os.path.join(tree, "KITTI", "object", "training")
    pts = np.fromfile(os.path.join(base, "velodyne", "%06d.bin" % sample_id), dtype=np.float32).reshape(-1, 4)
    calib = kitti_io.Calibration(os.path.join(base, "calib", "%06d.txt" % sample_id))
    plane = A.road_plane(os.path.join(base, "planes", "%06d.txt" % sample_id))
    return pts, calib, aug_tree.IMG_SHAPE, plane


@pytest.mark.parametrize("class_name", ("Car", "People"))
def test_replay_equals_try_by_try(tree, databases, class_name):
    """The stream replayed before any geometry gives the candidates, and leaves the generator in the state, of the loop that tests
    every candidate as it is drawn."""
    db = databases[class_name][1]
    scope = A.area_scope(class_name)
    meta, _ = g19()
    boxes = np.array([[0.0, 1.7, 30.0, 1.5, 1.6, 4.0, 0.3], [-9.0, 1.7, 14.0, 1.5, 1.6, 4.0, -1.0]], dtype=np.float32)
    a, b = A.new_rng(), A.new_rng()
    draws = 0
    for sample_id in aug_tree.SAMPLE_IDS[:3] * 2:
        pts, calib, shape, plane = scene_inputs(tree, sample_id)
        rect, inten = A.valid_points(pts, calib, shape, scope)
        st = A.aug_one_scene_cpu(a, sample_id, rect, inten, boxes, plane, db, scope)
        stats = {}
        cand = A.replay_candidates(b, db, scope, stats)
        assert cand == st.tested and 10 < len(cand) <= 15 and len(db) - 1 not in cand
        assert 0 < len(st.accepted) <= len(cand)
        draws += sum(stats.values())
        sa, sb = a.get_state(), b.get_state()
        assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    # the stream is np.random.seed(1024)'s: the first scenes' draw counts are the recorded run's
    if class_name == "Car":
        np.random.seed(1024)
        c = np.random.RandomState(1024)
        assert np.random.randint(10, 15) == c.randint(10, 15) and np.random.randint(0, 26) == c.randint(0, 26)


def test_all_candidates_out_of_range(tree, databases):
    """Every entry's centre outside the scope: 50 draws, no candidate, the scene's valid points come back unchanged."""
    db = [dict(e, gt_box3d=e["gt_box3d"] + np.array([0, 0, 100, 0, 0, 0, 0], np.float32)) for e in databases["Car"][1]]
    scope = A.area_scope("Car")
    pts, calib, shape, plane = scene_inputs(tree, 7)
    rect, inten = A.valid_points(pts, calib, shape, scope)
    assert 0 < len(rect) < len(pts)
    rng, twin = A.new_rng(), A.new_rng()
    st = A.aug_one_scene_cpu(rng, 7, rect, inten, np.zeros((0, 7), np.float32), plane, db, scope)       # not even a label is needed
    assert st.tested == [] and st.accepted == []
    rows = st.rows(db)
    assert rows.dtype == np.float32 and np.array_equal(rows[:, :3], rect) and np.array_equal(rows[:, 3], inten)
    stats = {}
    assert A.replay_candidates(twin, db, scope, stats) == [] and stats == {"range": 50}
    twin2 = A.new_rng()
    twin2.randint(10, 15)
    for _ in range(50):
        twin2.randint(0, len(db) - 1)
    assert np.array_equal(rng.get_state()[1], twin2.get_state()[1]) and rng.get_state()[2] == twin2.get_state()[2]


def test_scene_without_a_label_raises(tree, databases, tmp_path):
    db_path, db = databases["Car"]
    pts, calib, shape, plane = scene_inputs(tree, 11)
    none = np.zeros((0, 7), np.float32)
    with pytest.raises(ValueError, match="sample 000011 has no label besides DontCare"):
        A.aug_one_scene_cpu(A.new_rng(), 11, *A.valid_points(pts, calib, shape, A.area_scope("Car")), none, plane, db, A.area_scope("Car"))
    with pytest.raises(ValueError, match="sample 000011 has no label besides DontCare"):
        A.place_candidates([(pts, calib, shape, none, plane)], [(0, [0, 1])], db, device="cpu", ids=[11])
    # through the tool: a tree whose third scene holds a DontCare line only
    import shutil
    root = str(tmp_path / "tree")
    shutil.copytree(tree, root)
    with open(os.path.join(root, "KITTI", "object", "training", "label_2", "000011.txt"), "w") as f:
        f.write("DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10\n")
    with pytest.raises(ValueError, match="sample 000011"):
        A.generate_aug_scene(root, db, str(tmp_path / "aug"), aug_times=1, device="cpu", log=quiet)
    with open(str(tmp_path / "aug" / "log_info.txt")) as f:                                        # what was written before is logged
        logged = f.read().splitlines()
    assert [x.split("/")[-1] for x in logged] == ["400002.txt", "400007.txt"] and all(x.startswith("Save to file") for x in logged)
    assert sorted(os.listdir(str(tmp_path / "aug" / "aug_label"))) == ["400002.txt", "400007.txt"]
    assert not os.path.exists(str(tmp_path / "aug" / "train_aug.txt"))
    with pytest.raises(ValueError, match="Invalid classes: Truck"):
        A.generate_aug_scene(tree, db, str(tmp_path / "aug2"), class_name="Truck", device="cpu", log=quiet)
    with pytest.raises(ValueError, match="at most 16"):
        A.place_candidates([(pts, calib, shape, np.ones((1, 7), np.float32), plane)], [(0, [0] * 17)], db, device="cpu")


def test_place_candidates_cpu_is_the_loop(tree, databases):
    """place_candidates on replayed lists = the try-by-try run (rows and accepted boxes)."""
    db = databases["Car"][1]
    scope = A.area_scope("Car")
    boxes = np.array([[0.0, 1.7, 30.0, 1.5, 1.6, 4.0, 0.3]], dtype=np.float32)
    a, b = A.new_rng(), A.new_rng()
    scenes, jobs, want = [], [], []
    for k, sample_id in enumerate(aug_tree.SAMPLE_IDS[:2]):
        pts, calib, shape, plane = scene_inputs(tree, sample_id)
        st = A.aug_one_scene_cpu(a, sample_id, *A.valid_points(pts, calib, shape, scope), boxes, plane, db, scope)
        want.append((st.rows(db), st.accepted))
        scenes.append((pts, calib, shape, boxes, plane))
        jobs.append((k, A.replay_candidates(b, db, scope)))
    got = A.place_candidates(scenes, jobs, db, device="cpu")
    for (rows, acc), (wrows, wacc) in zip(got, want):
        assert rows.tobytes() == wrows.tobytes() and [i for i, _ in acc] == [i for i, _, _ in wacc]
        assert all(np.array_equal(x[1], y[1]) for x, y in zip(acc, wacc))


def test_cli_round_trip(tree, databases, tmp_path, capsys):
    save_dir = str(tmp_path / "cli")
    A.main(["--root", tree, "--save_dir", save_dir, "--class_name", "People", "--aug_times", "1", "--device", "cpu",
            "--gt_database_dir", databases["People"][0]])
    out = capsys.readouterr().out.splitlines()
    check_against_g19("People", tree, databases["People"][0], save_dir, out)
