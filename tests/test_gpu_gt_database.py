"""GT-database point extraction on the device (csrc/gt_database.hip) against the package's cpu path: counts, point order and the bits of
coordinates and intensities are equal, nothing less.  The g18 test compares with the REFERENCE tool's recorded output
(tests/golden, never the reference itself)."""
import importlib

import numpy as np
import pytest

import gt_tree
import helpers
from test_gt_database import G, check_against_g18, check_crafted, same_bits

pytestmark = pytest.mark.gpu
synth = importlib.import_module("3d_adapt_auto_driving_amd.synth")
kitti_io = importlib.import_module("3d_adapt_auto_driving_amd.kitti_io")


def calib_of(rng):
    cal = helpers.fake_kitti_calib(rng)
    return {"P2": cal["P2"], "R0": cal["R0_rect"], "Tr_velo2cam": cal["Tr_velo_to_cam"]}


def to_velo(rect, cal, rng):
    """rect-frame points -> a velodyne cloud (n, 4) f32 that the calibration maps (nearly) back onto them"""
    Rv, tv = cal["Tr_velo2cam"][:, :3], cal["Tr_velo2cam"][:, 3]
    velo = (rect.astype(np.float64) @ cal["R0"] - tv) @ Rv
    return np.concatenate([velo, rng.random((len(velo), 1))], 1).astype(np.float32)


def boxes_on(rng, rect, g, spread=0.0):
    """g boxes centred on points of the cloud (all near ONE point when ``spread`` > 0: they overlap and share most points)"""
    b = helpers.boxes3d(rng, g)
    if len(rect):
        at = rect[rng.integers(0, len(rect), g)] if spread == 0.0 else rect[rng.integers(0, len(rect))] + rng.uniform(-spread, spread, (g, 3))
        b[:, 0], b[:, 2] = at[:, 0], at[:, 2]
        b[:, 1] = at[:, 1] + b[:, 3] / 2
    return b.astype(np.float32)


def cloud(rng, n):
    return np.stack([rng.uniform(-20, 20, n), rng.uniform(-1, 2.5, n), rng.uniform(3, 60, n)], 1)


def scene_of(rng, n, g, spread=0.0):
    cal = calib_of(rng)
    rect = cloud(rng, n)
    return to_velo(rect, cal, rng), cal, boxes_on(rng, rect, g, spread)


def assert_same(got, want):
    assert len(got) == len(want)
    for s, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), s
        for k, ((p, i), (wp, wi)) in enumerate(zip(a, b)):
            assert p.shape == wp.shape and i.shape == wi.shape, (s, k, p.shape, wp.shape)
            assert same_bits(p, wp) and same_bits(i, wi), (s, k)


def check(scenes, min_points=1):
    want = G.extract_objects(scenes, device="cpu")
    got = G.extract_objects(scenes, device="cuda")
    assert_same(got, want)
    assert sum(len(p) for a in want for p, _ in a) >= min_points       # the case is not vacuous
    return want


@pytest.mark.parametrize("class_name", ("Car", "People"))
def test_g18_tree_on_the_device(tmp_path, class_name):
    root, save_dir = str(tmp_path / "tree"), str(tmp_path / "db")
    gt_tree.write_gt_tree(root)
    lines = []
    db = G.generate_gt_database(root, class_name=class_name, save_dir=save_dir, device="cuda", batch_size=3, log=lines.append)
    meta = check_against_g18(db, lines, class_name, save_dir)
    check_against_g18(G.load_gt_database(G.database_file_name(save_dir, "train", class_name)), lines, class_name, save_dir)
    assert meta["file"] in G.database_file_name(save_dir, "train", class_name)


def test_tile_boundaries():
    rng = np.random.default_rng(1801)
    scenes = [scene_of(rng, n, 3, spread=1.0) for n in (1, 63, 64, 65, 4097)]
    want = check(scenes)
    assert all(len(a) == 3 for a in want)
    # the one-point scene: its point is inside a box built on it
    pts, cal, _ = scenes[0]
    rect = kitti_io.Calibration(cal).lidar_to_rect(pts[:, :3])
    box = np.array([[rect[0, 0], rect[0, 1] + 0.75, rect[0, 2], 1.5, 1.6, 4.0, 0.4]], dtype=np.float32)
    assert len(check([(pts, cal, box)])[0][0][0]) == 1


def test_scan_carry_past_256_tiles():
    """16385 points are 257 tiles (the scan's second round holds one tile), 2 * 16384 + 65 points three rounds with a ragged last
    tile.  The boxes stand on points of the first, the 257th and the last tile; the cloud is unordered, so every box also holds points
    of tiles in between, and its rows from the later rounds land behind a non-zero carry."""
    rng = np.random.default_rng(1805)
    scenes = []
    for n in (16385, 2 * 16384 + 65):
        cal, rect = calib_of(rng), cloud(rng, n)
        b = helpers.boxes3d(rng, 3)
        at = rect[[5, 256 * 64, n - 1]]
        b[:, 0], b[:, 1], b[:, 2] = at[:, 0], at[:, 1] + b[:, 3] / 2, at[:, 2]
        scenes.append((to_velo(rect, cal, rng), cal, b.astype(np.float32)))
    want = check(scenes, min_points=6)
    for (pts, cal, _), objs in zip(scenes, want):
        rect = kitti_io.Calibration(cal).lidar_to_rect(pts[:, :3])
        idx = [[int(np.flatnonzero((rect == row).all(1))[0]) for row in p] for p, _ in objs]       # the objects' points in the cloud
        assert all(i == sorted(i) for i in idx) and 5 in idx[0] and 256 * 64 in idx[1] and len(pts) - 1 in idx[2]
        assert all(i[0] < 16384 <= i[-1] for i in idx[1:]), idx                  # rows of the first round and rows behind it


def test_box_chunk_boundaries():
    C = G.box_chunk()
    rng = np.random.default_rng(1802)
    scenes = [scene_of(rng, 700 + 13 * i, g, spread=0.8) for i, g in enumerate((C - 1, C, C + 1, 2 * C + 1))]
    want = check(scenes, min_points=4 * C)
    nonempty = [sum(len(p) > 0 for p, _ in a) for a in want]
    assert nonempty[3] > C + 1                                          # boxes of every chunk hold points


def test_ragged_batches():
    rng = np.random.default_rng(1803)
    none = lambda n: scene_of(rng, n, 0)
    far = scene_of(rng, 500, 4)
    far[2][:, 2] += 500.0                                               # boxes that contain no point
    check([none(300), scene_of(rng, 1000, 5), none(64), scene_of(rng, 129, 2), far, none(10)])
    got = G.extract_objects([far], device="cuda")
    assert [p.shape for p, _ in got[0]] == [(0, 3)] * 4 and [i.shape for _, i in got[0]] == [(0,)] * 4
    check([scene_of(rng, 2000, 7)])                                     # a batch of one scene
    assert G.extract_objects([none(100)], device="cuda") == [[]]
    assert G.extract_objects([], device="cuda") == []
    empty_cloud = (np.zeros((0, 4), np.float32), calib_of(rng), helpers.boxes3d(rng, 2))
    check([empty_cloud, scene_of(rng, 100, 2)])


def test_crafted_faces_and_the_10m_rule_on_the_device():
    check_crafted("cuda")


@pytest.mark.parametrize("seed", (1811, 1812, 1813))
def test_lidar_shaped_scenes(seed):
    rng = np.random.default_rng(seed)
    scenes = []
    for k, (n, g) in enumerate(((16384, 40), (9000, 11), (12345, 25))):
        rect, cars = synth.lidar_scene_with_labels(seed * 10 + k, n, min(g, 14))
        rect = rect[:, :3].astype(np.float64)
        boxes = np.concatenate([cars.reshape(-1, 7).astype(np.float32), boxes_on(rng, rect, g - len(cars))])
        boxes[:, 6] = rng.uniform(-2 * np.pi, 2 * np.pi, len(boxes)).astype(np.float32)          # arbitrary headings
        boxes[::5, 5] = rng.uniform(15, 30, len(boxes[::5]))                                     # long boxes: the 10 m rule decides
        cal = calib_of(rng)
        scenes.append((to_velo(rect, cal, rng), cal, boxes))
    check(scenes, min_points=1000)


def test_used_handle_equals_fresh():
    rng = np.random.default_rng(1804)
    big = [scene_of(rng, 5000, 70, spread=2.0), scene_of(rng, 3000, 9)]
    small = [scene_of(rng, 257, 3, spread=1.0), scene_of(rng, 64, 1, spread=0.5), scene_of(rng, 900, 6)]
    used = G.GtExtractor("cuda")
    first = used(big)
    second = used(small)                                                # the count buffer still holds the larger batch's
    assert_same(second, G.GtExtractor("cuda")(small))
    assert_same(second, G.extract_objects(small, device="cpu"))
    assert_same(used(big), first)
