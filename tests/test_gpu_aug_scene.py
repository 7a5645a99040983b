"""Augmented-scene placement on the device (csrc/aug_scene.hip) against the package's cpu path: the accepted objects, their order, the
kept points and every bit of the rows are equal, nothing less.  The g19 tests compare with the REFERENCE tool's recorded output
(tests/golden, never the reference itself).  The crafted cases use an identity calibration (rect = velodyne, u = x / z, v = y / z) and
the level plane y = 1.7, so that a database box lands where its x, z put it."""
import importlib

import numpy as np
import pytest

import helpers
from test_aug_scene import A, G, RUNS, check_against_g19, databases, tree  # noqa: F401  (the two fixtures)

pytestmark = pytest.mark.gpu

IDENTITY = {"P2": np.eye(3, 4), "R0": np.eye(3), "Tr_velo2cam": np.eye(3, 4)}
SHAPE = (1000, 1000)
LEVEL = np.array([0.0, -1.0, 0.0, 1.7])
CAR = (1.5, 1.6, 4.0)
FAR_BOX = np.array([[38.0, 1.7, 68.0, 1.5, 1.6, 4.0, 0.0]], dtype=np.float32)          # a label that is in nobody's way


def entry(rng, x, z, ry=0.0, hwl=CAR, n=40, y=1.2):
    """A database entry: a box at (x, y, z) with n points inside it."""
    h, w, l = hwl
    loc = rng.uniform(-0.45, 0.45, (n, 3)) * [l, h, w]
    c, s = np.cos(ry), np.sin(ry)
    pts = np.stack([x + loc[:, 0] * c + loc[:, 2] * s, y - h / 2 + loc[:, 1], z - loc[:, 0] * s + loc[:, 2] * c], 1)
    return {"gt_box3d": np.array([x, y, z, h, w, l, ry], dtype=np.float32), "points": pts.astype(np.float32),
            "intensity": rng.random(n).astype(np.float32)}


def cloud(rng, n_valid, n_invalid=0, around=None):
    """(n, 4) f32: n_valid points that pass the filter (some of them around the given (x, z) places, at car height) and n_invalid
    that do not (behind the image's left edge, below the scope, beyond z = 70.4), shuffled."""
    good = np.stack([rng.uniform(1, 36, n_valid), rng.uniform(0.05, 2.6, n_valid), rng.uniform(4, 66, n_valid)], 1)
    if around is not None and n_valid:
        k = n_valid // 2
        at = np.asarray(around, dtype=np.float64)[rng.integers(0, len(around), k)]
        good[:k, 0], good[:k, 2] = at[:, 0] + rng.uniform(-2.5, 2.5, k), at[:, 1] + rng.uniform(-1.2, 1.2, k)
        good[:k, 1] = rng.uniform(0.3, 1.6, k)
    bad = np.stack([rng.uniform(-30, -1, n_invalid), rng.uniform(0.1, 2.0, n_invalid), rng.uniform(4, 66, n_invalid)], 1)
    bad[::3, 0], bad[::3, 1] = 5.0, -0.5                                                # v < 0
    bad[1::3, 0], bad[1::3, 2] = 6.0, 71.0                                              # beyond the scope (70.4 decides in f64)
    pts = np.concatenate([good, bad], 0)
    pts = pts[rng.permutation(len(pts))]
    return np.concatenate([pts, rng.random((len(pts), 1))], 1).astype(np.float32)


def scene(pts, boxes=FAR_BOX, plane=LEVEL, calib=IDENTITY):
    return pts, calib, SHAPE, np.asarray(boxes, dtype=np.float32).reshape(-1, 7), plane


def check(scenes, jobs, db, class_name="Car"):
    """device == cpu, bit for bit -> the cpu path's results"""
    want = A.place_candidates(scenes, jobs, db, class_name=class_name, device="cpu")
    got = A.place_candidates(scenes, jobs, db, class_name=class_name, device="cuda")
    assert len(got) == len(want) == len(jobs)
    for j, ((rows, acc), (wrows, wacc)) in enumerate(zip(got, want)):
        assert [i for i, _ in acc] == [i for i, _ in wacc], (j, acc, wacc)
        assert all(a[1].tobytes() == b[1].tobytes() for a, b in zip(acc, wacc)), j
        assert rows.dtype == np.float32 and rows.shape == wrows.shape, (j, rows.shape, wrows.shape)
        assert rows.tobytes() == wrows.tobytes(), j
    return want


def n_valid(scene_):
    return len(A.valid_points(scene_[0], A.kitti_io.Calibration(scene_[1]), SHAPE, A.area_scope("Car"))[0])


@pytest.mark.parametrize("class_name,aug_times", RUNS)
def test_g19_tree_on_the_device(tree, databases, tmp_path, class_name, aug_times):  # noqa: F811
    save_dir, lines = str(tmp_path / "aug"), []
    A.generate_aug_scene(tree, databases[class_name][0], save_dir, class_name=class_name, aug_times=aug_times, device="cuda", batch_size=4,
                         log=lines.append)
    check_against_g19(class_name, tree, databases[class_name][0], save_dir, lines)


def test_tile_boundaries_in_one_batch():
    """clouds of 0, 1, 63, 64, 65 and 130 valid points (among invalid ones), a cloud of one raw point, an empty cloud"""
    rng = np.random.default_rng(1901)
    places = [(8.0, 12.0), (20.0, 30.0), (30.0, 50.0)]
    db = [entry(rng, x, z, ry) for (x, z), ry in zip(places, (0.0, 0.7, -1.2))] + [entry(rng, 12.0, 60.0)]
    sizes = (0, 1, 63, 64, 65, 130)
    scenes = [scene(cloud(rng, n, 37 + 5 * k, places)) for k, n in enumerate(sizes)]
    scenes.append(scene(np.array([[8.0, 1.0, 12.0, 0.5]], dtype=np.float32)))          # one raw point: numpy's gemv arithmetic
    scenes.append(scene(np.zeros((0, 4), np.float32)))
    cal = helpers.fake_kitti_calib(rng)
    fake = {"P2": cal["P2"], "R0": cal["R0_rect"], "Tr_velo2cam": cal["Tr_velo_to_cam"]}
    Rv, tv = fake["Tr_velo2cam"][:, :3], fake["Tr_velo2cam"][:, 3]
    one = ((np.array([[2.0, 1.0, 20.0]]) @ fake["R0"] - tv) @ Rv)
    scenes.append((np.concatenate([one, [[0.25]]], 1).astype(np.float32), fake, (375, 1242), FAR_BOX, LEVEL))
    assert [n_valid(s) for s in scenes[:8]] == list(sizes) + [1, 0]
    jobs = [(s, [0, 1, 2]) for s in range(len(scenes))] + [(5, [2, 0]), (3, [])]
    want = check(scenes, jobs, db)
    assert all(len(acc) == 3 for _, acc in want[:9]) and want[-1][1] == []
    assert len(want[5][0]) < 130 + 120 and len(want[6][0]) == 120                       # points were removed; the one point too
    assert len(want[8][0]) == 121 and len(want[-1][0]) == 64


def test_scan_carry_past_256_tiles():
    """16385 points are 257 tiles (the scan's second round holds one tile), 2 * 16384 + 65 points three rounds with a ragged last
    tile; invalid points among the valid ones.  Two jobs per scene; the clouds are unordered, so the accepted boxes remove points in the
    first round and in the last, and kept rows land behind a non-zero carry."""
    rng = np.random.default_rng(1908)
    places = [(8.0, 12.0), (20.0, 30.0), (30.0, 50.0)]
    db = [entry(rng, x, z, ry) for (x, z), ry in zip(places, (0.0, 0.7, -1.2))] + [entry(rng, 12.0, 60.0)]
    sizes = (16385, 2 * 16384 + 65)
    clouds = [cloud(rng, n - 1500, 1500, places) for n in sizes]
    clouds[0][-1], clouds[1][-1] = (8.0, 1.0, 12.0, 0.5), (20.0, 1.0, 30.0, 0.5)           # the last tile's last point: under entry 0 / 1
    scenes = [scene(c) for c in clouds]
    assert [len(s[0]) for s in scenes] == list(sizes)
    jobs = [(0, [0, 1, 2]), (0, [2, 0]), (1, [0, 1, 2]), (1, [1])]
    want = check(scenes, jobs, db)
    assert [[i for i, _ in acc] for _, acc in want] == [[0, 1, 2], [2, 0], [0, 1, 2], [1]]
    for (s, _), (rows, acc) in zip(jobs, want):
        pts, n = scenes[s][0], sizes[s]
        assert abs(n_valid(scenes[s]) - (n - 1500)) <= 1                                   # (the planted point took a row's place)
        kept = {r.tobytes() for r in rows[:len(rows) - 40 * len(acc)]}
        ok = (pts[:, 0] >= 1) & (pts[:, 1] >= 0.05) & (pts[:, 2] <= 66)                      # cloud()'s valid rows (rect = velodyne here)
        gone = np.array([ok[i] and pts[i].tobytes() not in kept for i in range(n)])
        assert len(kept) + gone.sum() == n_valid(scenes[s])
        last = 16384 * ((n - 1) // 16384)                                                  # where the scan's last round begins
        assert gone[:16384].any() and gone[last:].any() and gone[n - 1]


def test_more_label_boxes_than_one_chunk():
    C = G.box_chunk()
    rng = np.random.default_rng(1902)
    grid = np.array([[2.0 + 4.2 * (k % 8), 1.7, 6.0 + 6.0 * (k // 8), 1.5, 1.6, 3.0, 0.1 * k] for k in range(C + 1)], dtype=np.float32)
    assert grid[:, 2].max() < 66
    last = grid[C]
    db = [entry(rng, float(last[0]) + 0.5, float(last[2]) + 0.3, 0.4),                  # meets the LAST box only (chunk 2)
          entry(rng, float(grid[3][0]), float(grid[3][2]) + 0.2, 1.0),                  # meets box 3 (chunk 1)
          entry(rng, 36.0, 66.0), entry(rng, 5.0, 1.0)]
    sc = scene(cloud(rng, 500, 40, [(36.0, 66.0)]), grid)
    want = check([sc, scene(cloud(rng, 300, 10), grid[:C])], [(0, [0, 1, 2]), (1, [0, 1, 2]), (0, [2, 0])], db)
    assert [[i for i, _ in acc] for _, acc in want] == [[2], [0, 2], [2]]


def test_sixteen_accepted_and_sixteen_rejected():
    rng = np.random.default_rng(1903)
    db = [entry(rng, 3.0 + 8.0 * (k % 4), 8.0 + 14.0 * (k // 4), 0.3 * k, n=5 + k) for k in range(16)]
    db += [entry(rng, 20.0 + 0.1 * k, 40.0, 0.2 * k) for k in range(16)] + [entry(rng, 1.0, 1.0)]
    label = np.array([[20.5, 1.7, 40.2, 1.5, 1.6, 4.0, 0.5]], dtype=np.float32)
    pts = cloud(rng, 900, 50, [(3.0 + 8.0 * (k % 4), 8.0 + 14.0 * (k // 4)) for k in range(16)])
    far = scene(pts)
    want = check([far, scene(pts, label)], [(0, list(range(16))), (1, list(range(16, 32))), (0, list(range(15, -1, -1)))], db)
    assert [i for i, _ in want[0][1]] == list(range(16)) and want[1][1] == [] and [i for i, _ in want[2][1]] == list(range(15, -1, -1))
    assert len(want[1][0]) == 900 and len(want[0][0]) < 900 + sum(5 + k for k in range(16))
    assert want[0][0].tobytes() != want[2][0].tobytes()                                 # the objects' rows follow the acceptance order


def test_chain_blocked_by_the_previous_accepted_only():
    """boxes in a row, 0.15 m apart: k meets k - 1 only through the + 0.5 enlargement, so every second one is placed"""
    rng = np.random.default_rng(1904)
    db = [entry(rng, 3.0 + 4.15 * k, 20.0) for k in range(8)] + [entry(rng, 10.0, 30.0 + 1.75 * k) for k in range(8)] + [entry(rng, 1.0, 1.0)]
    sc = scene(cloud(rng, 400, 20, [(15.0, 20.0), (10.0, 36.0)]))
    want = check([sc], [(0, list(range(8))), (0, list(range(8, 16))), (0, [1, 0, 2, 3]), (0, [0, 2, 1, 4])], db)
    assert [[i for i, _ in acc] for _, acc in want] == [[0, 2, 4, 6], [8, 10, 12, 14], [1, 3], [0, 2, 4]]


def test_bev_overlap_with_disjoint_heights():
    """On a steep plane two boxes 1 m apart along z stand 2 m apart in height: both are placed, their h + 2 enlargements share
    points, and such a point is dropped once."""
    rng = np.random.default_rng(1905)
    plane = np.array([0.0, -1.0, -2.0, 22.5]) / np.sqrt(5.0)                            # road height 22.5 - 2 z
    db = [entry(rng, 10.0, 10.0), entry(rng, 10.0, 11.0), entry(rng, 1.0, 1.0)]
    shared = np.stack([rng.uniform(8.5, 11.5, 60), rng.uniform(0.02, 0.45, 60), rng.uniform(10.3, 10.7, 60)], 1)
    pts = np.concatenate([cloud(rng, 300, 20)[:, :3], shared], 0)
    pts = np.concatenate([pts, rng.random((len(pts), 1))], 1).astype(np.float32)
    sc = scene(pts, FAR_BOX, plane)
    want = check([sc], [(0, [0, 1]), (0, [0]), (0, [1])], db)
    assert [[i for i, _ in acc] for _, acc in want] == [[0, 1], [0], [1]]
    a, b = want[0][1][0][1], want[0][1][1][1]
    assert a[1] - a[3] > b[1]                                                           # disjoint heights
    kept = [len(rows) - 40 * len(acc) for rows, acc in want]
    gone = [n_valid(sc) - k for k in kept]
    assert gone[1] >= 60 and gone[2] >= 60 and gone[0] < gone[1] + gone[2]              # the shared points were in both


def test_edge_to_edge_and_the_10m_rule():
    rng = np.random.default_rng(1906)
    label = np.array([[12.0, 1.7, 30.0, 1.5, 1.5, 4.0, 0.0]], dtype=np.float32)         # grown: x in [9.75, 14.25], z in [29, 31]
    long_box = entry(rng, 20.0, 50.0, 0.0, (1.5, 2.0, 24.0))
    db = [entry(rng, 7.75, 30.0), entry(rng, 7.7499, 30.0), entry(rng, 7.76, 30.0), entry(rng, 12.0, 32.0, hwl=(1.5, 2.0, 4.0)), long_box,
          entry(rng, 1.0, 1.0)]
    ends = np.stack([np.concatenate([rng.uniform(8.5, 9.9, 30), rng.uniform(30.1, 31.5, 30)]), rng.uniform(0.4, 1.5, 60),
                     rng.uniform(49.2, 50.8, 60)], 1)                                   # inside the long box, > 10 m from its centre
    mid = np.stack([rng.uniform(11.0, 29.0, 80), rng.uniform(0.4, 1.5, 80), rng.uniform(49.2, 50.8, 80)], 1)
    pts = np.concatenate([cloud(rng, 200, 10)[:, :3], ends, mid], 0)
    pts = np.concatenate([pts, rng.random((len(pts), 1))], 1).astype(np.float32)
    sc = scene(pts, label)
    want = check([sc], [(0, [0]), (0, [1]), (0, [2]), (0, [3]), (0, [4])], db)
    # 7.75 + 2 = 9.75 = the grown label's face, and 32 - 1 = 31 likewise: the oracle's overlap of boxes that share an edge is exactly 0,
    # so they are placed (as the reference would); 1 cm inside they are not
    assert [[i for i, _ in acc] for _, acc in want] == [[0], [1], [], [3], [4]]
    rows = want[4][0]
    kept = rows[:len(rows) - 40, :3]
    has = lambda p: bool((np.abs(kept - p.astype(np.float32)).max(1) == 0).any())
    assert all(has(p) for p in ends) and not any(has(p) for p in mid)


def test_empty_batches_and_a_used_handle():
    rng = np.random.default_rng(1907)
    db = [entry(rng, 10.0, 20.0), entry(rng, 20.0, 40.0), entry(rng, 1.0, 1.0)]
    assert A.place_candidates([], [], db, device="cuda") == []
    sc = scene(cloud(rng, 200, 10, [(10.0, 20.0)]))
    assert A.place_candidates([sc], [], db, device="cuda") == []
    placer = A.AugPlacer(db, "cuda")
    scope = A.area_scope("Car")
    big = placer([scene(cloud(rng, 3000, 100, [(10.0, 20.0), (20.0, 40.0)]))] * 2, [(0, [0, 1]), (1, [1, 0]), (0, [])], scope)
    small = placer([sc], [(0, [1, 0])], scope)
    want = check([sc], [(0, [1, 0])], db)
    assert small[0][0].tobytes() == want[0][0].tobytes() and len(big) == 3 and len(big[2][0]) == 3000
    with pytest.raises(ValueError, match="no label besides DontCare"):
        A.place_candidates([scene(sc[0], np.zeros((0, 7)))], [(0, [0])], db, device="cuda")
