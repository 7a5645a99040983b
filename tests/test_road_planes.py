"""Road-plane estimation (3d_adapt_auto_driving_amd/road_planes.py), host side: the cpu path against KNOWN synthetic planes
(tests/planes_tree.py), its tie / rejection / fallback rules on hand-made draw tables, the file format against the package's two
readers, and the tool on a six-scene tree.  No fixture comes from the reference project: it has no counterpart."""
import importlib
import os

import numpy as np
import pytest

import planes_tree as T

PKG = "3d_adapt_auto_driving_amd"
R = importlib.import_module(PKG + ".road_planes")
A = importlib.import_module(PKG + ".aug_scene")
K = importlib.import_module(PKG + ".kitti_eval")
quiet = lambda s: None
DEFAULT = [0.0, -1.0, 0.0, 1.65]


def flat(rows):
    """Rect rows -> a scene whose LiDAR frame is the rect frame"""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 3)
    return np.concatenate([rows, np.zeros((len(rows), 1), np.float32)], 1), T.identity_calib()


def pick(table, m):
    """Candidate indices per hypothesis -> the draws that select them among m candidates"""
    return (np.asarray(table, dtype=np.float64) + 0.5) / m


def ground_rows(n, y=1.65, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-10, 10, n), np.full(n, y), rng.uniform(5, 30, n)], 1)


def one(rows, table, **kw):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    planes, infos = R.estimate_planes([flat(rows)], device="cpu", iters=len(table), u=[pick(table, len(rows))], details=True, **kw)
    return planes[0], infos[0]


# ---------------------------------------------------------------------------------------------------------------- recovery
def test_recovers_the_known_plane_of_forty_seeded_scenes():
    """Bars: 0.1 deg and 2 cm on every scene (noise alone predicts about 0.006 deg and 2 mm at N = 512).
    Worst case this implementation reaches over the 40 scenes: 0.011269 deg and 4.682 mm (printed below on every run)."""
    scenes, truths = zip(*[T.recovery_scene(k) for k in range(40)])
    planes, infos = R.estimate_planes(scenes, device="cpu", iters=256)
    errors = np.array([T.plane_error(p, t) for p, t in zip(planes, truths)])
    print("worst angle %.6f deg, worst height %.6f m" % (errors[:, 0].max(), errors[:, 1].max()))
    for p, info in zip(planes, infos):
        assert info["fallback"] is None and info["best_hypothesis"] >= 0
        assert abs(np.linalg.norm(p[0:3]) - 1.0) < 1e-12 and p[1] < 0 and p[3] > 0
        assert info["inliers"] >= info["ransac_inliers"] * 0.9 and info["rms"] < 0.05
    assert errors[:, 0].max() < 0.1 and errors[:, 1].max() < 0.02


# ------------------------------------------------------------------------------------------------------- ties and rejections
def test_two_identical_rows_give_the_smaller_index():
    rows = ground_rows(200)
    plane, info = one(rows, [[0, 1, 2], [3, 50, 120], [3, 50, 120], [3, 50, 120]], min_inliers=100)
    assert info["accepted"].tolist() == [True] * 4 and info["scores"].tolist() == [200] * 4
    assert info["best_hypothesis"] == 0
    rows[0:3, 1] = 1.0                                       # row 0's triple now spans another plane with fewer inliers
    plane, info = one(rows, [[0, 1, 2], [3, 50, 120], [3, 50, 120]], min_inliers=100)
    assert info["scores"][1] == info["scores"][2] > info["scores"][0] and info["best_hypothesis"] == 1


def test_three_collinear_points_are_rejected():
    rows = ground_rows(200)
    rows[0:3] = [[0, 1.65, 5], [1, 1.65, 6], [2, 1.65, 7]]
    plane, info = one(rows, [[0, 1, 2], [0, 0, 1], [3, 50, 120]], min_inliers=100)
    assert info["accepted"].tolist() == [False, False, True] and info["scores"].tolist() == [0, 0, 200]
    assert info["best_hypothesis"] == 2


def test_a_wall_with_more_points_loses_to_the_ground_by_the_tilt_bound():
    rng = np.random.default_rng(3)
    wall = np.stack([np.full(300, 5.0), rng.uniform(-2, 1.6, 300), rng.uniform(5, 30, 300)], 1)
    rows = np.concatenate([wall, ground_rows(200)], 0)
    plane, info = one(rows, [[0, 1, 2], [300, 350, 420], [10, 20, 30]], min_inliers=100)
    assert info["accepted"].tolist() == [False, True, False]
    assert info["best_hypothesis"] == 1 and info["ransac_inliers"] >= 200 and info["fallback"] is None
    # (the wall's few points within thresh of the ground take part in the refits: a small pull, far inside these bounds)
    assert T.plane_error(plane, np.array(DEFAULT))[0] < 0.5 and abs(plane[3] - 1.65) < 0.05


def test_a_plane_above_the_sensor_is_rejected():
    rows = np.concatenate([ground_rows(300, y=-2.0, seed=1), ground_rows(200)], 0)
    plane, info = one(rows, [[0, 1, 2], [300, 350, 420]], min_inliers=100)
    assert info["accepted"].tolist() == [False, True] and info["best_hypothesis"] == 1
    assert abs(plane[3] - 1.65) < 1e-6 and plane[1] < 0


# ---------------------------------------------------------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("rows, reason", [
    (np.zeros((0, 3)), 1),
    ([[0, 1.65, 80], [0, 1.65, 90], [30, 1.65, 10]], 1),                      # points, but M = 0
    ([[0, 1.65, 5], [1, 1.65, 6]], 1),                                         # M = 2
    (np.stack([np.arange(50.0) * 0.25, np.full(50, 1.625), 5 + np.arange(50.0) * 0.5], 1), 2),   # every candidate on one line (exact in f32)
    (ground_rows(50), 3),                                                       # best score below min_inliers
])
def test_fallbacks_give_the_default_plane_and_a_reason(rows, reason):
    planes, infos = R.estimate_planes([flat(rows)], device="cpu", iters=64, min_inliers=100)
    assert planes[0].tolist() == DEFAULT
    assert infos[0]["best_hypothesis"] == -1 and infos[0]["fallback"] == R.FALLBACK_REASONS[reason]
    assert infos[0]["ransac_inliers"] == (50 if reason == 3 else 0)
    planes, _ = R.estimate_planes([flat(rows)], device="cpu", iters=64, min_inliers=100, default_height=1.8)
    assert planes[0].tolist() == [0.0, -1.0, 0.0, 1.8]


# -------------------------------------------------------------------------------------------------------------- file format
@pytest.mark.parametrize("plane", [[1.234567891e-2, -9.998765432e-1, -9.87654321e-3, 1.723456789], [-0.02, 0.9996, 0.01, -1.6]])
def test_write_plane_is_read_back_by_both_readers(tmp_path, plane):
    path = str(tmp_path / "000007.txt")
    plane = np.asarray(plane) / np.linalg.norm(plane[0:3])
    if plane[1] > 0:
        plane = -plane
    R.write_plane(path, plane)
    lines = open(path).read().split("\n")
    assert lines[0:3] == ["# Plane", "Width 4", "Height 1"] and len(lines) == 5 and lines[4] == ""      # four lines
    assert float(lines[3].split()[1]) < 0
    for got in (A.road_plane(path), K.read_plane(path)):
        assert got.shape == (4,) and np.all(np.abs(got - plane) <= 1e-6 * np.maximum(np.abs(plane), 1e-1))


# --------------------------------------------------------------------------------------------------------------------- tool
def test_the_tool_on_a_six_scene_tree(tmp_path):
    root = str(tmp_path / "tree")
    ids = T.write_tree(root)
    base = os.path.join(root, "KITTI", "object", "training")
    lines = []
    got = R.generate_planes(root, device="cpu", iters=128, batch=4, log=lines.append)
    assert [g[0] for g in got] == ids and all(g[2]["fallback"] is None for g in got)
    assert sorted(os.listdir(os.path.join(base, "planes"))) == sorted(["%06d.txt" % i for i in ids] + [R.LOG_NAME])
    log = open(os.path.join(base, "planes", R.LOG_NAME)).read().splitlines()
    assert len(log) == 7 and [ln[:6] for ln in log[:6]] == ["%06d" % i for i in ids] and "0 on the fallback plane" in log[6]
    assert all(name + "=" in log[0] for name in R.INFO_FIELDS)
    for pos, (i, plane, info) in enumerate(got):
        read = A.road_plane(os.path.join(base, "planes", "%06d.txt" % i))
        assert np.all(np.abs(read - plane) < 1e-6)
        angle, height = T.plane_error(plane, T.true_plane(*T.seeded_pose(500 + pos)))
        assert angle < 0.1 and height < 0.02
    # a second run without --overwrite: raises, names the file, changes nothing
    before = T.listing(root)
    with pytest.raises(FileExistsError) as e:
        R.generate_planes(root, device="cpu", iters=128, log=quiet)
    assert os.path.join(base, "planes", "%06d.txt" % ids[0]) in str(e.value) and T.listing(root) == before
    # --check on the tree it just wrote: zero differences within the %e precision, nothing written
    lines = []
    figures = R.generate_planes(root, device="cpu", iters=128, check=True, log=lines.append)
    assert [f[0] for f in figures] == ids and len(lines) == 7 and "median" in lines[6]
    assert max(f[1] for f in figures) < 1e-4 and max(f[2] for f in figures) < 1e-5
    assert T.listing(root) == before
    # --save_dir writes elsewhere; --overwrite replaces
    other = str(tmp_path / "elsewhere")
    R.main(["--root", root, "--save_dir", other, "--device", "cpu", "--iters", "128"])
    assert sorted(os.listdir(other)) == sorted(os.listdir(os.path.join(base, "planes"))) and T.listing(root) == before
    for i in ids:
        assert open(os.path.join(other, "%06d.txt" % i)).read() == open(os.path.join(base, "planes", "%06d.txt" % i)).read()
    R.main(["--root", root, "--overwrite", "--device", "cpu", "--iters", "128", "--x_range", "-20", "20", "--z_range", "0", "50"])
    after = T.listing(root)
    assert set(after) == set(before) and all(after[k][0] == before[k][0] for k in before)


def test_the_draws_follow_the_sample_id_not_the_position():
    (s0, _), (s1, _) = T.recovery_scene(0), T.recovery_scene(3)
    both, _ = R.estimate_planes([s0, s1], device="cpu", iters=64, ids=[11, 5])
    single, _ = R.estimate_planes([s1], device="cpu", iters=64, ids=[5])
    assert both[1].tobytes() == single[0].tobytes()
    assert np.array_equal(R.draws_of(3, 4, 16), np.random.RandomState(7).random_sample((16, 3)))
