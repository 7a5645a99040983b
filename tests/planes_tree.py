"""Seeded LiDAR scenes over a KNOWN road plane, and fake KITTI trees of them, for road-plane estimation (tests/test_road_planes.py,
tests/test_gpu_road_planes.py, profiles/road_planes_probe.py).  Nothing here comes from a dataset or from the reference project.

The scene (seed, N, pitch, roll, height), in the rect frame: x uniform in +-20, z uniform in 0..40, the ground
y = -(n_x x + n_z z + height) / n_y with n = (sin roll, -cos roll cos pitch, sin pitch), plus Gaussian noise of sigma 0.02 m.  The first
35 % of the rows are outliers: half of them lifted 0.3 .. 3.0 m above the ground, the other half a slab 1.5 m above the ground over x in
+-3, z in 5..12 (car roofs).  ``outside`` further rows beyond the estimator's z range are mixed in at seeded positions (they are no
candidates: the compaction has something to skip).  The rows go to the LiDAR frame through the inverse of one fixed calibration.
"""
import os

import numpy as np

import helpers

CALIB_SEED = 2400
SIGMA = 0.02
TREE_IDS = (1, 4, 9, 12, 20, 33)
TREE_SIZES = (700, 1500, 2111, 4096, 999, 3000)
RECOVERY_SIZES = (512, 4096, 20000)


def calib_arrays():
    """The fixed calibration as helpers.fake_kitti_calib makes it (float64 arrays by the calib file's keys)"""
    return helpers.fake_kitti_calib(np.random.default_rng(CALIB_SEED))


def calib_dict(cal=None):
    """... as kitti_io.Calibration takes it"""
    cal = cal if cal is not None else calib_arrays()
    return {"P2": cal["P2"], "R0": cal["R0_rect"], "Tr_velo2cam": cal["Tr_velo_to_cam"]}


def identity_calib():
    """LiDAR frame = rect frame, exactly (products with 1 and 0)"""
    return {"P2": np.array([[700.0, 0, 600, 0], [0, 700, 180, 0], [0, 0, 1, 0]]), "R0": np.eye(3), "Tr_velo2cam": np.eye(3, 4)}


def true_plane(pitch, roll, height):
    """-> (4,) f64: unit normal facing up (b < 0), d > 0"""
    n = np.array([np.sin(roll), -np.cos(roll) * np.cos(pitch), np.sin(pitch), height], dtype=np.float64)
    return n / np.linalg.norm(n[0:3])


def rect_rows(seed, n, pitch, roll, height, outside=0):
    """-> (n + outside, 3) f64 rows in the rect frame"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = np.sin(roll), -np.cos(roll) * np.cos(pitch), np.sin(pitch)

    def ground(x, z):
        return -(nx * x + nz * z + height) / ny

    x, z = rng.uniform(-20, 20, n), rng.uniform(0, 40, n)
    y = ground(x, z) + rng.normal(0.0, SIGMA, n)
    n_out = int(0.35 * n)
    lifted = n_out // 2
    y[:lifted] -= rng.uniform(0.3, 3.0, lifted)                                  # up is -y
    x[lifted:n_out], z[lifted:n_out] = rng.uniform(-3, 3, n_out - lifted), rng.uniform(5, 12, n_out - lifted)
    y[lifted:n_out] = ground(x[lifted:n_out], z[lifted:n_out]) - 1.5 + rng.normal(0.0, SIGMA, n_out - lifted)
    rows = np.stack([x, y, z], 1)
    if outside:
        far = np.stack([rng.uniform(-20, 20, outside), rng.uniform(-1, 2, outside), rng.uniform(60, 70, outside)], 1)
        rows = np.concatenate([rows, far], 0)
        where = np.sort(rng.permutation(len(rows))[:outside])
        order = np.empty(len(rows), dtype=np.int64)                              # the ground rows keep their order; the far rows land at ``where``
        mask = np.zeros(len(rows), dtype=bool)
        mask[where] = True
        order[mask], order[~mask] = np.arange(n, n + outside), np.arange(n)
        rows = rows[order]
    return rows


def to_lidar(rect, cal=None, seed=0):
    """Rect rows -> (n, 4) f32 LiDAR rows (x, y, z, intensity) through the inverse of the calibration"""
    cal = cal if cal is not None else calib_arrays()
    Rv, tv = cal["Tr_velo_to_cam"][:, :3], cal["Tr_velo_to_cam"][:, 3]
    velo = (rect @ cal["R0_rect"] - tv) @ Rv
    inten = np.random.default_rng(seed + 77).random((len(velo), 1))
    return np.concatenate([velo, inten], 1).astype(np.float32)


def scene(seed, n, pitch, roll, height, outside=0):
    """-> (points (n + outside, 4) f32 in the LiDAR frame, calib dict)"""
    return to_lidar(rect_rows(seed, n, pitch, roll, height, outside), seed=seed), calib_dict()


def seeded_pose(seed):
    """Pitch uniform in +-4 deg, roll uniform in +-3 deg, height uniform in 1.5 .. 1.9 m, from the scene seed"""
    rng = np.random.default_rng(100000 + seed)
    return np.radians(rng.uniform(-4, 4)), np.radians(rng.uniform(-3, 3)), rng.uniform(1.5, 1.9)


def recovery_scene(k):
    """Scene k of the recovery recipe: N cycles 512 / 4096 / 20000 -> ((points, calib), true plane)"""
    pitch, roll, height = seeded_pose(k)
    return scene(k, RECOVERY_SIZES[k % 3], pitch, roll, height), true_plane(pitch, roll, height)


def plane_error(plane, truth):
    """-> (angle between the normals in degrees, difference of the heights under the sensor in metres)"""
    cosv = float(np.clip(np.dot(plane[0:3], truth[0:3]), -1.0, 1.0))
    angle = np.degrees(np.arctan2(np.linalg.norm(np.cross(plane[0:3], truth[0:3])), cosv))
    return float(angle), float(abs(-plane[3] / plane[1] - (-truth[3] / truth[1])))


def write_tree(root, split="train"):
    """-> the sample ids of a tree under ``root``: KITTI/object/training/{velodyne, calib} and KITTI/ImageSets/<split>.txt"""
    base = os.path.join(root, "KITTI", "object", "training")
    for sub in ("velodyne", "calib"):
        os.makedirs(os.path.join(base, sub), exist_ok=True)
    os.makedirs(os.path.join(root, "KITTI", "ImageSets"), exist_ok=True)
    cal = calib_arrays()
    for pos, sid in enumerate(TREE_IDS):
        pitch, roll, height = seeded_pose(500 + pos)
        to_lidar(rect_rows(500 + pos, TREE_SIZES[pos], pitch, roll, height, outside=37 * pos), cal, seed=pos).tofile(
            os.path.join(base, "velodyne", "%06d.bin" % sid))
        with open(os.path.join(base, "calib", "%06d.txt" % sid), "w") as f:
            for key in ("P0", "P1", "P2", "P3", "R0_rect", "Tr_velo_to_cam", "Tr_imu_to_velo"):
                f.write("%s: %s\n" % (key, " ".join("%.12e" % v for v in cal[key].reshape(-1))))
    with open(os.path.join(root, "KITTI", "ImageSets", split + ".txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in TREE_IDS))
    return list(TREE_IDS)


def listing(root):
    """Every file under ``root`` with its size and mtime_ns"""
    out = {}
    for d, _, files in os.walk(root):
        for name in files:
            st = os.stat(os.path.join(d, name))
            out[os.path.relpath(os.path.join(d, name), root)] = (st.st_size, st.st_mtime_ns)
    return out
