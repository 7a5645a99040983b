"""Seeded LiDAR sweeps with a KNOWN ring per point, and dataset-layout trees of them, for beam resampling (tests/test_beam_resample.py,
tests/test_gpu_beam_resample.py, profiles/beam_resample_probe.py).  Nothing here comes from a dataset or from the reference project.

A sweep: rays from the origin of the velodyne frame (x forward, y left, z up); ``beams`` elevations uniformly spaced over ELEVATION
(the lowest is ring 0), ``azimuths`` directions in an azimuth fan around the sensor.  A ray ends on the ground plane z = -GROUND or on a
closed wall ring (the cylinder of radius WALL around the sensor), whichever comes first: every beam returns.  The noise (sigma 2 cm) moves
a point ALONG its ray only, so its z / sqrt(x x + y y) is its ring's tangent up to the f32 rounding of the three coordinates.  The rows
are shuffled: a ring cannot be read off the row order.

``open_sky``: the wall ring is left out.  A ray that meets the ground within MAX_RANGE returns, the upper beams return nothing.  ``dead``
names rings whose laser never returns (a missing beam BETWEEN others).
"""
import os

import numpy as np

ELEVATION = (-24.8, 2.0)                 # degrees, lowest and highest beam
GROUND, WALL, MAX_RANGE, SIGMA = 1.73, 40.0, 80.0, 0.02
TREE_IDS = ("000001", "000004", "000009", "000012", "000020", "000033")
TREE_AZIMUTHS = (40, 64, 100, 33, 129, 70)
TREE_BEAMS = 16


def elevations(beams):
    return np.radians(np.linspace(ELEVATION[0], ELEVATION[1], beams))


def _sweep(seed, beams, azimuths, wall, dead=()):
    rng = np.random.default_rng(seed)
    ring, az = np.meshgrid(np.arange(beams), rng.uniform(-np.pi, np.pi, azimuths), indexing="ij")
    ring, az = ring.reshape(-1), az.reshape(-1)
    el = elevations(beams)[ring]
    with np.errstate(divide="ignore"):
        to_ground = np.where(el < 0.0, GROUND / -np.sin(np.minimum(el, -1e-12)), np.inf)
    reach = np.minimum(to_ground, WALL / np.cos(el)) if wall else to_ground
    back = (reach <= MAX_RANGE) & ~np.isin(ring, list(dead))
    ring, az, el, reach = ring[back], az[back], el[back], reach[back]
    reach = reach + rng.normal(0.0, SIGMA, len(reach))
    rows = np.stack([reach * np.cos(el) * np.cos(az), reach * np.cos(el) * np.sin(az), reach * np.sin(el), rng.random(len(reach))], 1)
    order = rng.permutation(len(rows))
    return np.ascontiguousarray(rows[order], dtype=np.float32), ring[order].astype(np.int32)


def wall_ring(seed, beams, azimuths):
    """-> (points (beams * azimuths, 4) f32, rings (beams * azimuths,) int32): every beam returns"""
    return _sweep(seed, beams, azimuths, True)


def open_sky(seed, beams, azimuths, dead=()):
    """-> (points, rings) of the beams that meet the ground within MAX_RANGE and are not ``dead``"""
    return _sweep(seed, beams, azimuths, False, dead)


def write_tree(root, beams=TREE_BEAMS):
    """A tree in the dataset layout under ``root``: training/{velodyne, label_2, calib, image_2, planes} and the split files
    -> (ids, the sweeps, their rings)"""
    tr = os.path.join(root, "training")
    for sub in ("velodyne", "label_2", "calib", "image_2", "planes"):
        os.makedirs(os.path.join(tr, sub), exist_ok=True)
    clouds, rings = zip(*[wall_ring(700 + k, beams, az) for k, az in enumerate(TREE_AZIMUTHS)])
    for i, c in zip(TREE_IDS, clouds):
        c.tofile(os.path.join(tr, "velodyne", "%s.bin" % i))
        for sub, ext, text in (("label_2", "txt", "Car 0.00 0 0.00 0 0 50 50 1.50 1.60 3.90 1.00 1.65 %d.00 0.00\n" % (10 + int(i))),
                               ("calib", "txt", "P2: 1 0 0 0 0 1 0 0 0 0 1 0\n"), ("image_2", "png", "not an image\n"),
                               ("planes", "txt", "# Plane\nWidth 4\nHeight 1\n0 -1 0 1.65\n")):
            with open(os.path.join(tr, sub, "%s.%s" % (i, ext)), "w") as f:
                f.write(text)
    for split, which in (("train", TREE_IDS[0::2]), ("val", TREE_IDS[1::2]), ("trainval", TREE_IDS)):
        with open(os.path.join(root, "%s.txt" % split), "w") as f:
            f.write("".join("%s\n" % i for i in which))
    return list(TREE_IDS), list(clouds), list(rings)


def listing(root):
    """Every file under ``root`` (links to directories not followed) with its bytes, every link with its target"""
    out = {}
    for d, dirs, files in os.walk(root):
        for name in dirs + files:
            path = os.path.join(d, name)
            if os.path.islink(path):
                out[os.path.relpath(path, root)] = ("link", os.readlink(path))
            elif os.path.isfile(path):
                with open(path, "rb") as f:
                    out[os.path.relpath(path, root)] = ("file", f.read())
    return out
