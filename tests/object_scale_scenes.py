"""Seeded scenes for the object-scaling tests (test_object_scale.py, test_gpu_object_scale.py): boxes on a 10 m grid -- centres at least
8 m apart, so that no box, enlarged band or grown box reaches a neighbour -- with ry over (-pi, pi), and points drawn within 0.6 of the
extents about the box centres (some inside, some in the band around the box)."""
import numpy as np

GRID = 10.0


def isolated_boxes(rng, g):
    """(g, 7) f32 [x, y_bottom, z, h, w, l, ry] on distinct grid nodes, jittered by less than 1 m"""
    side = int(np.ceil(np.sqrt(max(g, 1))))
    nodes = rng.permutation(side * side)[:g]
    boxes = np.zeros((g, 7), dtype=np.float64)
    boxes[:, 0] = (nodes % side - 0.5 * (side - 1)) * GRID + rng.uniform(-1.0, 1.0, g)
    boxes[:, 2] = 10.0 + (nodes // side) * GRID + rng.uniform(-1.0, 1.0, g)
    boxes[:, 1] = rng.uniform(1.4, 1.9, g)
    boxes[:, 3] = rng.uniform(1.3, 1.9, g)
    boxes[:, 4] = rng.uniform(1.4, 1.9, g)
    boxes[:, 5] = rng.uniform(3.2, 4.6, g)
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, g)
    return boxes.astype(np.float32)


def cluster_points(rng, boxes, n):
    """(n, 3) f32: point i belongs to box i % g and lies within 0.6 of the extents about the box centre (x, y - h / 2, z)"""
    g = boxes.shape[0]
    b = boxes[np.arange(n) % g].astype(np.float64)
    u = rng.uniform(-0.6, 0.6, (n, 3))
    a, v, w = u[:, 0] * b[:, 5], u[:, 1] * b[:, 3], u[:, 2] * b[:, 4]
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    pts = np.stack([b[:, 0] + a * c + w * s, b[:, 1] - 0.5 * b[:, 3] + v, b[:, 2] - a * s + w * c], axis=1)
    return pts.astype(np.float32)


def isolated_scenes(seed, B, N, G, lo=0.75, hi=1.25):
    """-> pts (B, N, 3) f32, gt list of B (G, 7) f32, factors (B, G) f64 in [lo, hi]"""
    rng = np.random.default_rng(seed)
    gts = [isolated_boxes(rng, G) for _ in range(B)]
    pts = np.stack([cluster_points(rng, g, N) for g in gts])
    return pts, gts, rng.uniform(lo, hi, (B, G))


def operator_case(seed, B, N, G, counts=None):
    """The device tests' case: isolated clusters, plus (G >= 2) box 1 = box 0 moved by half a metre (an overlapping pair: points inside
    both), a negative ry in box 0, a factor of exactly 1.0 in every scene, and counts below G where ``counts`` says so.
    -> pts, gt (B, G, 7), counts (B,) i32, factors (B, G)"""
    pts, gts, factors = isolated_scenes(seed, B, N, G)
    gt = np.stack(gts)
    gt[:, 0, 6] = -np.abs(gt[:, 0, 6]) - np.float32(0.25)
    if G >= 2:
        gt[:, 1] = gt[:, 0]
        gt[:, 1, 0] += np.float32(0.5)
        gt[:, 1, 6] += np.float32(0.3)
    rng = np.random.default_rng(seed + 1)
    pts = np.stack([cluster_points(rng, g, N) for g in gt])
    factors[np.arange(B), np.arange(B) % G] = 1.0
    counts = np.full(B, G, dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    gt[np.arange(G)[None, :] >= counts[:, None]] = 0.0                  # zero rows past each count, as pack_gt leaves them
    return pts, gt, counts, factors
