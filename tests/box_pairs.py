"""Seeded families of BEV box PAIRS at the places where the rotated overlap (csrc/rbox_iou.hpp, oracle.boxes_overlap_bev) is hard:
exactly touching / nested boxes in exact arithmetic, near-coincident boxes (clipped polygons of 9..16 vertices), the same rectangle
turned by quarter turns, long thin boxes around the `rbox_far_apart` reach, and NMS scenes made of near-coincident clusters.
No tests in here: tests/test_box_pairs.py (CPU) and tests/test_gpu_box_pairs.py use it.

Conventions: a 3-D box is [x, y, z, h, w, l, ry] (y = bottom), its BEV box [x - l/2, z - w/2, x + l/2, z + w/2, ry] evaluated in f32 as
kitti_utils.boxes3d_to_bev_torch does; the long side l lies along x at heading 0 and points along (cos ry, -sin ry) otherwise (the
rotation of iou3d_kernel.cu:92-96)."""
import numpy as np

F = np.float32
SHAPES = {"car": ((3.0, 5.0), (1.4, 2.2)), "pedestrian": ((0.72, 0.88), (0.54, 0.66)), "cyclist": ((1.584, 1.936), (0.54, 0.66))}
# 0.1 / 0.5 / 0.8 decide between clusters.  0.999 and 1.001 decide INSIDE a cluster: the IoU of near-coincident boxes lies in
# [0.9998, 1.0001], so every member but the first goes at 0.999 and every box stays at 1.001 -- only if the clipped polygon of 9..16
# vertices is right; an overlap that comes out too small shows at 0.999, one that comes out too large at 1.001
NMS_THRESHOLDS = (0.1, 0.5, 0.8, 0.999, 1.001)
BAND = 1e-5
HEADING_NUDGES = (0.0, 1e-6, -1e-6, 3e-6)


# ------------------------------------------------------------------------------------------------------------------- converters
def to_3d(cx, cz, l, w, ry, y=1.6, h=1.5):
    """-> (n, 7) f32 boxes [x, y, z, h, w, l, ry]"""
    cx = np.asarray(cx, np.float64)
    one = np.ones_like(cx)
    return np.stack([cx, y * one, np.asarray(cz) * one, h * one, np.asarray(w) * one, np.asarray(l) * one, np.asarray(ry) * one], 1).astype(F)


def to_bev(b3):
    """(n, 7) -> (n, 5) f32, the f32 operations of kitti_utils.boxes3d_to_bev_torch"""
    b3 = np.asarray(b3, F)
    hl, hw = b3[:, 5] / F(2), b3[:, 4] / F(2)
    return np.ascontiguousarray(np.stack([b3[:, 0] - hl, b3[:, 2] - hw, b3[:, 0] + hl, b3[:, 2] + hw, b3[:, 6]], 1), dtype=F)


def bev_to_3d(bev, y=1.6, h=1.5):
    """(n, 5) -> (n, 7); exact (and the inverse of to_bev) when the coordinates are dyadic, as in the exact family"""
    bev = np.asarray(bev, F)
    return to_3d((bev[:, 0] + bev[:, 2]) / F(2), (bev[:, 1] + bev[:, 3]) / F(2), bev[:, 2] - bev[:, 0], bev[:, 3] - bev[:, 1], bev[:, 4], y, h)


# ----------------------------------------------------------------------------------------------------------------- exact family
# (rectangle a, rectangle b) as (x1, y1, x2, y2); sizes from {4x2, 2x4, 2x2, 2x1, 8x0.5}, every coordinate a multiple of 0.25
EXACT_CONFIGS = (
    ("identical", (0, 0, 4, 2), (0, 0, 4, 2)),
    ("touch_whole_edge", (0, 0, 4, 2), (4, 0, 8, 2)),
    ("touch_part_of_edge", (0, 0, 4, 2), (4, 1, 6, 3)),
    ("touch_corner", (0, 0, 4, 2), (4, 2, 6, 4)),
    ("t_junction_touching", (0, 0, 8, 0.5), (3, 0.5, 5, 4.5)),
    ("t_junction_overlapping", (0, 0, 8, 0.5), (3, -3.5, 5, 0.5)),
    ("nested_no_shared_edge", (0, 0, 4, 2), (1, 0.5, 3, 1.5)),
    ("nested_one_shared_edge", (0, 0, 4, 2), (1, 0, 3, 1)),
    ("nested_two_shared_edges", (0, 0, 4, 2), (1, 0, 3, 2)),
    ("nested_in_a_corner", (0, 0, 4, 2), (0, 0, 2, 1)),
    ("plus", (-2, -1, 2, 1), (-1, -2, 1, 2)),
    ("half_shift", (0, 0, 4, 2), (2, 0, 6, 2)),
    ("half_shift_both_axes", (0, 0, 4, 2), (2, 1, 6, 3)),
    ("strip_across_full_width", (0, 0, 2, 4), (0, 1.5, 2, 2.5)),
    ("strip_crossing", (0, 0, 2, 4), (-3, 1.75, 5, 2.25)),
)
NESTED_PAIR = ((0.0, 0.0, 4.0, 2.0, 0.0), (1.0, 0.0, 3.0, 2.0, 0.0))          # 2x2 in 4x2: overlap 4, IoU exactly 0.5


def closed_form_overlap(a, b):
    """axis-aligned intersection area of every a with every b (heading 0 boxes), f64 of exact dyadic values -> (na, nb) f32"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    return (np.clip(w, 0, None) * np.clip(h, 0, None)).astype(F)


def closed_form_iou(a, b):
    """overlap / max(sa + sb - overlap, 1e-8) in f32: exact operands, so one rounding in the division"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ov = closed_form_overlap(a, b)
    sa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
    sb = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    return (ov / np.maximum(sa + sb - ov, F(1e-8))).astype(F)


def exact_pairs(n=None):
    """-> (a (p, 5), b (p, 5), overlap (p,), names): every configuration where it is defined and translated so that the pair's upper
    right corner is (64, 48); with ``n`` the list goes on with further dyadic translations until it holds n pairs.
    Headings exactly 0, |coordinate| <= 64: every operation of the algorithm is exact in f32 (the division by the vertex count feeds
    the angular sort only)."""
    anchors = [None, (64.0, 48.0)]
    if n is not None:
        anchors += [(x, y) for y in (-40.0, -17.75, 3.5, 26.25, 47.0) for x in (-52.0, -35.25, -20.5, -3.75, 12.0, 29.5, 45.25, 62.0)]
    a, b, names = [], [], []
    for anchor in anchors:
        for name, ra, rb in EXACT_CONFIGS:
            ra, rb = np.array(ra, np.float64), np.array(rb, np.float64)
            if anchor is not None:
                shift = np.array([anchor[0] - max(ra[2], rb[2]), anchor[1] - max(ra[3], rb[3])])
                ra, rb = ra + np.tile(shift, 2), rb + np.tile(shift, 2)
            a.append(list(ra) + [0.0]); b.append(list(rb) + [0.0]); names.append(name)
    a, b = np.array(a, F), np.array(b, F)
    if n is not None:
        a, b, names = a[:n], b[:n], names[:n]
        assert len(a) == n
    assert np.abs(a[:, :4]).max() <= 64 and np.abs(b[:, :4]).max() <= 64
    assert (a[:, :4] * 4 == np.round(a[:, :4] * 4)).all() and (b[:, :4] * 4 == np.round(b[:, :4] * 4)).all()
    return a, b, np.diagonal(closed_form_overlap(a, b)).copy(), names


def threshold_scene(pairs):
    """NMS scene of ``pairs`` copies of the nested 2x2-in-4x2 pair on a grid 8 x 4 (no two pairs touch): IoU inside a pair exactly 0.5,
    between pairs exactly 0.  Even pairs list the 4x2 box first, odd pairs the 2x2 box.
    -> (boxes (2 pairs, 5) f32, keep list at threshold 0.5 (all), keep list at any threshold in [0, 0.5) (the first box of each pair))"""
    assert pairs <= 16 * 24
    out = []
    for k in range(pairs):
        shift = np.array([-64.0 + 8 * (k % 16), -48.0 + 4 * (k // 16)] * 2 + [0.0])
        pair = [np.array(NESTED_PAIR[0]) + shift, np.array(NESTED_PAIR[1]) + shift]
        out += pair if k % 2 == 0 else pair[::-1]
    return np.array(out, F), np.arange(2 * pairs, dtype=np.int64), np.arange(0, 2 * pairs, 2, dtype=np.int64)


# -------------------------------------------------------------------------------------------------------- near-coincident family
def nearly(rng, cx, cz, ry):
    """the partner of the recipe: per axis +-10^U(-7, -4.3), heading + one of HEADING_NUDGES (f64; the caller rounds to f32)"""
    n = len(cx)
    dx = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -4.3, n)
    dz = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -4.3, n)
    return cx + dx, cz + dz, ry + np.array(HEADING_NUDGES)[rng.integers(0, len(HEADING_NUDGES), n)]


def near_coincident_pairs(seed, n, shape="car"):
    """-> (a3, b3) (n, 7) f32: centre x in [-40, 40], z in [0, 70], heading exactly 0 for even rows and uniform in (-pi, pi) for odd
    rows; b = a moved by 1e-7 .. 5e-5 m per axis and 0 .. 3e-6 rad, same size."""
    rng = np.random.default_rng(seed)
    (l0, l1), (w0, w1) = SHAPES[shape]
    cx, cz = rng.uniform(-40, 40, n), rng.uniform(0, 70, n)
    l, w = rng.uniform(l0, l1, n), rng.uniform(w0, w1, n)
    ry = rng.uniform(-np.pi, np.pi, n)
    ry[0::2] = 0.0
    bx, bz, bry = nearly(rng, cx, cz, ry)
    return to_3d(cx, cz, l, w, ry), to_3d(bx, bz, l, w, bry)


def _trig(t):
    """the project's f32 trig contract: the f64 libm value rounded to f32"""
    t = np.asarray(t, F).astype(np.float64)
    return np.cos(t).astype(F), np.sin(t).astype(F)


def _corners(b, c, s):
    cx, cy = (b[:, 0] + b[:, 2]) / F(2), (b[:, 1] + b[:, 3]) / F(2)
    xs = np.stack([b[:, 0], b[:, 2], b[:, 2], b[:, 0]], 1)
    ys = np.stack([b[:, 1], b[:, 1], b[:, 3], b[:, 3]], 1)
    dx, dy = xs - cx[:, None], ys - cy[:, None]
    c, s = c[:, None], s[:, None]
    return (dx * c + dy * s) + cx[:, None], ((-dx) * s + dy * c) + cy[:, None]


def _cross3(p1x, p1y, p2x, p2y, p0x, p0y):
    return (p1x - p0x) * (p2y - p0y) - (p2x - p0x) * (p1y - p0y)


def _inside(box, c, s, px, py):
    """corner_in_box: the point turned back by the box's heading, 1e-5 margin; px, py (n, 4)"""
    margin = F(1e-5)
    cx, cy = ((box[:, 0] + box[:, 2]) / F(2))[:, None], ((box[:, 1] + box[:, 3]) / F(2))[:, None]
    c, ns = c[:, None], (-s)[:, None]
    rx = ((px - cx) * c + (py - cy) * ns) + cx
    ry = ((-(px - cx)) * ns + (py - cy) * c) + cy
    return ((rx > (box[:, 0] - margin)[:, None]) & (rx < (box[:, 2] + margin)[:, None]) &
            (ry > (box[:, 1] - margin)[:, None]) & (ry < (box[:, 3] + margin)[:, None]))


def vertex_count(a, b):
    """f32 numpy restatement of the counting part of rbox_overlap_in for the PAIRS (a[i], b[i]), (n, 5) BEV boxes each: the strictly
    proper edge crossings plus the corners of either box inside the other with the 1e-5 margin -> (crossings (n,), corners (n,))"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    with np.errstate(all="ignore"):
        ca, sa = _trig(a[:, 4])
        cb, sb = _trig(b[:, 4])
        ax, ay = _corners(a, ca, sa)
        bx, by = _corners(b, cb, sb)
        crossings = np.zeros(len(a), np.int64)
        for i in range(4):
            p0x, p0y, p1x, p1y = ax[:, i], ay[:, i], ax[:, (i + 1) % 4], ay[:, (i + 1) % 4]
            for j in range(4):
                q0x, q0y, q1x, q1y = bx[:, j], by[:, j], bx[:, (j + 1) % 4], by[:, (j + 1) % 4]
                rect = ((np.minimum(p0x, p1x) <= np.maximum(q0x, q1x)) & (np.minimum(q0x, q1x) <= np.maximum(p0x, p1x)) &
                        (np.minimum(p0y, p1y) <= np.maximum(q0y, q1y)) & (np.minimum(q0y, q1y) <= np.maximum(p0y, p1y)))
                s1 = _cross3(q0x, q0y, p1x, p1y, p0x, p0y)
                s2 = _cross3(p1x, p1y, q1x, q1y, p0x, p0y)
                s3 = _cross3(p0x, p0y, q1x, q1y, q0x, q0y)
                s4 = _cross3(q1x, q1y, p1x, p1y, q0x, q0y)
                crossings += rect & (s1 * s2 > 0) & (s3 * s4 > 0)
        corners = _inside(a, ca, sa, bx, by).sum(1) + _inside(b, cb, sb, ax, ay).sum(1)
    return crossings, corners.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ turned family
def turned_pairs():
    """The same rectangle turned about its centre by k f32(pi/2), k = 1, 2, 3, and squares by f32(pi/4), at 12 centres out to 70 m
    -> (a3, b3) (n, 7) f32.  The first box has heading 0 or an odd one; the overlap is the box itself (k = 2), its central square
    (k = 1, 3) or the octagon (squares, pi/4)."""
    centres = [(0.0, 0.0), (0.5, 1.25), (-3.3, 7.1), (10.0, 20.0), (-20.7, 33.3), (35.2, 5.9), (-39.9, 49.1), (17.3, 58.6), (1.1, 69.7),
               (-40.0, 70.0), (40.0, 64.3), (-12.6, 44.4)]
    rects = [(3.9, 1.6), (4.4, 1.9), (0.8, 0.6), (1.76, 0.6)]
    squares = [(2.0, 2.0), (1.7, 1.7)]
    half, quarter = np.float64(F(np.pi / 2)), np.float64(F(np.pi / 4))
    a, b = [], []
    for k, (cx, cz) in enumerate(centres):
        base = 0.0 if k % 2 == 0 else 0.37 * k - 2.0
        for l, w in rects + squares:
            for turn in (1, 2, 3):
                a.append((cx, cz, l, w, base)); b.append((cx, cz, l, w, base + turn * half))
        for l, w in squares:
            a.append((cx, cz, l, w, base)); b.append((cx, cz, l, w, base + quarter))
    a, b = np.array(a), np.array(b)
    return to_3d(*a.T), to_3d(*b.T)


# --------------------------------------------------------------------------------------------------------------------- tip family
def far_apart(a, b):
    """numpy restatement of the three lines of rbox_far_apart (f32, one rounding per operation) for the pairs (a[i], b[i]) (n, 5)
    -> (far (n,) bool, centre distance / reach (n,) f64)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    h = F(0.5)
    ax, ay, bx, by = (a[:, 0] + a[:, 2]) * h, (a[:, 1] + a[:, 3]) * h, (b[:, 0] + b[:, 2]) * h, (b[:, 1] + b[:, 3]) * h
    ra = h * np.sqrt((a[:, 2] - a[:, 0]) * (a[:, 2] - a[:, 0]) + (a[:, 3] - a[:, 1]) * (a[:, 3] - a[:, 1]))
    rb = h * np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 2] - b[:, 0]) + (b[:, 3] - b[:, 1]) * (b[:, 3] - b[:, 1]))
    reach = (ra + rb) * F(1.001) + F(0.01)
    dx, dy = ax - bx, ay - by
    d2 = dx * dx + dy * dy
    return d2 > reach * reach, np.sqrt(d2.astype(np.float64)) / reach.astype(np.float64)


def _along(ry):
    """direction of a box's long side"""
    return np.stack([np.cos(ry), -np.sin(ry)], 1)


def tip_partners(rng, first):
    """first (n, 5) f64 rows [cx, cz, l, w, ry] -> (partners (n, 5) f64, kind (n,)): long thin boxes (l in [10, 20], w in [0.1, 0.3])
    whose centre distance is (1 + u) x reach, reach = (ra + rb) * 1.001 + 0.01 with the half diagonals ra, rb, u uniform in +-2 %.
    kind 0: inside the reach, the tips cross (a point on both long axes lies inside both boxes); kind 1: inside the reach,
    parallel and 0.5 m aside (disjoint); kind 2: beyond the reach.  A crossing needs (la + lb) / 2 - distance > 2 cm of slack: a row
    drawn as kind 0 without it becomes kind 1."""
    first = np.asarray(first, np.float64)
    n = len(first)
    ca, la, wa, rya = first[:, 0:2], first[:, 2], first[:, 3], first[:, 4]
    lb, wb = rng.uniform(10, 20, n), rng.uniform(0.1, 0.3, n)
    reach = 0.5 * (np.hypot(la, wa) + np.hypot(lb, wb)) * 1.001 + 0.01
    kind = np.array([0, 1, 2, 2])[np.arange(n) % 4]                      # half inside the reach (crossing / aside in turn), half beyond
    u =rng.uniform(0.001, 0.02, n) * np.where(kind == 2, 1.0, -1.0)
    d = reach * (1 + u)
    slack = (la + lb) / 2 - d
    kind = np.where((kind == 0) & (slack < 0.02), 1, kind)
    ea, na = _along(rya), np.stack([np.sin(rya), np.cos(rya)], 1)
    cb, ryb = np.zeros((n, 2)), np.zeros(n)
    # kind 0: T = ca + p ea lies delta inside a's end, cb = T + q eb puts b's end delta beyond T; the angle between the axes gives |cb - ca| = d
    delta = 0.5 * np.clip(slack, 0.02, None) * rng.uniform(0.3, 1.0, n)
    p, q = la / 2 - delta, lb / 2 - delta
    phi = np.arccos(np.clip((d * d - p * p - q * q) / (2 * p * q), -1, 1)) * rng.choice([-1.0, 1.0], n)
    cross = kind == 0
    ryb[cross] = (rya + phi)[cross]
    cb[cross] = (ca + p[:, None] * ea + q[:, None] * _along(rya + phi))[cross]
    # kind 1: parallel, 0.5 m aside
    side = rng.choice([-1.0, 1.0], n)
    aside = kind == 1
    ryb[aside] = rya[aside]
    cb[aside] = (ca + np.sqrt(d * d - 0.25)[:, None] * ea * side[:, None] + 0.5 * na)[aside]
    # kind 2: beyond the reach, roughly ahead of a's tip, any nearby heading
    psi, turn = rng.uniform(-0.2, 0.2, n), rng.uniform(-0.3, 0.3, n)
    out = kind == 2
    ryb[out] = (rya + turn)[out]
    cb[out] = (ca + d[:, None] * _along(rya + psi))[out]
    return np.concatenate([cb, lb[:, None], wb[:, None], ryb[:, None]], 1), kind


def tip_pairs(seed, n):
    """-> (a3, b3 (n, 7) f32, kind (n,)): see tip_partners; the first boxes are long and thin as well, anywhere in the scene"""
    rng = np.random.default_rng(seed)
    first = np.stack([rng.uniform(-30, 30, n), rng.uniform(10, 60, n), rng.uniform(10, 20, n), rng.uniform(0.1, 0.3, n),
                      rng.uniform(-np.pi, np.pi, n)], 1)
    second, kind = tip_partners(rng, first)
    return to_3d(*first.T), to_3d(*second.T), kind


# ---------------------------------------------------------------------------------------------------------------------- NMS scenes
def clustered_scene(seed, clusters, copies, n=None):
    """``clusters`` car-sized boxes on a jittered grid (3.2 m x 2.2 m: neighbours overlap), each followed by ``copies`` - 1
    near-coincident copies of itself (the recipe of near_coincident_pairs).  Rows in score order: every cluster's first member in a
    random order of the clusters, then the second members, ...; scores strictly descending (equal inside a cluster up to the row
    index: score = base - 1e-4 row).  ``n`` keeps the first n rows.
    -> (bev (n, 5) f32, boxes3d (n, 7) f32, cluster (n,) int, scores (n,) f32)"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(clusters)))
    k = np.arange(clusters)
    cx = -0.5 * 3.2 * side + 3.2 * (k % side) + rng.uniform(-1.0, 1.0, clusters)
    cz = 5.0 + 2.2 * (k // side) + rng.uniform(-0.7, 0.7, clusters)
    l, w = rng.uniform(3.0, 5.0, clusters), rng.uniform(1.4, 2.2, clusters)
    ry = rng.uniform(-np.pi, np.pi, clusters)
    ry[0::2] = 0.0
    near = k[2::4]                                                         # every fourth cluster sits on its predecessor: IoU 0.3 .. 0.95
    cx[near] = cx[near - 1] + rng.choice([-1.0, 1.0], len(near)) * rng.uniform(0.05, 0.9, len(near))
    cz[near] = cz[near - 1] + rng.choice([-1.0, 1.0], len(near)) * rng.uniform(0.02, 0.4, len(near))
    l[near], w[near] = l[near - 1] * rng.uniform(0.95, 1.05, len(near)), w[near - 1] * rng.uniform(0.95, 1.05, len(near))
    ry[near] = ry[near - 1] + rng.uniform(-0.08, 0.08, len(near))
    rows, ids = [], []
    for c in range(copies):
        order = rng.permutation(clusters)
        if c == 0:
            x, z, r = cx, cz, ry
        else:
            x, z, r = nearly(rng, cx, cz, ry)
        rows.append(to_3d(x[order], z[order], l[order], w[order], r[order]))
        ids.append(order)
    b3, ids = np.concatenate(rows, 0), np.concatenate(ids, 0)
    if n is not None:
        assert n <= len(b3)
        b3, ids = b3[:n], ids[:n]
    scores = (F(4.0) - F(1e-4) * np.arange(len(b3))).astype(F)
    return to_bev(b3), b3, ids, scores


# what tests/test_gpu_box_pairs.py runs its NMS forms on: (seed, clusters, copies, rows).  tests/test_box_pairs.py asserts for each that
# no pair of boxes from different clusters has an oracle IoU within BAND of a threshold in NMS_THRESHOLDS (the seeds were chosen so).
NMS_SCENES = {
    "nms_gpu": [(101, 17, 4, 65), (102, 33, 4, 129), (103, 500, 4, 2000)],
    "dense7": [(111, 4, 2, 7), (112, 4, 2, 7), (113, 4, 2, 7), (114, 4, 2, 7), (115, 4, 2, 7), (116, 4, 2, 7)],
    "dense65": [(121, 17, 4, 65), (122, 17, 4, 65), (123, 17, 4, 65), (124, 17, 4, 65), (125, 17, 4, 65), (126, 17, 4, 65)],
    "dense128": [(131, 32, 4, 128), (132, 32, 4, 128), (133, 32, 4, 128), (134, 32, 4, 128), (135, 32, 4, 128), (136, 32, 4, 128)],
    "general300": [(141, 75, 4, 300), (142, 75, 4, 300), (143, 75, 4, 300), (144, 75, 4, 300)],
    "general3000": [(151, 750, 4, 3000), (152, 750, 4, 3000), (153, 750, 4, 3000)],
}


def cross_cluster_band(iou, cluster):
    """how many pairs of boxes from DIFFERENT clusters have an IoU within BAND of a threshold; iou (n, n) from the oracle"""
    other = cluster[:, None] != cluster[None, :]
    near = np.zeros_like(other)
    for t in NMS_THRESHOLDS:
        near |= np.abs(iou.astype(np.float64) - t) <= BAND
    return int((near & other).sum())
