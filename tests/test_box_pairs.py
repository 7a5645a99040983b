"""What the rotated-overlap ALGORITHM (oracle.boxes_overlap_bev, the reference's operations one for one) does on the families of
tests/box_pairs.py, pinned on the CPU so that a later "fix" to it shows up, and the conditions under which the GPU tests of
tests/test_gpu_box_pairs.py are decidable: the families reach the polygon states they are meant to reach, and no NMS decision between
clusters sits near a threshold."""
import numpy as np
import pytest

import box_pairs as BP

U32 = np.uint32
LO = float(np.nextafter(np.float32(0.5), np.float32(0)))          # the largest f32 below 0.5


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(U32)


def pairwise(f, a, b):
    """f evaluated on the pairs (a[i], b[i]) only"""
    return np.array([f(a[i:i + 1], b[i:i + 1])[0, 0] for i in range(len(a))], dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------- exact family
def test_exact_family_equals_the_closed_form_bit_for_bit(oracle):
    """Headings 0, dyadic coordinates: every operation is exact in f32, so the algorithm must return the axis-aligned min/max area
    itself (touching: exactly 0), in both argument orders, on the crafted pairs and on everything against everything."""
    for n in (None, 256):
        a, b, want, names = BP.exact_pairs(n)
        for x, y in ((a, b), (b, a)):
            assert np.array_equal(bits(oracle.boxes_overlap_bev(x, y)), bits(BP.closed_form_overlap(x, y)))
            assert np.array_equal(bits(oracle.boxes_iou_bev(x, y)), bits(BP.closed_form_iou(x, y)))
    a, b, want, names = BP.exact_pairs()
    got = dict(zip(names, want[:len(BP.EXACT_CONFIGS)]))
    assert got["identical"] == 8 and got["plus"] == 4 and got["nested_two_shared_edges"] == 4 and got["t_junction_overlapping"] == 1
    assert all(got[k] == 0 for k in names if k.startswith("touch")) and got["t_junction_touching"] == 0
    assert np.array_equal(want[len(BP.EXACT_CONFIGS):], want[:len(BP.EXACT_CONFIGS)])          # the translated repeat
    assert (BP.closed_form_overlap(*BP.exact_pairs(256)[:2]) > 0).mean() > 0.03


def test_exact_family_vertex_states():
    a, b, _, names = BP.exact_pairs()
    cr, co = BP.vertex_count(a, b)
    state = {n: (int(x), int(y)) for n, x, y in zip(names[:len(BP.EXACT_CONFIGS)], cr, co)}
    assert state["identical"] == (0, 8) and state["plus"] == (4, 0) and state["touch_whole_edge"] == (0, 4)
    assert state["touch_part_of_edge"] == (0, 2) and state["touch_corner"] == (0, 2) and state["nested_no_shared_edge"] == (0, 4)


def test_nested_pair_sits_exactly_on_the_nms_threshold(oracle):
    """2x2 in 4x2: IoU = 4 / (8 + 4 - 4) = 0.5 exactly.  The NMS drops on IoU > threshold, strictly: both boxes stay at 0.5, the second
    goes at the next f32 below; the axis-aligned IoU is the same number for heading 0."""
    a, b = np.array([BP.NESTED_PAIR[0]], np.float32), np.array([BP.NESTED_PAIR[1]], np.float32)
    assert oracle.boxes_iou_bev(a, b)[0, 0] == np.float32(0.5) and oracle.boxes_iou_bev(b, a)[0, 0] == np.float32(0.5)
    assert np.float32(LO) < np.float32(0.5) and np.float32(LO) == np.nextafter(np.float32(0.5), np.float32(0))
    for pairs in (1, 64, 150):
        boxes, keep_at, keep_below = BP.threshold_scene(pairs)
        for nms in (oracle.nms, oracle.nms_normal):
            assert np.array_equal(nms(boxes, 0.5), keep_at)
            assert np.array_equal(nms(boxes, LO), keep_below)


# -------------------------------------------------------------------------------------------------------- near-coincident family
# shape -> the smallest admissible shares (>= 9 vertices, == 16 vertices, oracle IoU > 1).  Measured with seed 1, 3000 pairs:
#   car        42.9 % / 7.3 % / 40.9 %   (bounds: the issue's 35 % / 2 % / 25 %)
#   pedestrian 33.3 % / 1.1 % / 44.1 %   (bounds 25 % / 0.5 % / 25 %: small boxes meet the 1e-5 m margin with a larger part of their sides,
#   cyclist    36.3 % / 2.0 % / 44.1 %    bounds 25 % / 1 % / 25 %    but fewer of their shifts are above the f32 spacing of the centre)
SHARES = {"car": (0.35, 0.02, 0.25), "pedestrian": (0.25, 0.005, 0.25), "cyclist": (0.25, 0.01, 0.25)}


@pytest.mark.parametrize("shape", list(SHARES))
def test_near_coincident_family_reaches_the_large_polygons(oracle, shape):
    a3, b3 = BP.near_coincident_pairs(1, 3000, shape)
    assert np.array_equal(a3[:, 3:6], b3[:, 3:6]) and (a3[0::2, 6] == 0).all() and (a3[1::2, 6] != 0).all()
    assert np.abs(a3[:, [0, 2]].astype(np.float64) - b3[:, [0, 2]]).max() < 6e-5 and np.abs(a3[:, 6].astype(np.float64) - b3[:, 6]).max() < 4e-6
    a, b = BP.to_bev(a3), BP.to_bev(b3)
    crossings, corners = BP.vertex_count(a, b)
    v = crossings + corners
    iou = pairwise(oracle.boxes_iou_bev, a, b)
    big, full, above = (v >= 9).mean(), (v == 16).mean(), (iou > 1).mean()
    print("%s: >= 9 vertices %.3f, 16 vertices %.3f, largest %d, IoU > 1 %.3f, IoU in [%.7f, %.7f]" % (shape, big, full, v.max(), above, iou.min(), iou.max()))
    lo_big, lo_full, lo_above = SHARES[shape]
    assert big >= lo_big and full >= lo_full and above >= lo_above
    assert v.max() <= 24 and crossings.max() <= 16 and corners.max() <= 8
    assert ((crossings == 8) & (corners == 8)).sum() == (v == 16).sum()          # 16 = all 8 corners within the margin + all 8 proper crossings
    assert iou.min() > 0.999 and iou.max() < 1.0001


# ------------------------------------------------------------------------------------------ the algorithm against a plain f64 clip
def clip_area_f64(a, b):
    """Sutherland-Hodgman in f64: box a (corners turned as the reference turns them) clipped by the four edges of box b -> area"""
    def corners(v):
        v = np.asarray(v, np.float64)
        cx, cy, c, s = (v[0] + v[2]) / 2, (v[1] + v[3]) / 2, np.cos(v[4]), np.sin(v[4])
        p = np.array([[v[0], v[1]], [v[2], v[1]], [v[2], v[3]], [v[0], v[3]]]) - [cx, cy]
        return np.stack([p[:, 0] * c + p[:, 1] * s + cx, -p[:, 0] * s + p[:, 1] * c + cy], 1)
    poly, clip = list(corners(a)), corners(b)
    e = clip[1] - clip[0], clip[2] - clip[1]
    if e[0][0] * e[1][1] - e[0][1] * e[1][0] < 0:
        clip = clip[::-1]
    for k in range(4):
        e0, e1 = clip[k], clip[(k + 1) % 4]
        side = [(e1[0] - e0[0]) * (p[1] - e0[1]) - (e1[1] - e0[1]) * (p[0] - e0[0]) for p in poly]
        out = []
        for i, p in enumerate(poly):
            q, sp, sq = poly[(i + 1) % len(poly)], side[i], side[(i + 1) % len(poly)]
            if sp >= 0:
                out.append(p)
            if (sp > 0 > sq) or (sp < 0 < sq):
                out.append(p + (q - p) * (sp / (sp - sq)))
        poly = out
        if not poly:
            return 0.0
    x, y = np.array(poly)[:, 0], np.array(poly)[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def family(name):
    if name.startswith("near_"):
        a3, b3 = BP.near_coincident_pairs(1, 3000, name[5:])
    elif name == "turned":
        a3, b3 = BP.turned_pairs()
    else:
        a3, b3, _ = BP.tip_pairs(5, 400)
    return BP.to_bev(a3), BP.to_bev(b3)


# family -> (largest |oracle - f64 clip| measured on this family, in m^2; the bound is twice that)
MEASURED = {"near_car": 8.553e-5, "near_pedestrian": 1.82e-5, "near_cyclist": 3.266e-5, "turned": 2.114e-5, "tip": 8.123e-7}


@pytest.mark.parametrize("name", list(MEASURED))
def test_oracle_against_f64_convex_clip(oracle, name):
    """The reference's f32 algorithm (crossings + corners with a margin, angular bubble sort, shoelace) against a plain f64
    Sutherland-Hodgman clip of the same two rectangles.  This is about the ALGORITHM, not the device.  Measured largest absolute
    deviation of the overlap area and the bound (2 x measured), in m^2:
        near_car (3000 pairs) 8.553e-5 / 1.711e-4    near_pedestrian 1.82e-5 / 3.64e-5    near_cyclist 3.266e-5 / 6.532e-5
        turned (240 pairs) 2.114e-5 / 4.228e-5    tip (400 pairs) 8.123e-7 / 1.625e-6
    (against the box's own area the car family's overlap is off by up to 3.8e-5 relative)"""
    a, b = family(name)
    got = pairwise(oracle.boxes_overlap_bev, a, b).astype(np.float64)
    want = np.array([clip_area_f64(a[i], b[i]) for i in range(len(a))])
    worst = float(np.abs(got - want).max())
    print("%s: %d pairs, largest |oracle - f64 clip| = %.4g m^2 (bound %.4g)" % (name, len(a), worst, 2 * MEASURED[name]))
    assert worst <= 2 * MEASURED[name]
    assert (want > 0).any()


# --------------------------------------------------------------------------------------------------------------------- tip family
def test_tip_family_lies_on_both_sides_of_the_reach(oracle):
    """centre distance within 2 % of the reach on both sides; inside the reach about half of the pairs really overlap; and whatever
    rbox_far_apart prunes has overlap EXACTLY 0 in the algorithm (no vertex), which is what makes the pruning exact"""
    a3, b3, kind = BP.tip_pairs(5, 400)
    assert ((a3[:, 5] >= 10) & (a3[:, 5] <= 20) & (a3[:, 4] >= 0.1) & (a3[:, 4] <= 0.3)).all()
    assert ((b3[:, 5] >= 10) & (b3[:, 5] <= 20) & (b3[:, 4] >= 0.1) & (b3[:, 4] <= 0.3)).all()
    a, b = BP.to_bev(a3), BP.to_bev(b3)
    far, ratio = BP.far_apart(a, b)
    assert 0.979 < ratio.min() < 0.985 and 1.015 < ratio.max() < 1.021
    assert far.sum() == 200 and np.array_equal(far, kind == 2) and np.array_equal(far, BP.far_apart(b, a)[0])
    ov = pairwise(oracle.boxes_overlap_bev, a, b)
    print("inside the reach: %d crossing (overlap > 0), %d aside; beyond: %d; smallest positive overlap %.3g m^2" %
          ((kind == 0).sum(), (kind == 1).sum(), far.sum(), ov[ov > 0].min()))
    assert 70 <= (kind == 0).sum() <= 100 and (ov[kind == 0] > 1e-3).all()
    assert (ov[kind != 0] == 0).all()


# -------------------------------------------------------------------------------------------------------------------- NMS scenes
@pytest.mark.parametrize("group", list(BP.NMS_SCENES))
def test_clustered_scenes_have_no_decision_near_a_threshold(oracle, group):
    """A condition on the INPUT of the GPU NMS tests, not a tolerance: no pair of boxes from different clusters has an oracle IoU within
    1e-5 of a threshold of BP.NMS_THRESHOLDS (the seeds were chosen so), and inside a cluster every IoU is within 5e-4 of 1.  The device's IoU is within 1e-6 of the
    oracle's, so its keep list has to be the oracle's."""
    for seed, clusters, copies, n in BP.NMS_SCENES[group]:
        bev, b3, ids, scores = BP.clustered_scene(seed, clusters, copies, n)
        assert bev.shape == (n, 5) and np.array_equal(bev, BP.to_bev(b3)) and (np.diff(scores) < 0).all()
        iou = oracle.boxes_iou_bev(bev, bev)
        assert BP.cross_cluster_band(iou, ids) == 0, (group, seed)
        same = ids[:, None] == ids[None, :]
        assert 0.9995 < iou[same].min() and iou[same].max() < 1.0005 and iou[~same].max() < 0.99
        kept = [len(oracle.nms(bev, t)) for t in BP.NMS_THRESHOLDS]
        assert kept[0] < kept[1] < kept[2] or n <= 7, kept          # every threshold decides something between clusters
        assert kept[2] <= kept[3] == len(set(ids.tolist())) and kept[4] == n
