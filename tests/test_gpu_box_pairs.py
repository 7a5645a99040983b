"""-m gpu: the five consumers of rbox_overlap_in (csrc/rbox_iou.hpp) on the families of tests/box_pairs.py -- exactly touching and
nested boxes in exact arithmetic, near-coincident boxes (clipped polygons of 9..16 vertices, private and LDS form), quarter turns,
long thin boxes around the rbox_far_apart reach, NMS scenes of near-coincident clusters.

Every figure asserted here is the exact-arithmetic argument (bitwise), a tolerance an existing test of the same kernel uses (1e-5 on
overlaps, 1e-6 on IoUs: test_overlap_and_iou_bev; 99 % bitwise: test_rotate_iou_kernel_vs_reference_python_fixture; 1e-5 on final
boxes; 1e-4 on the target stage's floats), or a condition on the INPUT that tests/test_box_pairs.py asserts on the CPU (no NMS
decision between clusters within 1e-5 of a threshold)."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import box_pairs as BP  # noqa: E402
from conftest import pkg  # noqa: E402
from helpers import bev_boxes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO = float(np.nextafter(np.float32(0.5), np.float32(0)))          # the largest f32 below 0.5


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def device_matrices(ext, a, b):
    ov = torch.full((len(a), len(b)), -7.0, device=DEV)
    iou = torch.full((len(a), len(b)), -7.0, device=DEV)
    ext.iou3d.boxes_overlap_bev_gpu(T(a), T(b), ov)
    ext.iou3d.boxes_iou_bev_gpu(T(a), T(b), iou)
    return ov.cpu().numpy(), iou.cpu().numpy()


# ------------------------------------------------------------------------------------------------------- (a) matrix entry points
def test_exact_family_is_bitwise_the_closed_form(ext, oracle):
    """256 x 256: the crafted pairs on the diagonal, everything against everything beside it, both argument orders.  Exact
    arithmetic: device == oracle == closed form bit for bit, and == the reference's own kernel where oracle/_ref is built
    (contraction cannot move an exact result)."""
    from oracle import ref_gpu
    a, b, want, _ = BP.exact_pairs(256)
    print("oracle/_ref available for the bitwise check against the reference kernel: %s" % ref_gpu.available())
    for x, y in ((a, b), (b, a)):
        ov, iou = device_matrices(ext, x, y)
        assert np.array_equal(bits(ov), bits(oracle.boxes_overlap_bev(x, y)))
        assert np.array_equal(bits(iou), bits(oracle.boxes_iou_bev(x, y)))
        assert np.array_equal(bits(ov), bits(BP.closed_form_overlap(x, y)))
        assert np.array_equal(bits(iou), bits(BP.closed_form_iou(x, y)))
        if ref_gpu.available():
            assert np.array_equal(bits(ref_gpu.boxes_overlap_bev(T(x), T(y)).cpu().numpy()), bits(ov))
            assert np.array_equal(bits(ref_gpu.boxes_iou_bev(T(x), T(y)).cpu().numpy()), bits(iou))
    assert np.array_equal(np.diagonal(ov), want)          # (b, a) order: the overlap is symmetric


def matrix_family(name):
    """-> (a, b): BEV boxes whose pairs (a[i], b[i]) are the family's; the other entries of the matrix are whatever they are"""
    if name.startswith("near_"):
        a3, b3 = BP.near_coincident_pairs(1, 1024, name[5:])
    elif name == "turned":
        a3, b3 = BP.turned_pairs()
    else:
        a3, b3, _ = BP.tip_pairs(5, 400)
    return BP.to_bev(a3), BP.to_bev(b3)


@pytest.mark.parametrize("name", ["near_car", "near_pedestrian", "near_cyclist", "turned", "tip"])
def test_families_against_the_oracle(ext, oracle, name):
    """Tolerances of test_overlap_and_iou_bev (1e-5 absolute on the overlap, 1e-6 on the IoU) and at least 99 % of the entries bit
    for bit -- over the whole matrix and over the family's own pairs on its diagonal: a nudge of one heading by 1 f32 ulp moves 2-3 %
    of the near-coincident pairs by more than 1e-5, so a slip in the f32 trig contract (cos / sin / atan2 = the f64 value rounded to
    f32) cannot hide here."""
    a, b = matrix_family(name)
    ov, iou = device_matrices(ext, a, b)
    want_ov, want_iou = oracle.boxes_overlap_bev(a, b), oracle.boxes_iou_bev(a, b)
    same_ov, same_iou = bits(ov) == bits(want_ov), bits(iou) == bits(want_iou)
    d_ov, d_iou = np.abs(ov.astype(np.float64) - want_ov), np.abs(iou.astype(np.float64) - want_iou)
    k = np.arange(len(a))
    print("%s (%d x %d): overlap bitwise %.5f (pairs %.5f) max |d| %.3g; IoU bitwise %.5f (pairs %.5f) max |d| %.3g" %
          (name, len(a), len(b), same_ov.mean(), same_ov[k, k].mean(), d_ov.max(), same_iou.mean(), same_iou[k, k].mean(), d_iou.max()))
    np.testing.assert_allclose(ov, want_ov, rtol=0, atol=1e-5)
    np.testing.assert_allclose(iou, want_iou, rtol=0, atol=1e-6)
    assert same_ov.mean() >= 0.99 and same_iou.mean() >= 0.99
    assert same_ov[k, k].mean() >= 0.99 and same_iou[k, k].mean() >= 0.99


def degenerate_block():
    rng = np.random.default_rng(77)
    a = bev_boxes(rng, 32, spread=4.0)
    a[1, 2] = a[1, 0]                                   # zero width
    a[2, 2:4] = a[2, 0:2]                               # a point
    a[3, [0, 2]] = a[3, [2, 0]]                         # negative extent along x
    a[4, [1, 3]] = a[4, [3, 1]]; a[4, [0, 2]] = a[4, [2, 0]]          # ... along both
    a[5, 0] = np.nan
    a[6, 4] = np.nan
    a[7, 2] = np.inf
    a[8, 1] = -np.inf
    a[9, 4] = np.inf
    a[10, :4] = [-np.inf, -np.inf, np.inf, np.inf]
    a[11] = a[12]; a[11, 2] = a[11, 0]                  # zero width inside another box
    b = np.concatenate([a[:16], bev_boxes(rng, 16, spread=4.0)], 0)
    b[20] = a[3]; b[21] = a[1]
    return a, b


def test_degenerate_rows_equal_the_oracle(ext, oracle):
    """zero-area, negative-extent, NaN and infinite rows, here only (every loop of the function is bounded by the vertex count):
    the device equals the oracle, NaN positions included"""
    a, b = degenerate_block()
    with np.errstate(all="ignore"):
        want_ov, want_iou = oracle.boxes_overlap_bev(a, b), oracle.boxes_iou_bev(a, b)
    ov, iou = device_matrices(ext, a, b)
    print("non-finite entries: oracle overlap %d, IoU %d; device overlap %d, IoU %d" %
          ((~np.isfinite(want_ov)).sum(), (~np.isfinite(want_iou)).sum(), (~np.isfinite(ov)).sum(), (~np.isfinite(iou)).sum()))
    assert np.array_equal(np.isnan(ov), np.isnan(want_ov)) and np.array_equal(np.isnan(iou), np.isnan(want_iou))
    assert np.array_equal(np.isinf(ov), np.isinf(want_ov)) and np.array_equal(np.isinf(iou), np.isinf(want_iou))
    ok = np.isfinite(want_ov)
    np.testing.assert_allclose(ov[ok], want_ov[ok], rtol=0, atol=1e-5)
    # a box of negative extent has a negative "area": the union clamps at 1e-8 and the IoU is the overlap times 1e8, so an absolute
    # tolerance only makes sense where the oracle's IoU is a ratio (<= 1.5).  Everywhere, the device's IoU must be iou3d_kernel.cu:214-221
    # applied to the device's own overlap, bit for bit (f32 operations, fmax passing a NaN by)
    ratio = np.isfinite(want_iou) & (np.abs(want_iou) <= 1.5)
    np.testing.assert_allclose(iou[ratio], want_iou[ratio], rtol=0, atol=1e-6)
    assert (~ratio).sum() >= 5 and (want_ov[12:, 12:16] > 0).any()
    with np.errstate(all="ignore"):
        sa = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None]
        sb = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
        formula = ov / np.fmax((sa + sb) - ov, np.float32(1e-8))
    assert formula.dtype == np.float32 and np.array_equal(bits(formula), bits(iou))


# --------------------------------------------------------------------------------------------- (b) rotated NMS through every form
_WANT = {}


def want_keep(oracle, spec, count, thresh, rotated=True):
    key = (spec, count, thresh, rotated)
    if key not in _WANT:
        boxes = BP.clustered_scene(*spec)[0][:count]
        _WANT[key] = (oracle.nms if rotated else oracle.nms_normal)(boxes, thresh)
    return _WANT[key]


def run_device(ext, boxes, counts, thresh, rotated, K):
    P = boxes.shape[0]
    keep = torch.full((P, K), -9, dtype=torch.int32, device=DEV)
    num = torch.full((P,), -9, dtype=torch.int32, device=DEV)
    ext.iou3d.nms_device(T(boxes), T(np.asarray(counts, np.int32)), float(thresh), rotated, K, keep, num)
    return keep.cpu().numpy(), num.cpu().numpy()


def check_device(keep, num, wants, K):
    for p, want in enumerate(wants):
        want = want[:K]
        assert num[p] == len(want), (p, num[p], len(want))
        assert np.array_equal(keep[p, :num[p]], want), p
        assert (keep[p, num[p]:] == -1).all()


@pytest.mark.parametrize("thresh", BP.NMS_THRESHOLDS)
def test_nms_gpu_on_clustered_scenes(ext, oracle, thresh):
    for spec in BP.NMS_SCENES["nms_gpu"]:
        boxes = BP.clustered_scene(*spec)[0]
        keep = torch.zeros(len(boxes), dtype=torch.int64)
        k = ext.iou3d.nms_gpu(T(boxes), keep, thresh)
        want = want_keep(oracle, spec, len(boxes), thresh)
        assert k == len(want) and np.array_equal(keep[:k].numpy(), want), spec


@pytest.mark.parametrize("thresh", BP.NMS_THRESHOLDS)
@pytest.mark.parametrize("nmax,quota", [(7, 2), (65, 5), (128, 10)])
def test_nms_device_dense_form_on_clustered_scenes(ext, oracle, nmax, quota, thresh):
    """n <= 128: the all-pairs mask kernel keeps its polygon in LDS (PolyLds, slots 8..15 of base[(3 k + q) * stride]); ragged counts
    including 0 and 1, and a keep quota below the answer"""
    specs = BP.NMS_SCENES["dense%d" % nmax]
    counts = [nmax, nmax - 1, 0, 1, nmax // 2, nmax]
    boxes = np.stack([BP.clustered_scene(*s)[0] for s in specs], 0)
    wants = [want_keep(oracle, s, c, thresh) for s, c in zip(specs, counts)]
    assert len(wants[0]) > quota
    for K in (nmax, quota):
        check_device(*run_device(ext, boxes, counts, thresh, True, K), wants, K)


@pytest.mark.parametrize("thresh", BP.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", [300, 3000])
def test_nms_device_general_and_quota_on_clustered_scenes(ext, oracle, n, thresh):
    """n > 128: one workgroup per problem walks 64-row blocks; K = 70 is a quota below most answers, K = 300 is not"""
    specs = BP.NMS_SCENES["general%d" % n]
    counts = [n, n - 1, n // 2, 1][:len(specs)]
    boxes = np.stack([BP.clustered_scene(*s)[0] for s in specs], 0)
    wants = [want_keep(oracle, s, c, thresh) for s, c in zip(specs, counts)]
    for K in (70, 300):
        check_device(*run_device(ext, boxes, counts, thresh, True, K), wants, K)


@pytest.mark.parametrize("thresh", [0.5, LO])
def test_every_nms_form_decides_the_exact_threshold(ext, oracle, thresh):
    """Copies of the nested 2x2-in-4x2 pair: IoU exactly 0.5 (rotated and axis-aligned alike, heading 0) and exactly 0 between pairs.
    The test is IoU > threshold, strictly: at 0.5 every box stays, at the next f32 below the second box of every pair goes."""
    for pairs in (150, 64, 4):
        boxes, keep_at, keep_below = BP.threshold_scene(pairs)
        want = keep_at if thresh == 0.5 else keep_below
        n = len(boxes)
        assert np.array_equal(oracle.nms(boxes, thresh), want) and np.array_equal(oracle.nms_normal(boxes, thresh), want)
        for fn in (ext.iou3d.nms_gpu, ext.iou3d.nms_normal_gpu):
            keep = torch.zeros(n, dtype=torch.int64)
            k = fn(T(boxes), keep, thresh)
            assert k == len(want) and np.array_equal(keep[:k].numpy(), want), (pairs, fn)
        # pairs = 150: the general kernels (rotated; axis-aligned with the quota form at K = 70); 64 and 4 (cut to 7 rows): the dense form
        rows = 7 if pairs == 4 else n
        want_rows = want[want < rows]
        for rotated in (True, False):
            for K in (70, 300) if pairs == 150 else (rows, 3):
                check_device(*run_device(ext, boxes[None, :rows], [rows], thresh, rotated, K), [want_rows], K)


# ----------------------------------------------------------------------------------------------------- (c) the fused final stage
CH = 4 * 6 + 1 + 2 * 9 + 3


def zero_row_decode(cfg):
    """what a zero regression row decodes to against the RoI (0, 0, 0, ., ., ., 0): (x, y, z) offset in the RoI's frame and heading
    offset, from the package's own decode on the CPU"""
    R = cfg.RCNN
    anchor = torch.tensor([float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], np.float32)])
    box = pkg("bbox_transform").decode_bbox_target(torch.zeros(1, 7), torch.zeros(1, CH), anchor_size=anchor, loc_scope=R.LOC_SCOPE,
                                                    loc_bin_size=R.LOC_BIN_SIZE, num_head_bin=R.NUM_HEAD_BIN, get_xz_fine=True,
                                                    get_y_by_bin=R.LOC_Y_BY_BIN, loc_y_scope=R.LOC_Y_SCOPE, loc_y_bin_size=R.LOC_Y_BIN_SIZE,
                                                    get_ry_fine=True)[0].double().numpy()
    return box, anchor.double().numpy()


def rois_that_decode_to(cfg, boxes3d):
    """RoIs and regression rows -- zero but for the three size residuals, which carry h, w, l (the decode takes the size from the
    anchor, not from the RoI) -- whose decoded boxes are ``boxes3d`` up to f32 rounding"""
    off, anchor = zero_row_decode(cfg)
    want = np.asarray(boxes3d, np.float64)
    ry = want[:, 6] - off[6]
    c, s = np.cos(-ry), np.sin(-ry)
    rois = want.copy()
    rois[:, 0] = want[:, 0] - (off[0] * c - off[2] * s)
    rois[:, 2] = want[:, 2] - (off[0] * s + off[2] * c)
    rois[:, 1] = want[:, 1] - off[1]
    rois[:, 6] = ry
    reg = np.zeros((len(want), CH))
    reg[:, -3:] = want[:, 3:6] / anchor - 1.0
    return rois.astype(np.float32), reg.astype(np.float32)


def cluster_scene(seed, shape):
    """M = 128 RoIs: 32 clusters of 4 near-coincident RoIs 10 m x 7 m apart, one regression row per cluster
    -> rois (128, 7), reg (128, CH), cls (128, 1), cluster (128,)"""
    rng = np.random.default_rng(seed)
    (l0, l1), (w0, w1) = BP.SHAPES[shape]
    k = np.arange(32)
    cx, cz = -35.0 + 10.0 * (k % 8) + rng.uniform(-1, 1, 32), 8.0 + 7.0 * (k // 8) + rng.uniform(-1, 1, 32)
    ry = rng.uniform(-np.pi, np.pi, 32)
    ry[0::2] = 0.0
    l, w = rng.uniform(l0, l1, 32), rng.uniform(w0, w1, 32)
    rows = [BP.to_3d(cx, cz, l, w, ry)]
    for _ in range(3):
        x, z, r = BP.nearly(rng, cx, cz, ry)
        rows.append(BP.to_3d(x, z, l, w, r))
    rois = np.stack(rows, 1).reshape(128, 7)                                    # rows 4 c .. 4 c + 3: cluster c
    reg = np.repeat((rng.standard_normal((32, CH)) * 0.05).astype(np.float32), 4, axis=0)
    anchor = np.asarray(pkg("config").default_eval_cfg().CLS_MEAN_SIZE[0], np.float64)
    reg[:, -3:] = np.repeat(np.stack([np.full(32, 1.5), w, l], 1) / anchor - 1.0, 4, axis=0).astype(np.float32)
    cls = (2.0 + 0.5 * rng.standard_normal((128, 1))).astype(np.float32)
    order = rng.permutation(128)
    return rois[order], reg[order], cls[order], order // 4


TIP_SEED = 6          # chosen on the CPU: the margins of test_final_stage_on_the_tip_family hold, and 0.1 decides one pair


def tip_scene(cfg):
    """M = 100 boxes of the tip family (50 pairs): the decoded boxes are the family's -> rois, reg, cls, the boxes themselves"""
    a3, b3, _ = BP.tip_pairs(TIP_SEED, 50)
    want = np.stack([a3, b3], 1).reshape(100, 7)
    rois, reg = rois_that_decode_to(cfg, want)
    cls = (3.0 - 0.01 * np.arange(100)).astype(np.float32).reshape(100, 1)          # score order = row order
    return rois, reg, cls, want


def both_paths(cfg, rois, reg, cls):
    E = pkg("eval_rcnn")
    B, M = rois.shape[:2]
    ret = {"rois": T(rois), "rcnn_reg": T(reg).view(B * M, -1), "rcnn_cls": T(cls).view(B * M, 1)}
    pkg("runners").FUSED_POSTPROCESS = True
    f = E.postprocess(cfg, ret, B)
    pkg("runners").FUSED_POSTPROCESS = False
    try:
        t = E.postprocess(cfg, ret, B)
    finally:
        pkg("runners").FUSED_POSTPROCESS = True
    torch.cuda.synchronize()
    assert "blob" in f and "blob" not in t                                      # the fused entry ran, and then it did not
    assert torch.equal(f["num"], t["num"]), (f["num"], t["num"])
    assert torch.equal(f["scores"], t["scores"])
    d_box, d_pred = (f["boxes"] - t["boxes"]).abs().max().item(), (f["pred_boxes3d"] - t["pred_boxes3d"]).abs().max().item()
    print("fused against batched torch path: num %s, max |boxes| difference %.3g, decoded %.3g" % (f["num"].tolist(), d_box, d_pred))
    assert d_box < 1e-5 and d_pred < 1e-5
    return f, t


def test_final_stage_on_near_coincident_clusters(oracle):
    """scene 1 (one scene per shape): every cluster's four decoded boxes are near-coincident, clusters do not touch -- the fused
    kernel's LDS polygon holds 9..16 vertices here.  At the configuration's threshold 0.1 and at 0.999 one box per cluster survives
    (the best-scored), at 1.001 every box does: the IoU inside a cluster must come out within 1e-3 of 1, on both paths.  The host
    decodes the scene with the package's torch decode on the CPU and asserts those margins with the oracle."""
    cfg = pkg("config").default_eval_cfg()
    scenes = [cluster_scene(31 + k, shape) for k, shape in enumerate(BP.SHAPES)]
    rois, reg, cls = (np.stack([s[q] for s in scenes], 0) for q in range(3))
    R = cfg.RCNN
    anchor = torch.tensor([float(v) for v in np.asarray(cfg.CLS_MEAN_SIZE[0], np.float32)])
    for b in range(3):
        dec = pkg("bbox_transform").decode_bbox_target(torch.from_numpy(rois[b]), torch.from_numpy(reg[b]), anchor_size=anchor, loc_scope=R.LOC_SCOPE,
                                                        loc_bin_size=R.LOC_BIN_SIZE, num_head_bin=R.NUM_HEAD_BIN, get_xz_fine=True,
                                                        get_y_by_bin=R.LOC_Y_BY_BIN, loc_y_scope=R.LOC_Y_SCOPE, loc_y_bin_size=R.LOC_Y_BIN_SIZE,
                                                        get_ry_fine=True).numpy()
        iou = oracle.boxes_iou_bev(BP.to_bev(dec), BP.to_bev(dec))
        same = scenes[b][3][:, None] == scenes[b][3][None, :]
        crossings, corners = BP.vertex_count(BP.to_bev(dec)[np.argsort(scenes[b][3], kind="stable")][0::4], BP.to_bev(dec)[np.argsort(scenes[b][3], kind="stable")][1::4])
        print("scene %d: IoU inside a cluster %.6f .. %.6f, between clusters <= %g; first two members: %d of 32 polygons with >= 9 vertices" %
              (b, iou[same].min(), iou[same].max(), iou[~same].max(), ((crossings + corners) >= 9).sum()))
        assert 0.9995 < iou[same].min() and iou[same].max() < 1.0005 and iou[~same].max() == 0
        assert ((crossings + corners) >= 9).sum() >= 5
    for thresh, survivors in ((0.1, 32), (0.999, 32), (1.001, 128)):
        cfg.RCNN.NMS_THRESH = thresh
        f, _ = both_paths(cfg, rois, reg, cls)
        assert f["num"].tolist() == [survivors] * 3, thresh
        for b in range(3):                                                      # the survivor is the best-scored member of its cluster
            best = sorted((max(cls[b, scenes[b][3] == c, 0]) for c in range(32)), reverse=True) if survivors == 32 else sorted(cls[b, :, 0], reverse=True)
            assert f["scores"][b, :survivors].tolist() == [float(v) for v in best]


TIP_THRESHOLDS = (0.1, 1e-3)          # the configuration's own, and one that the crossing tips (IoU 0.002 .. 0.06) exceed


def tip_scene_margins(oracle, want):
    """host view of scene 2, all pairs (i < j): beyond the rbox_far_apart reach?  within 2 % of it?  oracle IoU"""
    bev = BP.to_bev(want)
    i, j = np.triu_indices(len(bev), 1)
    far, ratio = BP.far_apart(bev[i], bev[j])
    return far, np.abs(ratio - 1) <= 0.02, oracle.boxes_iou_bev(bev, bev)[i, j]


def test_final_stage_on_the_tip_family(oracle):
    """scene 2: 100 long thin boxes, 50 pairs laid around the reach of rbox_far_apart (the candidate filter of the fused kernel), at
    the configuration's threshold 0.1 and at 1e-3, which every crossing pair exceeds.  The survivors are the oracle's on the intended
    boxes: the decoded boxes are within 2e-5 m of them, which moves an IoU of thin boxes by ~1e-6, and no IoU of the scene lies within
    5e-5 of either threshold (asserted on the host, as is that whatever the filter drops has IoU exactly 0)."""
    cfg = pkg("config").default_eval_cfg()
    assert cfg.RCNN.NMS_THRESH == TIP_THRESHOLDS[0]
    rois, reg, cls, want = tip_scene(cfg)
    far, near_reach, iou = tip_scene_margins(oracle, want)
    print("pairs within 2 %% of the reach: %d beyond it, %d inside it; all pairs: %d beyond, %d inside, %d with IoU > 0 (largest %.4f)" %
          ((far & near_reach).sum(), (~far & near_reach).sum(), far.sum(), (~far).sum(), (iou > 0).sum(), iou.max()))
    assert (far & near_reach).sum() >= 25 and (~far & near_reach).sum() >= 25
    assert (iou[far] == 0).all() and (iou > 0).sum() >= 10
    assert all((np.abs(iou.astype(np.float64) - t) > 5e-5).all() for t in TIP_THRESHOLDS)
    for thresh in TIP_THRESHOLDS:
        cfg.RCNN.NMS_THRESH = thresh
        f, _ = both_paths(cfg, rois[None], reg[None], cls[None])
        # the scene is the one the host looked at: the decode rounds a coordinate of up to 64 m a few times (f32 spacing 3.8e-6 m)
        assert np.abs(f["pred_boxes3d"][0].cpu().numpy() - want).max() < 2e-5
        keep = oracle.nms(BP.to_bev(want), thresh)
        assert f["num"].tolist() == [len(keep)] and len(keep) == (99 if thresh == TIP_THRESHOLDS[0] else 47)
        assert np.abs(f["boxes"][0, :len(keep)].cpu().numpy() - want[keep]).max() < 2e-5


# --------------------------------------------------------------------------------- (d) the RCNN target stage's assignment
def targets_batch(seed):
    """rcnn_targets_batch.make_batch, then every second RoI becomes a near-coincident copy of one of its scene's ground-truth boxes"""
    import rcnn_targets_batch as RB
    d = RB.make_batch(seed=seed, B=2, M=64, g_real=3, g_pad=1, N=512, C=4, plan={"fg_lo": 3, "fg": 4, "none": 0.1, "hard": 0.3, "easy": 0.1})
    rng = np.random.default_rng(seed)
    rois, gt = d["roi_boxes3d"].numpy().copy(), d["gt_boxes3d"].numpy()
    for b in range(rois.shape[0]):
        src = gt[b, rng.integers(0, 3, 32)].astype(np.float64)
        x, z, ry = BP.nearly(rng, src[:, 0], src[:, 2], src[:, 6])
        src[:, 0], src[:, 2], src[:, 6] = x, z, ry
        rois[b, 0::2] = src.astype(np.float32)
    d["roi_boxes3d"] = torch.from_numpy(rois)
    return d


@pytest.mark.parametrize("aug_data,seed", [(True, 21), (False, 24)])
def test_target_stage_assigns_near_coincident_rois(aug_data, seed):
    """device against cpu path: max_overlaps within TOL, the three lists, the chosen RoIs and (without the data augmentation, where
    gt_of_rois carries the ground truth's h, w, l untouched) the assigned ground-truth index exact"""
    import rcnn_targets_batch as RB
    import test_gpu_rcnn_targets as G
    from test_rcnn_targets import T as targets, make_cfg
    d = targets_batch(seed)
    cfg = make_cfg()
    cfg.update({"AUG_DATA": aug_data})
    cpu = targets().RcnnTargets(cfg, seed=1, device="cpu")
    cpu_out = cpu.forward({k: v.clone() for k, v in d.items()})
    bad = RB.margin_failures(cpu.decisions, cpu_out)
    assert not bad, "the case does not hold the margins (choose another seed): %s" % bad
    for b, rec in enumerate(cpu.decisions):
        assert (rec["max_overlaps"][0::2] > 0.999).all() and set(range(0, 64, 2)) <= set(rec["lists"][0].tolist())
    dev = targets().RcnnTargets(cfg, seed=1, device="cuda")
    dev_out = dev.forward({k: v.cuda() for k, v in d.items()})
    assert G.compare(dev, dev_out, cpu, cpu_out) <= G.TOL
    if not aug_data:
        gt = d["gt_boxes3d"].numpy()
        R = len(cpu.decisions[0]["chosen"])
        got = dev_out["gt_of_rois"].cpu().numpy().reshape(len(gt), R, 7)
        for b, rec in enumerate(cpu.decisions):
            want = rec["iou3d"][rec["chosen"]].argmax(1)
            assigned = [np.nonzero((gt[b, :, 3:6] == row[3:6]).all(1))[0] for row in got[b]]
            assert all(len(a) == 1 for a in assigned) and np.array_equal(np.concatenate(assigned), want)


# -------------------------------------------------------------------------------------------- (e) the augmentation collision test
def aug_case():
    """24 long thin labels in rows 2.5 m apart; candidate k is the tip-family partner of label k GROWN by 0.5 m (what the collision
    test compares with) -> labels (24, 7), database (25 entries), partner kinds"""
    import test_gpu_aug_scene as GA
    rng = np.random.default_rng(1911)
    n = 24
    first = np.stack([rng.uniform(-25, 25, n), 8.0 + 2.5 * np.arange(n), rng.uniform(10, 20, n), rng.uniform(0.1, 0.3, n),
                      rng.uniform(-0.02, 0.02, n)], 1)
    labels = BP.to_3d(*first.T, y=1.7, h=1.5)
    grown = labels.astype(np.float64)[:, [0, 2, 5, 4, 6]] + [0, 0, 0.5, 0.5, 0]
    second, kind = BP.tip_partners(rng, grown)
    db = [GA.entry(rng, x, z, ry, (1.5, w, l)) for x, z, l, w, ry in second] + [GA.entry(rng, 1.0, 1.0)]
    return labels, db, kind


def test_aug_collision_on_the_tip_family(oracle):
    """One batch in the style of test_edge_to_edge_and_the_10m_rule: every candidate alone against the labels, and chains of 16.
    The device short-circuits with rbox_far_apart; its accept / reject decisions (and every bit of the rows) equal the cpu path's.
    Host conditions: the (candidate, grown label) pairs lie on both sides of the reach, and every BEV overlap is 0 or > 1e-3 m^2."""
    import test_gpu_aug_scene as GA
    labels, db, kind = aug_case()
    big = labels.copy()
    big[:, 4:6] += np.float32(0.5)
    cand = np.stack([e["gt_box3d"] for e in db[:-1]])
    ov = oracle.boxes_overlap_bev(BP.to_bev(cand), BP.to_bev(big))
    k = np.arange(len(cand))
    far, ratio = BP.far_apart(BP.to_bev(cand), BP.to_bev(big))
    print("partner pairs: %d beyond the reach, %d inside it (distance / reach %.4f .. %.4f); candidates with an overlap: %d of %d" %
          (far.sum(), (~far).sum(), ratio.min(), ratio.max(), (ov.max(1) > 0).sum(), len(cand)))
    assert far.sum() >= 8 and (~far).sum() >= 8 and np.abs(ratio - 1).max() <= 0.021
    assert not ((ov > 0) & (ov <= 1e-3)).any() and (ov[k, k][kind == 0] > 1e-3).all()
    rng = np.random.default_rng(1912)
    sc = GA.scene(GA.cloud(rng, 300, 10), labels)
    jobs = [(0, [i]) for i in range(len(cand))] + [(0, list(range(16))), (0, list(range(23, 7, -1)))]
    want = GA.check([sc], jobs, db)
    alone = [bool(acc) for _, acc in want[:len(cand)]]
    assert alone == [bool(v) for v in ov.max(1) == 0]
    assert sum(alone) == 18                                                     # the six crossing partners are turned away
    assert [[i for i, _ in acc] for _, acc in want[len(cand):]] == [[i for i in range(16) if i % 4], [i for i in range(23, 7, -1) if i % 4]]
