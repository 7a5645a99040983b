"""-m gpu: the proposal layer at the TRAINING quotas (csrc/proposal.hip with RPN_POST_NMS_TOP_N up to 512: 358 near + 154 far) and the
axis-aligned quota NMS with the 512-row kept-box table (csrc/nms_device.hip nms_quota_kernel<512>, max_keep 257..512).

Every comparison is exact (torch.equal / array_equal): the fused layer states the batched torch formulation operation for operation,
and a keep list is a list of decisions.  Before the quotas were lifted everything above 128 raised "rpn_proposals: unsupported quotas"."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import box_pairs as BP  # noqa: E402
from conftest import pkg  # noqa: E402
from test_gpu_box_pairs import run_device, check_device  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------- the layer against the torch path
def train_cfg(M, nms_type="normal"):
    C = pkg("config")
    cfg = C.default_eval_cfg()
    C.merge_into({"RPN": {"NMS_TYPE": nms_type}, "TRAIN": {"RPN_PRE_NMS_TOP_N": 9000, "RPN_POST_NMS_TOP_N": M, "RPN_NMS_THRESH": 0.85}}, cfg)
    return cfg


_INPUTS = {}


def layer_inputs():
    """B = 4 scenes of N = 7000 points (no power of two, above the 4096-key one-workgroup sort; scene 1 needs more than 6300 near
    points for the spill pass).  scene 0: both bands full; 1: no far point (z in [5, 35]: a decoded centre moves by less than 5 m), the
    far band takes near ranks 6300..6999; 2: 200 near points, the rest far; 3: 50 points in range, the rest beyond 80 m"""
    if not _INPUTS:
        rng = np.random.default_rng(4512)
        B, N = 4, 7000
        xyz = rng.uniform([-40, -1, 0.5], [40, 3, 70], (B, N, 3)).astype(np.float32)
        xyz[1, :, 2] = rng.uniform(5, 35, N)
        xyz[2, :200, 2] = rng.uniform(5, 35, 200)
        xyz[2, 200:, 2] = rng.uniform(45, 70, N - 200)
        xyz[3, :, 2] = rng.uniform(100, 120, N)
        xyz[3, :50, 2] = rng.uniform(5, 30, 50)
        _INPUTS["xyz"] = torch.from_numpy(xyz).to(DEV)
        _INPUTS["reg"] = torch.from_numpy((rng.standard_normal((B, N, 76)) * 0.5).astype(np.float32)).to(DEV)
        _INPUTS["scores"] = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32)).to(DEV)
    return _INPUTS["xyz"], _INPUTS["reg"], _INPUTS["scores"]


def fused_layer(ext, cfg, PL, xyz, reg, scores):
    M = cfg.TRAIN.RPN_POST_NMS_TOP_N
    rois = torch.full((xyz.shape[0], M, 7), -7.0, device=DEV)
    sc = torch.full((xyz.shape[0], M), -7.0, device=DEV)
    ext.iou3d.rpn_proposals(xyz, scores, reg, PL._anchor, cfg.RPN.LOC_SCOPE, cfg.RPN.LOC_BIN_SIZE, cfg.RPN.NUM_HEAD_BIN, cfg.RPN.LOC_XZ_FINE,
                            cfg.TRAIN.RPN_PRE_NMS_TOP_N, M, cfg.TRAIN.RPN_NMS_THRESH, cfg.RPN.NMS_TYPE == "rotate", rois, sc)
    return rois, sc


def check_layer(ext, M, nms_type):
    cfg = train_cfg(M, nms_type)
    PL = pkg("net.proposal_layer").ProposalLayer(cfg, mode="TRAIN").to(DEV)
    xyz, reg, scores = layer_inputs()
    rois_f, sc_f = fused_layer(ext, cfg, PL, xyz, reg, scores)
    PL.fused = False
    rois_t, sc_t = PL(scores, reg, xyz)
    torch.cuda.synchronize()
    near, far = int(M * 0.7), M - int(M * 0.7)
    filled = (rois_t.abs().sum(-1) > 0).sum(1).tolist()
    print("M %d (%d + %d), %s: RoIs per scene %s" % (M, near, far, nms_type, filled))
    # the inputs do what they are meant to (conditions on the torch path's own result)
    assert filled[0] == M                                                     # scene 0 fills both quotas
    assert filled[1] == M and float(rois_t[1, :, 2].max()) <= 40.0            # scene 1: the far quota filled from NEAR proposals (the spill pass)
    if near > 200:                                                            # scene 2: fewer near keeps than the quota, far ones behind them, zeros
        assert far < filled[2] <= 200 + far < M and (rois_t[2, filled[2]:] == 0).all()
    else:                                                                     # (M = 129, 128: 200 near points fill a quota of 90 / 89)
        assert filled[2] == M
    assert float(rois_t[2, filled[2] - far, 2]) > 40.0 and float(rois_t[2, filled[2] - far - 1, 2]) <= 40.0
    assert 0 < filled[3] <= 50
    assert torch.equal(sc_f, sc_t)
    assert torch.equal(rois_f, rois_t), float((rois_f - rois_t).abs().max())


@pytest.mark.parametrize("M", [512, 300, 129, 128])
def test_fused_proposal_layer_at_training_quotas_equals_batched_torch_path(ext, M):
    """512 = 358 + 154 (TRAIN of the shipped configurations), 300 = 210 + 90 (neither a multiple of 64), 129 = 90 + 39 (the first size
    beyond the inference limit: two trips of the assembly, the 256-row table), 128 (what inference may ask for: one trip)"""
    check_layer(ext, M, "normal")


def test_fused_proposal_layer_at_training_quotas_rotated_nms(ext):
    """NMS_TYPE rotate: the lazy form as before (its quota is any max_keep), the assembly in four trips"""
    check_layer(ext, 512, "rotate")


def test_quotas_beyond_512_still_raise(ext):
    L = pkg("_lib")
    cfg = train_cfg(513)
    PL = pkg("net.proposal_layer").ProposalLayer(cfg, mode="TRAIN").to(DEV)
    xyz, reg, scores = layer_inputs()
    with pytest.raises(L.PrcnnError, match="rpn_proposals"):
        fused_layer(ext, cfg, PL, xyz, reg, scores)


# ------------------------------------------------------------------------------------------------ the quota form against the oracle
N_MAX = 700
SCENE_A = (202, 700, 1, N_MAX)        # 700 boxes of their own on the overlapping grid: 688 survive 0.85, 387 survive 0.1
SCENE_C = (212, 175, 4, N_MAX)        # 175 clusters of 4 near-coincident copies: fewer survivors than any quota here


def spread(bev, f):
    """every box moved to f times its centre: the grid's neighbours no longer touch, boxes placed on their predecessor still do"""
    b = bev.copy()
    cx, cz = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    b[:, 0] += (f - 1) * cx
    b[:, 2] += (f - 1) * cx
    b[:, 1] += (f - 1) * cz
    b[:, 3] += (f - 1) * cz
    return b.astype(np.float32)


_SETS = {}


def quota_sets(oracle, thresh):
    """-> (a, c, s, the oracle's axis-aligned greedy keep lists of each over all 700 rows)"""
    if thresh not in _SETS:
        a, c = BP.clustered_scene(*SCENE_A)[0], BP.clustered_scene(*SCENE_C)[0]
        s = spread(a, 2.0)
        _SETS[thresh] = (a, c, s) + tuple(oracle.nms_normal(x, thresh) for x in (a, c, s))
    return _SETS[thresh]


@pytest.mark.parametrize("thresh", [0.85, 0.1])
@pytest.mark.parametrize("K", [257, 358, 512])
def test_quota_form_with_the_512_row_table_against_the_oracle(ext, oracle, K, thresh):
    """nms_device, axis-aligned, n_max = 700, max_keep = K in (256, 512]: keep list and count are the first K entries of the oracle's
    full greedy pass (the lazy form's contract), and the first 256 of them are what max_keep = 256 -- the 256-row instantiation --
    returns.  Problems: the grid scene (0.85: the quota is reached; 0.1: at 512 it is not), near-coincident clusters (never reached),
    counts = 0, the spread scene cut behind its K-th survivor (exactly K survivors, the walk ends with the rows) and the spread scene
    whole (more than K survivors at both thresholds: the walk stops at the quota)."""
    a, c, s, want_a, want_c, want_s = quota_sets(oracle, thresh)
    assert len(want_s) > K and len(want_c) < 257
    last = int(want_s[K - 1])
    print("thresh %g K %d: survivors %d / %d / %d, the K-th survivor of the spread scene is row %d (%d of its block)"
          % (thresh, K, len(want_a), len(want_c), len(want_s), last, last % 64))
    assert last % 64 != 63                                   # the quota is reached in the MIDDLE of a 64-row block: rows of the block are left over
    if thresh == 0.85:
        assert len(want_a) > K and int(want_a[K - 1]) % 64 != 63
    boxes = np.stack([a, c, a, s, s], 0)
    counts = [N_MAX, N_MAX, 0, last + 1, N_MAX]
    wants = [want_a, want_c, want_a[:0], want_s[:K], want_s]
    assert len(oracle.nms_normal(s[:last + 1], thresh)) == K                    # exactly max_keep survivors
    keep, num = run_device(ext, boxes, counts, thresh, False, K)
    check_device(keep, num, wants, K)
    keep256, num256 = run_device(ext, boxes, counts, thresh, False, 256)
    check_device(keep256, num256, wants, 256)
    for p in range(len(wants)):
        assert np.array_equal(keep[p, :min(256, num[p])], keep256[p, :num256[p]])
