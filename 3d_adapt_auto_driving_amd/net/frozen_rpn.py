"""The frozen first stage of ``--train_mode rcnn`` on the inference engine.

With ``RPN.ENABLED = RPN.FIXED = True`` the reference trains the RCNN on a first stage that never changes (point_rcnn.py:27-38:
``self.rpn.eval()``, no grad).  That is an inference workload, so `FrozenFirstStage` hands it to the point-major engine
(net/fast_infer.py) built over ``model.rpn`` ALONE: backbone, heads with the box decode in the fused tail (csrc/rpn_tail.hip), the
per-point RCNN inputs (`point_aux`) and the proposal layer at the TRAIN-mode quotas (csrc/proposal.hip: RPN_POST_NMS_TOP_N <= 512).
It stands where the reference has ``rcnn_offline`` (features dumped to disk once): nothing is written, the first stage is simply cheap.

What the engine folds and version-tracks is the RPN's parameters and buffers -- BatchNorm with its RUNNING statistics, which is what
the module path uses under RPN.FIXED.  Nothing of ``rcnn_net`` is folded or watched, so the optimizer steps on it freely; a change of
the RPN's own tensors (``load_state_dict``) makes the next call raise through ``check_weights()`` until `refresh()` is called.

A configuration the engine does not cover raises NotImplementedError BY NAME at construction; there is no fall-back to the module
graph (leave the stage off for those).

Tensor lifetime: every tensor handed out is allocated by the call that returns it (the engine's outputs are new tensors; its scratch
is internal and never handed out), so all of them stay valid for as long as the caller holds them -- across later calls too.  The
stage runs under ``no_grad`` and the RCNN's target stage makes new tensors from these, so autograd never keeps a buffer the engine
rewrites.  tests/test_gpu_frozen_rpn.py pins this.
"""
import torch

from .fast_infer import FastPointRCNN

POST_NMS_MAX = 512        # csrc/proposal.hip: near int(0.7 * 512) = 358, far 154
POINTS_MAX = 65536


def check_quotas(pre, post):
    """the quota rules of prcnn_rpn_proposals (include/prcnn_hip.h), by name"""
    pre_near, post_near = int(pre * 0.7), int(post * 0.7)
    if post > POST_NMS_MAX:
        raise NotImplementedError("FrozenFirstStage: RPN_POST_NMS_TOP_N = %d, the fused proposal layer takes at most %d" % (post, POST_NMS_MAX))
    if post < 1 or post_near < post - post_near or pre_near < pre - pre_near:
        raise NotImplementedError("FrozenFirstStage: RPN_PRE_NMS_TOP_N = %d / RPN_POST_NMS_TOP_N = %d are quotas the fused proposal layer does "
                                  "not take (near >= far)" % (pre, post))


def check_cfg(cfg, mode="TRAIN"):
    """What can be refused from the configuration alone (no model, no GPU): raises NotImplementedError naming the key."""
    from ..runners import engine_covers
    if cfg.RPN.USE_INTENSITY:
        raise NotImplementedError("FrozenFirstStage: RPN.USE_INTENSITY (the engine's general kernels, no fused tail) is not covered")
    if not engine_covers(cfg):
        raise NotImplementedError("FrozenFirstStage: engine_covers(cfg) is false (RCNN.USE_INTENSITY stays on the module graph)")
    if cfg.RPN.NUM_POINTS > POINTS_MAX:
        raise NotImplementedError("FrozenFirstStage: RPN.NUM_POINTS = %d > %d points per scene" % (cfg.RPN.NUM_POINTS, POINTS_MAX))
    if not cfg.TEST.RPN_DISTANCE_BASED_PROPOSE:
        raise NotImplementedError("FrozenFirstStage: TEST.RPN_DISTANCE_BASED_PROPOSE off (the score-based proposal layer) is not covered")
    if cfg.RPN.NMS_TYPE not in ("normal", "rotate"):
        raise NotImplementedError("FrozenFirstStage: RPN.NMS_TYPE %r is not covered" % (cfg.RPN.NMS_TYPE,))
    check_quotas(cfg[mode].RPN_PRE_NMS_TOP_N, cfg[mode].RPN_POST_NMS_TOP_N)


class FrozenFirstStage:
    """``stage = FrozenFirstStage(model, cfg); model.use_engine_first_stage(stage)``.  ``model`` may be in training mode; ``model.rpn``
    is put into eval mode (PointRCNN._first_stage does the same on every call under RPN.FIXED)."""

    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg
        pl = model.rpn.proposal_layer
        check_cfg(cfg, pl.mode)
        model.rpn.eval()
        self.engine = FastPointRCNN(model, cfg, rpn_only=True)
        if self.engine.rpn_tail is None:
            raise NotImplementedError("FrozenFirstStage: this RPN has no fused tail (csrc/rpn_tail.hip: FP_MLPS[0] 128-128 over 256 "
                                      "interpolated channels, CLS_FC / REG_FC [128])")
        if self.engine._tail_decode_cfg(cfg.RPN.NUM_POINTS) is None:
            raise NotImplementedError("FrozenFirstStage: the fused tail cannot decode this configuration's boxes for the fused proposal "
                                      "layer (regression layout, ProposalLayer.fused, or an extension entry is missing)")

    def check_weights(self):
        self.engine.check_weights()

    def refresh(self):
        """The RPN's weights were replaced on purpose (--ckpt, --rpn_ckpt): fold them again, in place (FastPointRCNN.reload_weights)."""
        self.model.rpn.eval()
        self.engine.reload_weights()

    @torch.no_grad()
    def __call__(self, pts_input):
        """pts_input (B, N, 3) -> dict: the RCNN's feed ``rpn_xyz`` (B,N,3), ``rpn_features`` (B,N,128) point-major, ``seg_mask`` (B,N),
        ``pts_depth`` (B,N), ``roi_boxes3d`` (B,M,7), and the extras ``rois``, ``roi_scores_raw`` (B,M), ``seg_result``, ``backbone_xyz``,
        ``rpn_cls`` (B,N,1) -- what PointRCNN._first_stage + _second_stage_inputs hand on, all new tensors (module docstring)."""
        eng = self.engine
        if self.model.rpn.training:
            self.model.rpn.eval()
        if pts_input.shape[1] > POINTS_MAX:
            raise NotImplementedError("FrozenFirstStage: %d > %d points per scene" % (pts_input.shape[1], POINTS_MAX))
        st = eng.rpn_stage(pts_input, want_reg=False)
        if st.get("rpn_boxes") is None:
            raise RuntimeError("FrozenFirstStage: the fused tail did not decode the boxes (N = %d)" % pts_input.shape[1])
        eng.point_aux(st)
        rois, roi_scores_raw = eng.propose(st)
        return {"rpn_xyz": st["backbone_xyz"], "rpn_features": st["rpn_features"], "seg_mask": st["seg_result"], "pts_depth": st["pts_depth"],
                "roi_boxes3d": rois, "rois": rois, "roi_scores_raw": roi_scores_raw, "seg_result": st["seg_result"],
                "backbone_xyz": st["backbone_xyz"], "rpn_cls": st["rpn_cls"]}


FEED_KEYS = ("rpn_xyz", "rpn_features", "seg_mask", "roi_boxes3d", "pts_depth")
EXTRA_KEYS = ("rois", "roi_scores_raw", "seg_result")
