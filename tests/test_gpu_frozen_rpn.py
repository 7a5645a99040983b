"""-m gpu: the frozen first stage of --train_mode rcnn on the inference engine (net/frozen_rpn.py FrozenFirstStage,
PointRCNN.use_engine_first_stage, train_rcnn --engine_rpn).

Model: default.yaml's networks (the fused RPN tail needs their widths) at 4096 points per scene with a quarter of the SA levels' points
-- the shape __graft_entry__.smoke() runs -- B = 2, seeded weights with BatchNorm statistics away from the identity
(helpers.seeded_state_dict).  Bounds: 1e-4 between engine and module graph is the project's bound for that pair
(test_full_size_engine_with_intensity_equals_module_path); everything else is exact."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import helpers  # noqa: E402
import train_tree  # noqa: E402
from conftest import pkg  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = {"RPN": {"NUM_POINTS": 4096, "SA_CONFIG": {"NPOINTS": [1024, 256, 64, 16]}}}
B, N = 2, 4096


def make_cfg(**over):
    C = pkg("config")
    cfg = C.apply_train_defaults(C.make_cfg(), "rcnn")
    from test_host_logic import TINY
    C.merge_into(SHAPE, cfg)
    C.merge_into({"RCNN": TINY["RCNN"]}, cfg)                  # the second stage is not what these tests are about: the small one
    C.merge_into(over, cfg)
    return cfg


def make_model(cfg, seed=31):
    model = pkg("net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN")
    sd, _ = helpers.seeded_state_dict(model.state_dict(), seed)
    model.load_state_dict(sd)
    model = model.to(DEV)
    for p in model.rpn.parameters():
        p.requires_grad = False
    return model.train()


_CACHE = {}


def shared():
    """-> (cfg, model in training mode, its stage, input A, input B, the stage's output on A): built once, left unchanged"""
    if not _CACHE:
        cfg = make_cfg()
        model = make_model(cfg)
        S = pkg("synth")
        a = torch.from_numpy(S.lidar_scenes(B, N, seed0=810)).to(DEV)
        b = torch.from_numpy(S.lidar_scenes(B, N, seed0=820)).to(DEV)
        with torch.no_grad():                                  # the score bias moved so that a fifth of A's points is foreground
            raw = model._first_stage({"pts_input": a})["rpn_cls"]
            logit = float(np.log(cfg.RPN.SCORE_THRESH / (1 - cfg.RPN.SCORE_THRESH)))
            model.rpn.rpn_cls_layer[-1].conv.bias += logit - float(torch.quantile(raw.flatten(), 0.8))
        stage = pkg("net.frozen_rpn").FrozenFirstStage(model, cfg)
        out = {k: v.clone() for k, v in stage(a).items()}
        _CACHE["v"] = (cfg, model, stage, a, b, out)
    return _CACHE["v"]


def test_stage_equals_the_module_graph_within_the_engine_bound():
    cfg, model, stage, a, _, out = shared()
    assert model.training and not model.rpn.training
    with torch.no_grad():
        first = model._first_stage({"pts_input": a})
        extras, feed = model._second_stage_inputs(first)
    assert out["rpn_features"].shape == (B, N, 128) and out["rpn_features"].is_contiguous()
    for name, got, want in (("rpn_features", out["rpn_features"], feed["rpn_features"]), ("pts_depth", out["pts_depth"], feed["pts_depth"]),
                            ("rpn_cls", out["rpn_cls"], first["rpn_cls"])):
        err = float((got - want).abs().max())
        print("%-14s largest difference %.3e (values up to %.3e)" % (name, err, float(want.abs().max())))
        assert got.shape == want.shape and err <= 1e-4, name
    assert torch.equal(out["rpn_xyz"], feed["rpn_xyz"]) and torch.equal(out["backbone_xyz"], a)
    prob = torch.sigmoid(first["rpn_cls"][:, :, 0])
    decided = (prob - cfg.RPN.SCORE_THRESH).abs() > 1e-4
    assert int(decided.sum()) > 0.99 * B * N and 0 < float(feed["seg_mask"].mean()) < 1
    assert torch.equal(out["seg_mask"][decided], feed["seg_mask"][decided]) and torch.equal(out["seg_mask"], out["seg_result"])
    M = cfg.TRAIN.RPN_POST_NMS_TOP_N
    assert M == 512 and out["rois"].shape == (B, M, 7) and out["roi_scores_raw"].shape == (B, M) and torch.equal(out["rois"], out["roi_boxes3d"])
    assert sorted(out) == sorted(["rpn_xyz", "rpn_features", "seg_mask", "pts_depth", "roi_boxes3d", "rois", "roi_scores_raw", "seg_result",
                                  "backbone_xyz", "rpn_cls"])


def test_proposals_equal_the_torch_path_on_the_engines_own_rows():
    """the proposal layer alone: the TRAIN-mode torch formulation (fused = False) over the SAME engine's scores and regression rows"""
    cfg, model, stage, a, _, out = shared()
    pl = model.rpn.proposal_layer
    assert pl.mode == "TRAIN"
    with torch.no_grad():
        st = stage.engine.rpn_stage(a, want_reg=True)
        assert st["rpn_reg"] is not None and torch.equal(st["rpn_cls"], out["rpn_cls"])
        pl.fused = False
        try:
            rois, raw = pl(st["rpn_scores_raw"], st["rpn_reg"], st["backbone_xyz"])
        finally:
            pl.fused = True
    filled = (rois.abs().sum(-1) > 0).sum(1).tolist()
    print("RoIs per scene", filled)
    assert min(filled) > 358                                   # both bands contribute
    assert torch.equal(out["roi_scores_raw"], raw)
    assert torch.equal(out["rois"], rois), float((out["rois"] - rois).abs().max())


def test_outputs_outlive_the_next_call():
    cfg, model, stage, a, b, out = shared()
    first = stage(a)
    clones = {k: v.clone() for k, v in first.items()}
    second = stage(b)
    torch.cuda.synchronize()
    assert not torch.equal(second["rpn_features"], clones["rpn_features"])
    for k, v in first.items():
        assert torch.equal(v, clones[k]), k
        assert torch.equal(v, out[k]), k                       # and a call repeats itself bit for bit
        assert not v.requires_grad


def test_two_training_iterations_leave_the_first_stage_alone():
    cfg, model0, _, a, _, out = shared()
    L, O = pkg("losses"), pkg("optim")
    model = copy.deepcopy(model0)
    model.use_engine_first_stage(None)
    stage = pkg("net.frozen_rpn").FrozenFirstStage(model, cfg)
    model.use_engine_first_stage(stage)
    model.train()
    model.rcnn_net.target_seed = 5
    T = cfg.TRAIN
    opt = O.OneCycleAdam(model, 4, T.LR, list(T.MOMS), T.DIV_FACTOR, T.PCT_START, T.WEIGHT_DECAY, T.GRAD_NORM_CLIP)
    rpn_before = {k: v.clone() for k, v in model.rpn.state_dict().items()}
    rcnn_before = {k: v.detach().clone() for k, v in model.rcnn_net.named_parameters()}
    batch = {"pts_input": a, "gt_boxes3d": out["rois"][:, :3].contiguous()}      # three RoIs of each scene as its labels: foreground exists
    assert (batch["gt_boxes3d"].abs().sum(-1) > 0).all()
    # the same batch through the module graph's first stage (no flag): the loop's other path, same RoI-sampling seed
    model.use_engine_first_stage(None)
    model.rcnn_net.target_seed, model.rcnn_net._targets = 5, None
    plain = float(L.model_fn(cfg, model, batch)[0].detach())
    model.use_engine_first_stage(stage)
    model.rcnn_net.target_seed, model.rcnn_net._targets = 5, None
    print("first loss through the module graph %.6f" % plain)
    assert np.isfinite(plain)
    for it in range(2):
        opt.schedule(it)
        opt.zero_grad()
        loss, tb, _ = L.model_fn(cfg, model, batch)
        loss.backward()
        assert all(p.grad is None for p in model.rpn.parameters())
        for k, p in model.rcnn_net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        opt.step()
        print("it %d loss %.6f grad norm %.4f fg %s" % (it, float(loss.detach()), float(opt.total_norm), tb.get("rcnn_reg_fg")))
        assert np.isfinite(float(loss.detach())) and np.isfinite(float(opt.total_norm))
    for k, p in model.rcnn_net.named_parameters():
        assert not torch.equal(p.detach(), rcnn_before[k]), k
    now = model.rpn.state_dict()
    assert list(now) == list(rpn_before) and any(k.endswith("num_batches_tracked") for k in now)
    for k, v in now.items():
        assert torch.equal(v, rpn_before[k]), k
    stage.check_weights()                                      # the optimizer stepped on rcnn_net: not this engine's business
    assert len(stage.engine._state) == len(list(model.rpn.parameters())) + len(list(model.rpn.buffers()))
    assert not any(n.startswith(("xyz_up", "merge_down", "rcnn")) for n, _ in stage.engine.weight_tensors())
    again = stage(a)
    assert torch.equal(again["rpn_features"], out["rpn_features"]) and torch.equal(again["rois"], out["rois"])


def test_stale_weights_raise_and_refresh_rebuilds():
    cfg, model0, _, a, _, out = shared()
    model = copy.deepcopy(model0)
    model.use_engine_first_stage(None)
    F = pkg("net.frozen_rpn")
    stage = F.FrozenFirstStage(model, cfg)
    sd, _ = helpers.seeded_state_dict(model.rpn.state_dict(), 77)
    model.rpn.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="parameters changed after the engine was built"):
        stage(a)
    stage.refresh()
    got = stage(a)
    fresh = F.FrozenFirstStage(model, cfg)(a)
    assert not torch.equal(got["rpn_features"], out["rpn_features"])
    for k in got:
        assert torch.equal(got[k], fresh[k]), k


def test_refusals():
    cfg, model, _, a, _, _ = shared()
    F, P = pkg("net.frozen_rpn"), pkg("net.point_rcnn")
    stage = F.FrozenFirstStage(model, cfg)
    loose = make_cfg()
    loose.RPN.FIXED = False
    with pytest.raises(ValueError, match="use_engine_first_stage"):
        P.PointRCNN(loose, num_classes=2, use_xyz=True, mode="TRAIN").use_engine_first_stage(stage)
    inten = make_cfg(RPN={"USE_INTENSITY": True})
    with pytest.raises(NotImplementedError, match="RPN.USE_INTENSITY"):
        F.FrozenFirstStage(P.PointRCNN(inten, num_classes=2, use_xyz=True, mode="TRAIN").to(DEV), inten)
    wide = make_cfg(TRAIN={"RPN_POST_NMS_TOP_N": 600})
    with pytest.raises(NotImplementedError, match="RPN_POST_NMS_TOP_N = 600"):
        F.FrozenFirstStage(model, wide)
    narrow = make_cfg(RPN={"REG_FC": [128, 128]})              # a three-layer regression head: no fused tail (csrc/rpn_tail.hip has two)
    with pytest.raises(NotImplementedError, match="no fused tail"):
        F.FrozenFirstStage(P.PointRCNN(narrow, num_classes=2, use_xyz=True, mode="TRAIN").to(DEV), narrow)


def test_train_rcnn_engine_rpn_trains_checkpoints_and_resumes(tmp_path):
    import yaml
    from test_host_logic import TINY
    G, T = pkg("gt_database"), pkg("train_rcnn")
    root = str(tmp_path / "tree")
    os.makedirs(root)
    train_tree.write_train_tree(root)
    G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cpu", log=lambda *a: None)
    db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
    over = dict(SHAPE, RCNN=TINY["RCNN"], TRAIN={"SPLIT": train_tree.SPLIT, "PCT_START": 0.5})
    cfg_file = str(tmp_path / "shape.yaml")
    with open(cfg_file, "w") as f:
        yaml.safe_dump(over, f)
    out = str(tmp_path / "out")
    base = ["--train_mode", "rcnn", "--root", root, "--gt_database", db, "--cfg_file", cfg_file, "--batch_size", "2", "--ckpt_save_interval", "1",
            "--npoints_faraway", "1000", "--output_dir", out, "--seed", "1", "--engine_rpn"]
    cfg = T.make_cfg(T.build_parser().parse_args(base))
    torch.manual_seed(1)                                       # the loop's own initialisation
    init = pkg("net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN").state_dict()
    seeded, _ = helpers.seeded_state_dict(init, 41)
    C = {k: v for k, v in seeded.items() if k.startswith("rpn.")}
    rpn_ckpt = str(tmp_path / "rpn.pth")
    torch.save({"model_state": C}, rpn_ckpt)

    per_epoch = len(train_tree.SAMPLE_IDS) // 2
    assert T.main(base + ["--epochs", "1", "--rpn_ckpt", rpn_ckpt]) == per_epoch
    ckpt = os.path.join(out, "ckpt", "checkpoint_epoch_1.pth")
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert sorted(saved) == ["epoch", "it", "model_state", "optimizer_state"] and list(saved["model_state"]) == list(init)
    for k, v in saved["model_state"].items():
        if k.startswith("rpn."):
            assert torch.equal(v, C[k]), k
    changed = [k for k, v in saved["model_state"].items() if k.startswith("rcnn_net.") and not torch.equal(v, init[k])]
    same = [k for k in init if k.startswith("rcnn_net.") and k not in changed]
    print("unchanged after %d iterations: %s" % (per_epoch, same))
    # the regression head learns from foreground RoIs only, which a seeded first stage does not propose on this tree: its biases (no
    # weight decay) may stand still; everything else moves (the two-iteration test above trains with foreground)
    assert len(changed) >= 30 and all(k.startswith("rcnn_net.reg_layer.") and k.endswith(".bias") for k in same)
    with open(os.path.join(out, "log_train.txt")) as f:
        text = f.read()
    assert sum(ln.split("INFO")[-1].strip().startswith("engine_rpn") for ln in text.splitlines()) == 1 and text.count("engine_rpn True:") == 1
    with open(os.path.join(out, "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["it"] for ln in lines] == list(range(1, per_epoch + 1))
    assert all(np.isfinite(ln["loss"]) and np.isfinite(ln["grad_norm"]) and "rcnn_loss" in ln for ln in lines)

    assert T.main(base + ["--epochs", "2", "--ckpt", ckpt]) == 2 * per_epoch       # the stage is built after the load, from the checkpoint's RPN
    with open(os.path.join(out, "log_train.txt")) as f:
        text = f.read()
    assert "resumed at epoch 1, it %d" % per_epoch in text and text.count("engine_rpn True") == 2
    again = torch.load(os.path.join(out, "ckpt", "checkpoint_epoch_2.pth"), map_location="cpu", weights_only=False)
    assert again["it"] == 2 * per_epoch and again["epoch"] == 2
    for k, v in again["model_state"].items():
        if k.startswith("rpn."):
            assert torch.equal(v, C[k]), k
    assert any(not torch.equal(again["model_state"][k], saved["model_state"][k]) for k in changed)
    with open(os.path.join(out, "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert len(lines) == 2 * per_epoch and all(np.isfinite(ln["loss"]) for ln in lines)
