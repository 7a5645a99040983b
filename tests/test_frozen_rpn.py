"""The frozen first stage without a GPU: train_rcnn's --engine_rpn (parsed, refused with --train_mode rpn before anything is written,
silent without it), the refusals that the configuration alone decides (net/frozen_rpn.py check_cfg), and
PointRCNN.use_engine_first_stage on a model whose RPN is not fixed."""
import os

import pytest

from conftest import pkg


def test_train_rcnn_parses_engine_rpn_and_refuses_it_for_rpn_training(tmp_path):
    T = pkg("train_rcnn")
    assert T.build_parser().parse_args(["--train_mode", "rcnn", "--root", "r"]).engine_rpn is False
    assert T.build_parser().parse_args(["--train_mode", "rcnn", "--root", "r", "--engine_rpn"]).engine_rpn is True
    out = tmp_path / "out"
    with pytest.raises(ValueError, match="--engine_rpn"):
        T.main(["--train_mode", "rpn", "--engine_rpn", "--root", str(tmp_path / "empty"), "--output_dir", str(out), "--device", "cpu"])
    assert not os.path.exists(out)
    with pytest.raises(NotImplementedError, match="RPN_POST_NMS_TOP_N = 600"):       # a quota the fused layer does not take: by name, nothing written
        T.main(["--train_mode", "rcnn", "--engine_rpn", "--root", str(tmp_path / "empty"), "--output_dir", str(out), "--device", "cpu",
                "--set", "TRAIN.RPN_POST_NMS_TOP_N", "600"])
    assert not os.path.exists(out)


def test_a_run_without_the_flag_logs_what_it_always_logged(tmp_path):
    """main() up to the input stage, which finds no tree under an empty root: by then the arguments are logged (the pattern of
    test_scatter_ref.test_train_rcnn_accepts_and_logs_ordered_backward)"""
    T = pkg("train_rcnn")
    out = tmp_path / "plain"
    with pytest.raises(Exception):
        T.main(["--train_mode", "rcnn", "--root", str(tmp_path / "empty"), "--output_dir", str(out), "--device", "cpu"])
    text = (out / "log_train.txt").read_text()
    assert "Start logging" in text and "engine_rpn" not in text
    keys = [ln.split("INFO")[-1].split()[0] for ln in text.splitlines() if "INFO" in ln and "*" not in ln]
    want = [k for k in vars(T.build_parser().parse_args(["--train_mode", "rcnn", "--root", "r"])) if k not in ("ordered_backward", "fused_layers", "engine_rpn")]
    assert keys == want


def test_check_cfg_refuses_by_name():
    C, F = pkg("config"), pkg("net.frozen_rpn")

    def cfg(**over):
        c = C.apply_train_defaults(C.make_cfg(), "rcnn")
        C.merge_into(over, c)
        return c
    F.check_cfg(cfg())                                                             # default.yaml: 9000 -> 512 at 0.85, 'normal'
    for over, name in ((dict(RPN={"USE_INTENSITY": True}), "RPN.USE_INTENSITY"), (dict(RCNN={"USE_INTENSITY": True}), "engine_covers"),
                       (dict(TRAIN={"RPN_POST_NMS_TOP_N": 600}), "RPN_POST_NMS_TOP_N = 600"), (dict(TRAIN={"RPN_POST_NMS_TOP_N": 513}), "RPN_POST_NMS_TOP_N = 513"),
                       (dict(TRAIN={"RPN_POST_NMS_TOP_N": 1}), "near >= far"), (dict(RPN={"NUM_POINTS": 65537}), "RPN.NUM_POINTS"),
                       (dict(RPN={"NMS_TYPE": "soft"}), "RPN.NMS_TYPE"), (dict(TEST={"RPN_DISTANCE_BASED_PROPOSE": False}), "RPN_DISTANCE_BASED_PROPOSE")):
        with pytest.raises(NotImplementedError, match=name):
            F.check_cfg(cfg(**over))
    F.check_cfg(cfg(TRAIN={"RPN_POST_NMS_TOP_N": 512}))
    F.check_cfg(cfg(TRAIN={"RPN_POST_NMS_TOP_N": 129}))


def test_use_engine_first_stage_needs_a_fixed_rpn():
    from test_host_logic import TINY
    C, P = pkg("config"), pkg("net.point_rcnn")
    cfg = C.apply_train_defaults(C.make_cfg(), "rcnn")
    C.merge_into(TINY, cfg)
    model = P.PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN")
    marker = object()
    model.use_engine_first_stage(marker)                                           # fixed RPN under an RCNN: accepted
    assert model._engine_first_stage is marker and "_engine_first_stage" not in model.state_dict()
    model.use_engine_first_stage(None)
    assert model._engine_first_stage is None
    cfg.RPN.FIXED = False
    with pytest.raises(ValueError, match="use_engine_first_stage"):
        model.use_engine_first_stage(marker)
    model.use_engine_first_stage(None)                                             # unsetting is always allowed
