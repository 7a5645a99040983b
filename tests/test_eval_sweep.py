"""The checkpoint sweep (eval_rcnn --eval_all) without a GPU: which checkpoints it picks, what --rpn_ckpt / --rcnn_ckpt load, and the
engine's in-place weight reload on the tiny PointRCNN over the oracle operator backend.  eval_rcnn.main has no CPU path (it raises
without a GPU), so the end-to-end sweep is tests/test_gpu_eval_sweep.py's."""
import argparse
import glob
import logging
import os
import re

import pytest
import torch

from conftest import pkg
from test_host_logic import tiny_model


# ---------------------------------------------------------------------------------------------------------------- selection
def _reference_loop(ckpt_dir, record_file, start_epoch):
    """get_no_evaluated_ckpt of the reference (tools/eval_rcnn.py:775-788) called until nothing is left, every pick recorded as
    repeat_eval_ckpt records it.  An id that is no number makes the reference's float() raise; the sweep passes it over."""
    picked = []
    evaluated = [float(x.strip()) for x in open(record_file).readlines()]
    while True:
        ckpt_list = glob.glob(os.path.join(ckpt_dir, "*checkpoint_epoch_*.pth"))
        ckpt_list.sort(key=os.path.getmtime)
        hit = None
        for cur in ckpt_list:
            num_list = re.findall("checkpoint_epoch_(.*).pth", cur)
            if len(num_list) == 0:
                continue
            epoch_id = num_list[-1]
            try:
                float(epoch_id)
            except ValueError:
                continue
            if float(epoch_id) not in evaluated and int(float(epoch_id)) >= start_epoch:
                hit = (epoch_id, cur)
                break
        if hit is None:
            return picked
        picked.append(hit)
        evaluated.append(float(hit[0]))


@pytest.fixture()
def ckpt_tree(tmp_path):
    d = tmp_path / "ckpt"
    d.mkdir()
    # (name, modification time): the order by time is not the order by name
    files = [("checkpoint_epoch_10.pth", 500), ("checkpoint_epoch_2.pth", 900), ("checkpoint_epoch_12.5.pth", 100),
             ("checkpoint_epoch_best.pth", 50), ("best_checkpoint_epoch_7.pth", 700), ("checkpoint_epoch_3.pth", 300),
             ("checkpoint_epoch_4.pth", 400), ("checkpoint.pth", 10), ("checkpoint_epoch_5.txt", 20)]
    for name, t in files:
        p = d / name
        p.write_bytes(b"x")
        os.utime(p, (1_000_000 + t, 1_000_000 + t))
    record = tmp_path / "eval_list_val.txt"
    record.write_text("")
    return str(d), str(record)


def test_selection_is_the_references_loop(ckpt_tree):
    S = pkg("eval_sweep")
    d, record = ckpt_tree
    got = S.unevaluated_ckpts(d, record, 0)
    assert [e for e, _ in got] == ["12.5", "3", "4", "10", "7", "2"]              # by modification time; "best" and the rest are no ids
    assert os.path.basename(got[4][1]) == "best_checkpoint_epoch_7.pth"
    assert got == _reference_loop(d, record, 0)
    assert S.get_no_evaluated_ckpt(d, record, 0) == got[0]
    # ids already in the record (as the reference writes them, and as a number written another way), and --start_epoch
    with open(record, "w") as f:
        f.write("3\n12.5\n10.0\n")
    got = S.unevaluated_ckpts(d, record, 0)
    assert [e for e, _ in got] == ["4", "7", "2"] and got == _reference_loop(d, record, 0)
    got = S.unevaluated_ckpts(d, record, 4)
    assert [e for e, _ in got] == ["4", "7"] and got == _reference_loop(d, record, 4)
    open(record, "w").close()
    got = S.unevaluated_ckpts(d, record, 11)
    assert [e for e, _ in got] == ["12.5"] and got == _reference_loop(d, record, 11)    # int(float("12.5")) = 12 >= 11
    assert S.unevaluated_ckpts(d, record, 13) == [] and S.get_no_evaluated_ckpt(d, record, 13) == (-1, None)


def test_a_train_output_directory_is_a_ckpt_dir(ckpt_tree):
    S = pkg("eval_sweep")
    d, _ = ckpt_tree
    assert S.resolve_ckpt_dir(os.path.dirname(d)) == d and S.resolve_ckpt_dir(d) == d


def test_the_driver_knows_the_sweeps_flags():
    a = pkg("eval_rcnn").build_parser().parse_args(["--eval_all", "--ckpt_dir", "d", "--rpn_ckpt", "r", "--rcnn_ckpt", "c"])
    assert a.eval_all and a.ckpt_dir == "d" and a.start_epoch == 0 and a.extra_tag == "default" and a.wait is None
    assert (a.rpn_ckpt, a.rcnn_ckpt) == ("r", "c")


# ---------------------------------------------------------------------------------------------------------------- part checkpoints
def _randomised(model, seed):
    """a state dict of the model's shapes with other weights AND other BatchNorm statistics (the fold matters)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = v.clone()
        elif k.endswith("running_var"):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        else:
            sd[k] = v + torch.randn(v.shape, generator=g) * 0.02 * (v.abs().mean() + 0.05)
    return sd


def test_part_checkpoints_load_the_keys_the_model_has(tmp_path):
    E = pkg("eval_rcnn")
    model, cfg, _ = tiny_model()
    a_state = {k: v.clone() for k, v in model.state_dict().items()}
    b_state = _randomised(model, 5)
    full = str(tmp_path / "full.pth")
    torch.save({"model_state": b_state, "epoch": 3, "it": 7}, full)
    rcnn_only = str(tmp_path / "rcnn.pth")
    torch.save({"model_state": {k: v for k, v in _randomised(model, 6).items() if k.startswith("rcnn_net.")}}, rcnn_only)
    foreign = str(tmp_path / "foreign.pth")
    torch.save({"model_state": {"some.other.net.weight": torch.zeros(3)}}, foreign)
    args = argparse.Namespace(rpn_ckpt=None, rcnn_ckpt=rcnn_only)
    # --ckpt, then --rcnn_ckpt: the RPN keys stay the first file's, the RCNN keys are the second's
    E.load_checkpoint(model, full)
    E.load_part_ckpts(model, args, logging.getLogger("test"))
    c_state = torch.load(rcnn_only, weights_only=False)["model_state"]
    for k, v in model.state_dict().items():
        want = c_state[k] if k.startswith("rcnn_net.") else b_state[k]
        assert torch.equal(v, want), k
    assert any(not torch.equal(a_state[k], b_state[k]) for k in a_state if k.startswith("rpn."))
    with pytest.raises(RuntimeError):
        E.load_part_ckpts(model, argparse.Namespace(rpn_ckpt=foreign, rcnn_ckpt=None))
    with pytest.raises(FileNotFoundError):
        E.load_part_ckpts(model, argparse.Namespace(rpn_ckpt=None, rcnn_ckpt=str(tmp_path / "nothing.pth")))
    # one function, shared with the train loop
    assert getattr(E, "load_part_ckpt", pkg("train_rcnn").load_part_ckpt) is pkg("train_rcnn").load_part_ckpt
    S = pkg("eval_sweep")
    assert S.misfit(model, b_state) is None
    short = dict(b_state)
    k0 = "rpn.rpn_cls_layer.0.conv.weight"
    short[k0] = short[k0][:-1]
    assert k0 in S.misfit(model, short)


# ---------------------------------------------------------------------------------------------------------------- reload in place
KEYS = ("rpn_cls", "rpn_reg", "rpn_features", "rois", "roi_scores_raw", "rcnn_cls", "rcnn_reg")


def _forward(eng, pts):
    out = eng.forward(pts)
    return {k: out[k].clone() for k in KEYS}


def test_reload_weights_is_a_fresh_engine_in_the_old_tensors(oracle):
    from oracle import ext_cpu
    F, fm = pkg("net.fast_infer"), pkg("pointnet2.fused_mlp")
    model, cfg, g = tiny_model()
    pts = torch.from_numpy(g["pts"])
    a_state = {k: v.clone() for k, v in model.state_dict().items()}
    b_state = _randomised(model, 11)
    with ext_cpu.patch_package():
        eng = F.FastPointRCNN(model, cfg)
        out_a = _forward(eng, pts)
        held = eng.weight_tensors()
        names = [n for n, _ in held]
        # the tiny network has every kind of form but the default.yaml-only ones (packed / wide / the fused tail: the GPU test's)
        assert any(".layers[" in n for n in names) and any(".split[" in n for n in names) and any(".narrow[" in n for n in names)
        assert eng.rcnn_head1 is None or "rcnn_head1.w" in names
        ptrs = [(n, t.data_ptr(), tuple(t.shape)) for n, t in held]
        folded = [(m, [(w.data_ptr(), b.data_ptr()) for w, b in m.__dict__["_prcnn_folded"][1]])
                  for m in model.modules() if "_prcnn_folded" in m.__dict__]
        assert folded

        owned = [t.clone() for _, t in held]
        model.load_state_dict(b_state)
        with pytest.raises(RuntimeError, match="load the checkpoint first"):
            eng.check_weights()
        for (n, t), was in zip(held, owned):
            assert torch.equal(t, was), "%s is the model's own storage: the load reached the engine" % n
        with pytest.raises(RuntimeError):
            eng.forward(pts)
        eng.reload_weights()
        eng.check_weights()
        out_b = _forward(eng, pts)
        fresh = F.FastPointRCNN(model, cfg)
        want_b = _forward(fresh, pts)
        for k in KEYS:
            assert torch.equal(out_b[k], want_b[k]), k
        assert any(not torch.equal(out_a[k], out_b[k]) for k in ("rpn_cls", "rcnn_cls"))
        # every tensor of the engine is where it was, and holds what a fresh engine's holds
        assert [(n, t.data_ptr(), tuple(t.shape)) for n, t in eng.weight_tensors()] == ptrs
        for (n, t), (n2, t2) in zip(eng.weight_tensors(), fresh.weight_tensors()):
            assert n == n2 and torch.equal(t, t2), n
        # ... and so is fused_mlp's folded cache, which the nn.Module path reads
        for m, was in folded:
            sig, layers = m.__dict__["_prcnn_folded"]
            assert [(w.data_ptr(), b.data_ptr()) for w, b in layers] == was and sig == fm._signature(m)
            for (w, b), (w2, b2) in zip(layers, fm.fold_fresh(m)):
                assert torch.equal(w, w2) and torch.equal(b, b2)

        # back to A: the first outputs
        model.load_state_dict(a_state)
        eng.reload_weights()
        out_a2 = _forward(eng, pts)
        for k in KEYS:
            assert torch.equal(out_a2[k], out_a[k]), k

        # one layer of another width: ValueError naming it, nothing written
        conv = model.rpn.rpn_cls_layer[0].conv
        keep = conv.weight
        conv.weight = torch.nn.Parameter(torch.zeros(keep.shape[0] + 8, *keep.shape[1:]))
        before = [t.clone() for _, t in eng.weight_tensors()]
        with pytest.raises(ValueError, match=r"rpn\.rpn_cls_layer\.0\.conv\.weight"):
            eng.reload_weights()
        conv.weight = keep
        for t, (n, t2) in zip(before, eng.weight_tensors()):
            assert torch.equal(t, t2), n
        out_a3 = _forward(eng, pts)
        for k in KEYS:
            assert torch.equal(out_a3[k], out_a[k]), k


def test_runners_refuse_a_reload_with_a_batch_in_flight(oracle):
    from oracle import ext_cpu
    E = pkg("eval_rcnn")
    model, cfg, g = tiny_model(intensity=True)
    pts = torch.from_numpy(g["pts"])
    b_state = _randomised(model, 12)
    with ext_cpu.patch_package():
        runner = E.make_runner(model, cfg, "cpu")
        assert isinstance(runner, E.EngineRunner)
        assert runner.submit(pts) is None
        with pytest.raises(RuntimeError, match="in flight"):
            runner.reload_weights()
        det_a = runner.flush()
        model.load_state_dict(b_state)
        runner.reload_weights()
        runner.submit(pts)
        det_b = runner.flush()
        want = E.infer_batch(model, cfg, pts, engine=E.FastPointRCNN(model, cfg))
    for k in ("boxes", "scores", "num", "rcnn_cls"):
        assert torch.equal(det_b[k], want[k]), k
    assert not torch.equal(det_a["rcnn_cls"], det_b["rcnn_cls"])
