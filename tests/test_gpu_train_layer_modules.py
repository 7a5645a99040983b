"""-m gpu: the training layer behind pytorch_utils.FUSED_TRAIN_LAYERS, at module level: conv blocks, SharedMLPs, one SA and one FP
module, and train_rcnn --fused_layers.

The small chains run from equal weights and random normal inputs with the switch on and off.  The seed is the first one whose f64 CPU
run keeps every pre-activation 1e-4 from zero (asserted), so no ReLU mask differs between the paths; outputs, every parameter
gradient and the BatchNorm buffers then sit inside 8 x e_ref (losses_batch.tolerance), e_ref = |torch's f32 modules on this GPU - the
f64 CPU run|.  The SA + FP graph has no f64 form (its operators are f32 only): there the fused graph is held to the same graph with
the switches off under the bar tests/test_gpu_autograd.py sets between two f32 graphs of these modules (2e-5 of the tensor's largest
magnitude + 1e-7)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import losses_batch as LB
import train_layer_ref as R
import train_tree
from conftest import pkg
from test_engine_structure import Recorder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pt():
    return pkg("pointnet2.pytorch_utils")


def build(kind):
    """-> (module on the CPU in f32, input shape)"""
    P = pt()
    if kind == "shared_mlp_bn":
        return P.SharedMLP([6, 16, 32], bn=True), (2, 6, 37, 5)
    if kind == "head_chain":                                       # an RPN head: Conv1d + bn + ReLU, dropout, a last Conv1d without activation
        return nn.Sequential(P.Conv1d(32, 16, bn=True), nn.Dropout(0.0), P.Conv1d(16, 3, activation=None)), (2, 32, 61)
    if kind == "rcnn_mlp":                                         # RCNN.USE_BN off: bias + ReLU
        return P.SharedMLP([7, 16, 24], bn=False), (3, 7, 29, 4)
    raise KeyError(kind)


KINDS = ["shared_mlp_bn", "head_chain", "rcnn_mlp"]


def run_module(net, x, dy):
    """one training forward + backward -> (y, dx, {parameter: grad}, {buffer: value}) as f64 numpy"""
    net.train()
    for p in net.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    y = net(x)
    y.backward(dy)
    n64 = lambda t: t.detach().double().cpu().numpy()
    return n64(y), n64(x.grad), {k: n64(p.grad) for k, p in net.named_parameters()}, {k: n64(b) for k, b in net.named_buffers()}


def margin_of(net, x):
    """the smallest |pre-activation| of a training forward: the input of every ReLU, read before it is applied in place"""
    seen, hooks = [], []
    for act in {id(m): m for m in net.modules() if isinstance(m, nn.ReLU)}.values():
        hooks.append(act.register_forward_pre_hook(lambda mod, args: seen.append(float(args[0].detach().abs().min()))))
    state = copy.deepcopy(net.state_dict())
    try:
        net.train()
        net(x)
    finally:
        for h in hooks:
            h.remove()
        net.load_state_dict(state)
    return min(seen) if seen else float("inf")


_SOLVED = {}


def solved(kind):
    """-> dict: the f64 CPU run, torch's f32 GPU run (switch off), the fused GPU run, and the two GPU modules; computed once"""
    if kind in _SOLVED:
        return _SOLVED[kind]
    for seed in range(64):
        torch.manual_seed(1000 + seed)
        net, shape = build(kind)
        with torch.no_grad():                                      # BatchNorm parameters and buffers off their defaults
            for m in net.modules():
                if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                    m.weight.uniform_(0.5, 1.5); m.bias.normal_(); m.running_mean.normal_(); m.running_var.uniform_(0.5, 2.0)
                if isinstance(m, (nn.Conv1d, nn.Conv2d)) and m.bias is not None:
                    m.bias.normal_()
        x, dy_seed = torch.randn(shape), seed
        net64 = copy.deepcopy(net).double()
        margin = margin_of(net64, x.double())
        if margin >= R.MARGIN:
            break
    assert margin >= R.MARGIN, "no seed keeps the pre-activations %g from zero" % R.MARGIN
    y64 = net64.train()(x.double())
    dy = torch.randn(y64.shape, generator=torch.Generator().manual_seed(dy_seed))
    net64.load_state_dict(copy.deepcopy(net).double().state_dict())
    ref = run_module(net64, x.double(), dy.double())
    plain, fused = copy.deepcopy(net).to(DEV), copy.deepcopy(net).to(DEV)
    t32 = run_module(plain, x.to(DEV), dy.to(DEV))
    with pt().fused_train_layers():
        got = run_module(fused, x.to(DEV), dy.to(DEV))
    _SOLVED[kind] = dict(ref=ref, t32=t32, got=got, plain=plain, fused=fused, net64=net64, margin=margin, seed=seed, x=x, dy=dy)
    return _SOLVED[kind]


def flat(run):
    y, dx, grads, bufs = run
    out = {"y": y, "dx": dx}
    out.update({"grad " + k: v for k, v in grads.items()})
    out.update({"buffer " + k: v for k, v in bufs.items() if not k.endswith("num_batches_tracked")})
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_fused_blocks_sit_inside_the_bound_of_torchs_own_modules(kind):
    s = solved(kind)
    print("%s: seed %d, smallest |pre-activation| of the f64 run %.3e" % (kind, s["seed"], s["margin"]))
    ref, t32, got = flat(s["ref"]), flat(s["t32"]), flat(s["got"])
    assert set(ref) == set(t32) == set(got)
    report, ok = [], True
    for k in sorted(ref):
        e_ref = float(np.abs(t32[k] - ref[k]).max())
        assert np.isfinite(got[k]).all(), k
        ok &= LB.check_tensor("%s %s" % (kind, k), got[k], ref[k], e_ref, report)
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_blocks_leave_the_state_dict_torch_would_have_left(kind):
    s = solved(kind)
    a, b = s["plain"].state_dict(), s["fused"].state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].device == b[k].device, k
        if k.endswith("num_batches_tracked"):
            assert int(a[k]) == int(b[k]) == 1, k
    assert any(k.endswith("num_batches_tracked") for k in a) == (kind != "rcnn_mlp")


def entries_reached(net, x, switch, train=True):
    pu = pkg("pointnet2.pointnet2_utils")
    log, saved = [], pu.pointnet2
    pu.pointnet2 = Recorder(saved, log)
    try:
        net.train(train)
        with pt().fused_train_layers(switch):
            y = net(x)
            if train:
                y.sum().backward()
        torch.cuda.synchronize()
    finally:
        pu.pointnet2 = saved
    return [n for n in log if n.startswith("train_layer")]


def test_only_covered_blocks_with_the_switch_on_reach_the_entries():
    P = pt()
    torch.manual_seed(3)
    mlp = P.SharedMLP([6, 16, 32], bn=True).to(DEV)
    x = torch.randn((2, 6, 37, 5), device=DEV)
    assert entries_reached(mlp, x, False) == []
    assert entries_reached(mlp, x, True, train=False) == []                 # eval mode: the fixed RPN of --train_mode rcnn
    preact = P.SharedMLP([6, 16, 32], bn=True, preact=True).to(DEV)
    assert entries_reached(preact, x, True) == []
    inorm = P.Conv2d(6, 16, instance_norm=True).to(DEV)
    assert entries_reached(inorm, x, True) == []
    on = entries_reached(mlp, x, True)
    assert on.count("train_layer_forward_wrapper") == 2 and on.count("train_layer_backward_wrapper") == 2
    # weights frozen and an input without gradient: nothing is left to differentiate, the backward entry is not reached
    for p in mlp.parameters():
        p.requires_grad_(False)
    mlp.train()
    with P.fused_train_layers():
        assert not mlp(x).requires_grad


def test_an_extension_module_without_the_entries_raises_by_name():
    import types
    pu = pkg("pointnet2.pointnet2_utils")
    block = pt().Conv1d(8, 8, bn=True).to(DEV).train()
    saved = pu.pointnet2
    pu.pointnet2 = types.SimpleNamespace(__name__="nine_names_only")
    try:
        with pt().fused_train_layers(), pytest.raises(RuntimeError, match="train_layer_forward_wrapper"):
            block(torch.randn((2, 8, 5), device=DEV))
    finally:
        pu.pointnet2 = saved


def test_sa_and_fp_modules_under_both_switches_stay_at_the_graph_with_the_switches_off():
    PM, pu = pkg("pointnet2.pointnet2_modules"), pkg("pointnet2.pointnet2_utils")
    torch.manual_seed(4)
    B, N, M, C = 3, 2048, 512, 24
    xyz = torch.from_numpy(pkg("synth").scenes(B, N, seed0=60)).to(DEV)
    sa = PM.PointnetSAModuleMSG(npoint=M, radii=[0.8, 1.6], nsamples=[16, 32], mlps=[[C, 32, 48], [C, 32, 64]], use_xyz=True, bn=True).to(DEV)
    fp = PM.PointnetFPModule(mlp=[48 + 64 + C, 64, 32], bn=True).to(DEV)
    sa.train(); fp.train()
    base = torch.randn((B, C, N), device=DEV)
    target = torch.randn((B, 32, N), device=DEV)
    params = list(sa.parameters()) + list(fp.parameters())
    state = copy.deepcopy((sa.state_dict(), fp.state_dict()))
    results = []
    for on in (False, True):
        sa.load_state_dict(state[0]); fp.load_state_dict(state[1])
        feats = base.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        with pt().fused_train_layers(on), pu.ordered_backward(on):
            new_xyz, coarse = sa(xyz, feats)
            out = fp(xyz, new_xyz, feats, coarse)
            loss = ((out - target) ** 2).mean() + coarse.abs().mean()
            loss.backward()
        torch.cuda.synchronize()
        bufs = [b.detach().clone() for m in (sa, fp) for k, b in m.named_buffers()]
        results.append((out.detach().clone(), coarse.detach().clone(), feats.grad.detach().clone(), [p.grad.detach().clone() for p in params], bufs))
    (o1, c1, g1, p1, b1), (o2, c2, g2, p2, b2) = results
    assert float(g1.abs().max()) > 0 and all(float(p.abs().max()) > 0 for p in p2)

    def close(a, b, what):
        scale = max(1e-6, float(b.abs().max()))
        err = float((a.double() - b.double()).abs().max())
        print("%-24s err %.3e of %.3e (%.2e)" % (what, err, scale, err / scale))
        assert err <= 2e-5 * scale + 1e-7, (what, err, scale)
    close(o2, o1, "fp output"); close(c2, c1, "sa output"); close(g2, g1, "d loss / d features")
    for k, (a, b) in enumerate(zip(p2, p1)):
        close(a, b, "parameter %d" % k)
    for k, (a, b) in enumerate(zip(b2, b1)):
        close(a, b, "buffer %d" % k)


def test_train_rcnn_fused_layers_two_iterations(tmp_path):
    import yaml
    from test_host_logic import TINY
    G, C, T = pkg("gt_database"), pkg("config"), pkg("train_rcnn")
    root = str(tmp_path / "tree")
    os.makedirs(root)
    train_tree.write_train_tree(root)
    G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cpu", log=lambda *a: None)
    db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
    over = {"RPN": dict(TINY["RPN"], NUM_POINTS=train_tree.NPOINTS), "TRAIN": {"SPLIT": train_tree.SPLIT, "PCT_START": 0.5}}
    cfg_file = str(tmp_path / "tiny.yaml")
    with open(cfg_file, "w") as f:
        yaml.safe_dump(over, f)
    runs = {}
    for name, extra in (("plain", []), ("fused", ["--fused_layers"])):
        out = str(tmp_path / name)
        it = T.main(["--train_mode", "rpn", "--root", root, "--gt_database", db, "--cfg_file", cfg_file, "--batch_size", "3", "--epochs", "1",
                     "--ckpt_save_interval", "1", "--npoints_faraway", str(train_tree.NPOINTS_FARAWAY), "--output_dir", out, "--seed", "1"] + extra)
        assert it == 2
        with open(os.path.join(out, "train_log.jsonl")) as f:
            lines = [json.loads(ln) for ln in f]
        with open(os.path.join(out, "log_train.txt")) as f:
            runs[name] = (lines, f.read(), os.path.join(out, "ckpt", "checkpoint_epoch_1.pth"))
    assert pt().FUSED_TRAIN_LAYERS is False
    assert "fused_layers True" not in runs["plain"][1] and not any(ln.split("INFO")[-1].strip().startswith("fused_layers") for ln in runs["plain"][1].splitlines())
    assert runs["fused"][1].count("fused_layers True") == 1
    cfg = C.apply_train_defaults(C.make_cfg(), "rpn")
    C.merge_into(over, cfg)
    model = pkg("net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TEST")
    assert pkg("eval_rcnn").load_checkpoint(model, runs["fused"][2]) == 1
    plain_state = torch.load(runs["plain"][2], map_location="cpu", weights_only=False)["model_state"]
    fused_state = torch.load(runs["fused"][2], map_location="cpu", weights_only=False)["model_state"]
    assert list(plain_state) == list(fused_state) and all(plain_state[k].dtype == fused_state[k].dtype for k in plain_state)
    assert all(int(v) == 2 for k, v in fused_state.items() if k.endswith("num_batches_tracked"))
    a, b = runs["plain"][0][0]["loss"], runs["fused"][0][0]["loss"]
    print("first iteration: loss %.9e without the flag, %.9e with it (relative %.2e)" % (a, b, abs(a - b) / abs(a)))
    assert [ln["it"] for ln in runs["fused"][0]] == [1, 2] and all(np.isfinite(ln["loss"]) for ln in runs["fused"][0])
    assert abs(a - b) <= 1e-4 * abs(a)
