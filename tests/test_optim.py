"""The weight step on the host (optim.py: schedules, groups, the cpu checker path, checkpoints; the C entries' argument checks;
train_rcnn.py's out-of-scope switches) against fixture g24 (tests/golden/make_golden_optim.py: the reference's own OptimWrapper, OneCycle
and clip_grad_norm_ in f32, and teacher-forced single steps in f64).  No GPU.

Bound (tests/losses_batch.py tolerance, the g23 rule): every tensor and quantity within 8 x its own e_ref = max |ref32 - ref64| of the
f64 step, 4 ulp (f32) at the tensor's largest magnitude where e_ref is 0."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_batch as OB  # noqa: E402
from conftest import pkg  # noqa: E402


def test_one_cycle_equals_every_recorded_table_bit_for_bit():
    z, _names, _sizes = OB.load_fixture()
    O = OB.O()
    lr_max, m0, m1, div = (float(v) for v in z["oc_hyper"])
    seen = 0
    for total, pct in OB.TABLES:
        key = "oc_%d_%g" % (total, pct)
        if key + "_raises" in z:                                             # an empty first phase: the reference divides by zero
            with pytest.raises(ZeroDivisionError):
                O.one_cycle(0, total, lr_max, [m0, m1], div, pct)
            continue
        want = z[key]
        got = np.array([O.one_cycle(k, total, lr_max, [m0, m1], div, pct) for k in range(total)], dtype=np.float64)
        assert got.shape == want.shape == (total, 2) and np.array_equal(got.view(np.uint64), want.view(np.uint64)), key
        seen += 1
    assert seen >= 5
    lr, mom = O.one_cycle(0, 12, lr_max, [m0, m1], div, 0.4)
    assert type(lr) is float and type(mom) is float                          # plain floats, not numpy scalars


def test_layer_groups_of_the_full_model_are_the_recorded_names():
    z, _names, _sizes = OB.load_fixture()
    want = json.loads(str(z["rcnn_groups"]))
    cfg = pkg("config").default_eval_cfg()
    model = pkg("eval_rcnn").build_model(cfg, "cpu")
    got = OB.O().group_names(model)
    assert got == want and len(got[0]) + len(got[1]) == 142
    groups = OB.O().layer_groups(model)
    assert sum(p.numel() for g in groups for p in g) == 3887452
    bn = {id(p) for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for p in m.parameters()}
    assert all(id(p) in bn for p in groups[1]) and not any(id(p) in bn for p in groups[0])
    for p in model.rpn.parameters():                                         # frozen later: still in its group
        p.requires_grad = False
    assert OB.O().group_names(model) == want


def test_cpu_path_teacher_forced_through_g24():
    assert OB.teacher_forced("cpu") == []


def test_bn_momentum_schedule_and_setter():
    O, cfg = OB.O(), pkg("config").make_cfg()
    T = cfg.TRAIN
    assert O.bn_momentum(cfg, 0) == T.BN_MOMENTUM and O.bn_momentum(cfg, 50) == T.BN_MOMENTUM * T.BN_DECAY
    assert O.bn_momentum(cfg, 10 ** 6) == T.BN_MOMENTUM * T.BN_DECAY ** 6 > T.BNM_CLIP
    T.BN_MOMENTUM = 0.1                                                      # 0.1 / 64 lies below the floor
    assert O.bn_momentum(cfg, 10 ** 6) == T.BNM_CLIP and O.bn_momentum(cfg, 49) == 0.1
    model = OB.tiny_model()
    O.set_bn_momentum(model, 0.03)
    assert model.bn.momentum == 0.03 and model.block.bn2.momentum == 0.03


def _run(opt, model, z, names, sizes, steps):
    for k in steps:
        opt.schedule(k)
        opt.zero_grad()
        OB.set_grads(model, names, z["grads"][k], sizes)
        opt.step()


def test_state_dict_structure_and_interchange_with_torch_adam():
    z, names, sizes = OB.load_fixture()
    want = json.loads(str(z["state_structure"]))
    model, opt = OB.fresh(z, names, sizes)
    _run(opt, model, z, names, sizes, range(OB.STEPS))
    sd = opt.state_dict()
    assert sorted(sd) == want["top"] and [sorted(g) for g in sd["param_groups"]] == want["group_keys"]
    assert [g["params"] for g in sd["param_groups"]] == want["params"]
    assert {str(i): list(st) for i, st in sd["state"].items()} == want["state_keys"]
    assert sorted(sd["state"]) == json.loads(str(z["state_ids"]))
    assert [g["betas"][1] for g in sd["param_groups"]] == want["betas2"] and [g["weight_decay"] for g in sd["param_groups"]] == want["weight_decay"]
    assert all(g["lr"] == opt.lr and g["betas"][0] == opt.mom for g in sd["param_groups"])
    # ours -> torch.optim.Adam
    groups = opt.groups
    adam = torch.optim.Adam([{"params": g, "lr": 0} for g in groups], betas=(0.9, 0.99))
    adam.load_state_dict(sd)
    back = adam.state_dict()
    assert sorted(back["state"]) == sorted(sd["state"])
    for i, st in sd["state"].items():
        assert float(back["state"][i]["step"]) == OB.STEPS and torch.equal(back["state"][i]["exp_avg"], st["exp_avg"])
    # torch.optim.Adam -> a fresh object of ours
    model2, opt2 = OB.fresh(z, names, sizes)
    opt2.load_state_dict(back)
    m1, v1, ids1, steps1 = OB.get_state(sd, names, sizes)
    m2, v2, ids2, steps2 = OB.get_state(opt2.state_dict(), names, sizes)
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and ids1 == ids2 and steps1 == steps2 == [OB.STEPS] * len(ids1)
    assert (opt2.lr, opt2.mom, opt2.steps_done) == (opt.lr, opt.mom, OB.STEPS)
    with pytest.raises(ValueError):
        bad = {"state": {}, "param_groups": [dict(sd["param_groups"][0], params=[0]), sd["param_groups"][1]]}
        opt2.load_state_dict(bad)


def test_twelve_steps_equal_six_plus_checkpoint_plus_six(tmp_path):
    z, names, sizes = OB.load_fixture()
    model, opt = OB.fresh(z, names, sizes)
    _run(opt, model, z, names, sizes, range(12))
    half, opt_h = OB.fresh(z, names, sizes)
    _run(opt_h, half, z, names, sizes, range(6))
    torch.save({"model_state": half.state_dict(), "optimizer_state": opt_h.state_dict()}, str(tmp_path / "c.pth"))
    ckpt = torch.load(str(tmp_path / "c.pth"), map_location="cpu", weights_only=False)
    resumed, opt_r = OB.fresh(z, names, sizes)
    resumed.load_state_dict(ckpt["model_state"])
    opt_r.load_state_dict(ckpt["optimizer_state"])
    _run(opt_r, resumed, z, names, sizes, range(6, 12))
    assert np.array_equal(OB.get_params(model, names), OB.get_params(resumed, names))
    a, b = OB.get_state(opt.state_dict(), names, sizes), OB.get_state(opt_r.state_dict(), names, sizes)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert opt_r.steps_done == 12 and float(opt.total_norm) == float(opt_r.total_norm)


def test_parameters_must_be_contiguous_f32():
    O = OB.O()
    model = OB.tiny_model().half()
    with pytest.raises(ValueError, match="contiguous float32"):
        O.OneCycleAdam(model, **OB.HYPER)
    model = OB.tiny_model()
    model.lin_a.weight.data = torch.randn(5, 3).t()                          # (3, 5) with strides (1, 3)
    with pytest.raises(ValueError, match="contiguous float32"):
        O.OneCycleAdam(model, **OB.HYPER)
    model = OB.tiny_model()
    opt = O.OneCycleAdam(model, **OB.HYPER)
    model.lin_a.weight.data = torch.randn(5, 3).t()
    with pytest.raises(ValueError, match="contiguous float32"):
        opt.step()
    with pytest.raises(ValueError, match="grad_norm_clip"):
        O.OneCycleAdam(OB.tiny_model(), **dict(OB.HYPER, grad_norm_clip=0.0))


def test_c_entries_reject_null_pointers_and_bad_sizes():
    L = pkg("_lib")
    L.load()
    assert OB.O().CHUNK == L.PRCNN_OPTIM_CHUNK == 2048
    assert L.call("prcnn_optim_workspace", 0) == 2 and L.call("prcnn_optim_workspace", 7) == 9
    buf = (C.c_double * 64)()
    ok = C.addressof(buf)                                                    # a non-null address: every call below is rejected before any launch
    cases = [("prcnn_optim_workspace", [-1])]
    sumsq = [ok, ok, ok, ok, 1, 1, ok, None]
    finish = [ok, ok, 1, 1, 1.0, ok, None]
    update = [ok, ok, ok, ok, ok, ok, ok, ok, ok, 1, 1, 1e-3, 0.9, 0.99, 1e-8, 1e-3, ok, None]
    for name, good, ptrs, sizes in (("prcnn_optim_sumsq", sumsq, (0, 1, 2, 3, 6), (4, 5)), ("prcnn_optim_finish", finish, (0, 1, 5), (2, 3)),
                                    ("prcnn_optim_update", update, (0, 1, 2, 3, 4, 5, 6, 7, 8, 16), (9, 10))):
        for k in ptrs:
            cases.append((name, good[:k] + [None] + good[k + 1:]))
        for k in sizes:
            cases += [(name, good[:k] + [v] + good[k + 1:]) for v in (0, -1)]
    cases.append(("prcnn_optim_sumsq", sumsq[:5] + [(1 << 22) + 1] + sumsq[6:]))
    cases.append(("prcnn_optim_finish", finish[:4] + [0.0] + finish[5:]))
    cases.append(("prcnn_optim_finish", finish[:4] + [float("nan")] + finish[5:]))
    cases += [("prcnn_optim_update", update[:k] + [v] + update[k + 1:]) for k, v in ((11, -1.0), (12, 1.0), (13, -0.1), (14, -1.0), (15, float("nan")))]
    for name, args in cases:
        with pytest.raises(L.PrcnnError, match=name[len("prcnn_"):]):
            L.call(name, *args)
    assert len(cases) >= 30


@pytest.mark.parametrize("argv, name", [
    (["--train_mode", "rpn", "--mgpus"], "--mgpus"),
    (["--train_mode", "rpn", "--train_with_eval"], "--train_with_eval"),
    (["--train_mode", "rcnn_offline"], "rcnn_offline"),
    (["--train_mode", "rpn"], "TRAIN.OPTIMIZER 'adam'"),
    (["--train_mode", "rpn"], "TRAIN.OPTIMIZER 'sgd'"),
])
def test_out_of_scope_switches_raise_by_name(tmp_path, argv, name):
    T = pkg("train_rcnn")
    with pytest.raises(NotImplementedError) as e:
        T.main(argv + ["--root", str(tmp_path), "--output_dir", str(tmp_path / "out"), "--device", "cpu"] +
               (["--set", "TRAIN.OPTIMIZER", name.split("'")[1]] if "OPTIMIZER" in name else []))     # --set takes the rest of the line
    assert name in str(e.value)
    assert not (tmp_path / "out").exists()                                   # raised before anything is written
