"""Generates tests/golden/g24_optim_ref.npz: the REFERENCE's own weight step -- tools/train_utils/fastai_optim.py OptimWrapper.create(
partial(optim.Adam, betas=(0.9, 0.99)), 3e-3, layer_groups, wd, true_wd=True, bn_wd=True), learning_schedules_fastai.OneCycle and
torch.nn.utils.clip_grad_norm_, driven as tools/train_utils/train_utils.py Trainer drives them -- on the tiny model and the recorded
gradients of tests/optim_batch.py.

RUN IN THE BUILD CONTAINER ONLY (imports the reference through ref_harness, read-only):
    python tests/golden/make_golden_optim.py

One shim: the reference's ``from collections import Iterable`` needs collections.Iterable (gone since Python 3.10) set before the import.
The run is TEACHER-FORCED: the f32 run goes through the 12 steps; for every step a fresh f64 model and wrapper are loaded with the f32
run's parameters and optimizer state from BEFORE that step and take that one step on the same (f32-valued) grads, so every comparison
is one step deep.  e_ref = max |ref32 - ref64| per step, tensor and quantity is the reference's own rounding scale.

Contents (tensors are concatenated in optimizer order: group 0, then group 1):
  names (json), sizes, p0 (total) f32, grads (12, total) f32, lr (12), mom (12) f64
  p32 m32 v32 (12, total) f32, norm32 (12);  p64 m64 v64 (12, total) f64, norm64 (12);  eref_p eref_m eref_v (12, tensors), eref_norm (12)
  state_ids (json: the parameter indices that have state after the run), state_structure (json: the key structure of state_dict())
  oc_<total>_<pct> (total, 2) f64 [lr, mom] of OneCycle.step(0 .. total - 1), or oc_<total>_<pct>_raises = 1 where the reference raises
  ZeroDivisionError (an empty first phase), with oc_hyper (lr_max, moms, div_factor)
  rcnn_groups (json: two lists of state-dict key names, the reference's groups for its full PointRCNN under cfgs/default.yaml)
  torch_version
The fixture holds only data.
"""
import collections
import collections.abc
import copy
import json
import os
import sys
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_harness as H  # noqa: E402
import optim_batch as OB  # noqa: E402
from make_golden_losses import LIMIT  # noqa: E402

FAIL = ": change the model or the seed"


def reference_optimizer(model, hyper):
    """tools/train_rcnn.py create_optimizer ('adam_onecycle') and create_scheduler on the reference's classes"""
    import torch.nn as nn
    import torch.optim as optim
    from tools.train_utils.fastai_optim import OptimWrapper
    from tools.train_utils import learning_schedules_fastai as lsf
    flatten = lambda m: sum(map(flatten, m.children()), []) if len(list(m.children())) else [m]
    opt = OptimWrapper.create(partial(optim.Adam, betas=(0.9, 0.99)), 3e-3, [nn.Sequential(*flatten(model))], wd=hyper["wd"], true_wd=True,
                              bn_wd=True)
    sched = lsf.OneCycle(opt, hyper["total_steps"], hyper["lr_max"], list(hyper["moms"]), hyper["div_factor"], hyper["pct_start"])
    return opt, sched


def reference_names(model, opt):
    name = {id(p): k for k, p in model.named_parameters()}
    return [[name[id(p)] for p in g["params"]] for g in opt.opt.param_groups]


def one_step(model, opt, sched, k, names, grads, sizes, clip):
    from torch.nn.utils import clip_grad_norm_
    sched.step(k)
    lr, mom = float(opt.lr), float(opt.mom)
    opt.zero_grad()
    OB.set_grads(model, names, grads, sizes)
    norm = float(clip_grad_norm_(model.parameters(), clip))
    opt.step()
    m, v, ids, steps = OB.get_state(opt.state_dict(), names, sizes)
    return lr, mom, norm, OB.get_params(model, names), m, v, ids, steps


def main():
    import torch
    H.install()
    collections.Iterable = collections.abc.Iterable
    from tools.train_utils import learning_schedules_fastai as lsf
    hyper = OB.HYPER
    out = {"seed": np.int64(OB.SEED), "torch_version": np.array(torch.__version__)}

    model = OB.tiny_model()
    opt, sched = reference_optimizer(model, hyper)
    OB.freeze(model)                                                          # after creation, as create_optimizer freezes the RPN
    names, sizes = OB.layout(model)
    assert sum(reference_names(model, opt), []) == names, "the package's groups differ from the reference's on the tiny model"
    assert {1, 3, 15, 64, 65} <= set(sizes) and 190 <= sum(sizes) <= 210, sizes
    grads = OB.make_grads(names, sizes)
    out["names"], out["sizes"] = np.array(json.dumps(names)), np.array(sizes, dtype=np.int64)
    out["p0"], out["grads"] = OB.get_params(model, names).astype(np.float32), grads
    rec = {k: [] for k in ("lr", "mom", "p32", "m32", "v32", "norm32", "p64", "m64", "v64", "norm64", "eref_p", "eref_m", "eref_v", "eref_norm")}
    clipped = []
    for k in range(OB.STEPS):
        before_sd, before_p = copy.deepcopy(opt.state_dict()), OB.get_params(model, names)
        lr, mom, n32, p32, m32, v32, ids, steps = one_step(model, opt, sched, k, names, grads[k], sizes, hyper["grad_norm_clip"])
        model64 = OB.tiny_model(torch.float64)
        opt64, sched64 = reference_optimizer(model64, hyper)
        OB.freeze(model64)
        OB.set_params(model64, names, before_p, sizes)
        opt64.load_state_dict(before_sd)                                      # (casts exp_avg / exp_avg_sq to the parameters' f64)
        lr64, mom64, n64, p64, m64, v64, ids64, steps64 = one_step(model64, opt64, sched64, k, names, grads[k], sizes, hyper["grad_norm_clip"])
        assert (lr, mom, ids, steps) == (lr64, mom64, ids64, steps64) and steps == [k + 1] * len(ids)
        assert ids == [i for i, name in enumerate(names) if OB.has_grad(name)]
        for q, a32, a64 in (("p", p32, p64), ("m", m32, m64), ("v", v32, v64)):
            rec[q + "32"].append(a32.astype(np.float32))
            rec[q + "64"].append(a64)
            rec["eref_" + q].append([float(np.abs(a - b).max()) for a, b in zip(OB.split(a32, sizes), OB.split(a64, sizes))])
        for key, val in (("lr", lr), ("mom", mom), ("norm32", n32), ("norm64", n64), ("eref_norm", abs(n32 - n64))):
            rec[key].append(val)
        clipped.append(n64 + 1e-6 > hyper["grad_norm_clip"])
        print("step %2d lr %.6e mom %.4f norm32 %.9g norm64 %.17g clipped %s" % (k, lr, mom, n32, n64, clipped[-1]))
    assert clipped == [k % 2 == 1 for k in range(OB.STEPS)], "the steps do not alternate unclipped / clipped" + FAIL
    n_near = rec["norm64"][OB.NEAR]
    assert hyper["grad_norm_clip"] - 1e-3 <= n_near and n_near + 1e-6 < hyper["grad_norm_clip"], "the near-clip step" + FAIL
    frozen = [i for i, name in enumerate(names) if name.startswith(OB.FROZEN)]
    for i in frozen:                                                          # never touched
        a, b = np.cumsum([0] + sizes)[i], np.cumsum([0] + sizes)[i + 1]
        assert all(np.array_equal(p[a:b], out["p0"][a:b]) for p in rec["p32"])
    for key, val in rec.items():
        out[key] = np.array(val, dtype=np.float32 if key in ("p32", "m32", "v32") else np.float64)
    sd = opt.state_dict()
    out["state_ids"] = np.array(json.dumps(sorted(sd["state"])))
    out["state_structure"] = np.array(json.dumps({
        "top": sorted(sd), "group_keys": [sorted(g) for g in sd["param_groups"]], "params": [g["params"] for g in sd["param_groups"]],
        "state_keys": {str(i): list(st) for i, st in sd["state"].items()}, "betas2": [g["betas"][1] for g in sd["param_groups"]],
        "weight_decay": [g["weight_decay"] for g in sd["param_groups"]]}))

    # the OneCycle tables
    class Fake:
        lr = mom = 0
    out["oc_hyper"] = np.array([hyper["lr_max"], hyper["moms"][0], hyper["moms"][1], hyper["div_factor"]], dtype=np.float64)
    for total, pct in OB.TABLES:
        fake = Fake()
        s = lsf.OneCycle(fake, total, hyper["lr_max"], list(hyper["moms"]), hyper["div_factor"], pct)
        rows = []
        try:
            for k in range(total):
                s.step(k)
                rows.append((float(fake.lr), float(fake.mom)))
            out["oc_%d_%g" % (total, pct)] = np.array(rows, dtype=np.float64)
        except ZeroDivisionError:
            out["oc_%d_%g_raises" % (total, pct)] = np.int64(1)
        print("OneCycle total %d pct %g:" % (total, pct), "%d rows" % len(rows))

    # the reference's groups for its full PointRCNN
    ref_model, _cfg = H.reference_model()
    ref_opt, _ = reference_optimizer(ref_model, hyper)
    groups = reference_names(ref_model, ref_opt)
    print("PointRCNN groups:", [len(g) for g in groups], "tensors,", sum(p.numel() for p in ref_model.parameters()), "elements")
    out["rcnn_groups"] = np.array(json.dumps(groups))

    path = os.path.join(HERE, "g24_optim_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < LIMIT, "the fixture is not below the generators' size limit"


if __name__ == "__main__":
    main()
