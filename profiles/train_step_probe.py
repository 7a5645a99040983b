"""Times the weight step (3d_adapt_auto_driving_amd/optim.py OneCycleAdam.step(), csrc/optim.hip) on the full PointRCNN's parameter
list -- 142 tensors, 3 887 452 elements, seeded grads resident on the device -- against the reference's sequence on the SAME CUDA
tensors: torch.nn.utils.clip_grad_norm_, the wrapper's per-parameter ``p.data.mul_(1 - wd lr)`` loop and torch.optim.Adam as torch
configures it by default (what a user of the reference runs today).
  step      fused    OneCycleAdam.step(): three launches
            torch    the reference's sequence
            both in one process, alternating, every repetition ended by a synchronize: median of REPS after WARM warm-up rounds, with
            the range.  (The torch sequence scales the grads in place; the fused step never writes them.  The values do not change
            the work of either.)
  launches  the device kernels each launches per step, counted with torch.profiler (a run of its own: tracing slows the host)
  split     one training iteration of the RPN at B = 16 x 16384 points split into input (RpnTrainInput.batch on a small labelled tree,
            scenes repeated to 16), forward, loss (losses.rpn_loss and its tb_dict read), backward and step: median of 3 after 1 warm-up

Every step is a child process of its own under ``timeout``; its exit status is checked and a failure ends the run.
    python profiles/train_step_probe.py            # all steps, one JSON line each
    python profiles/train_step_probe.py step       # one step (what the parent starts)
"""
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "3d_adapt_auto_driving_amd"
WARM, REPS = 3, 7
HYPER = dict(total_steps=1000, lr_max=0.002, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4, wd=0.001, grad_norm_clip=1.0)


def stats(v):
    return {"us_median": 1e6 * float(np.median(v)), "us_min": 1e6 * min(v), "us_max": 1e6 * max(v)}


def full_model(mode="rcnn"):
    import torch
    C = importlib.import_module(PKG + ".config")
    cfg = C.apply_train_defaults(C.make_cfg(), mode)
    torch.manual_seed(0)
    model = importlib.import_module(PKG + ".net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN").cuda()
    return cfg, model


def setup():
    """-> {"fused": fn, "torch": fn}, info: two copies of the model's parameters, each with its own optimizer and the same grads"""
    import copy
    import torch
    from torch.nn.utils import clip_grad_norm_
    O = importlib.import_module(PKG + ".optim")
    _cfg, model = full_model()
    twin = copy.deepcopy(model)
    g = torch.Generator(device="cuda").manual_seed(1)
    for p, q in zip(model.parameters(), twin.parameters()):
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 0.01
        q.grad = p.grad.clone()
    opt = O.OneCycleAdam(model, **HYPER)
    opt.schedule(400)
    groups = O.layer_groups(twin)
    adam = torch.optim.Adam([{"params": grp, "lr": opt.lr} for grp in groups], betas=(opt.mom, 0.99))
    params = list(twin.parameters())

    def torch_sequence():
        clip_grad_norm_(params, HYPER["grad_norm_clip"])
        for grp in adam.param_groups:
            for p in grp["params"]:
                p.data.mul_(1 - HYPER["wd"] * opt.lr)
        adam.step()
    info = {"tensors": len(params), "elements": sum(p.numel() for p in params), "foreach": adam.param_groups[0]["foreach"]}
    return {"fused": opt.step, "torch": torch_sequence}, info


def time_step():
    import torch
    paths, info = setup()
    times = {k: [] for k in paths}
    for rep in range(WARM + REPS):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARM:
                times[k].append(time.perf_counter() - t0)
    print(json.dumps(dict(info, step="step", reps=REPS, **{k: stats(v) for k, v in times.items()})))


def count_step():
    import torch
    from torch.profiler import ProfilerActivity, profile
    paths, _info = setup()
    out = {"step": "launches"}
    for k, fn in paths.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        out[k] = {"device_events": len(names), "memcpy_or_memset": sum("mem" in x.lower() for x in names), "distinct": len(set(names))}
    print(json.dumps(out))


def split_step():
    import torch
    import train_tree
    O, L = importlib.import_module(PKG + ".optim"), importlib.import_module(PKG + ".losses")
    G, T = importlib.import_module(PKG + ".gt_database"), importlib.import_module(PKG + ".train_input")
    cfg, model = full_model("rpn")
    cfg["GT_AUG_ENABLED"], cfg["GT_AUG_RAND_NUM"], cfg["GT_AUG_APPLY_PROB"] = True, True, 1.0
    model.train()
    opt = O.OneCycleAdam(model, **HYPER)
    B, N = 16, cfg.RPN.NUM_POINTS
    with tempfile.TemporaryDirectory() as root:
        train_tree.write_train_tree(root)
        G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cpu", log=lambda *a: None)
        src = T.RpnTrainInput(root, cfg, G.database_file_name(os.path.join(root, "db"), "train", "Car"), split=train_tree.SPLIT, npoints=N,
                              npoints_faraway=4000, seed=0, device="cuda")
        names = ("input", "forward", "loss", "backward", "step")
        times = {k: [] for k in names}
        for rep in range(1 + 3):
            marks = []

            def mark():
                torch.cuda.synchronize()
                marks.append(time.perf_counter())
            opt.schedule(400 + rep)
            opt.zero_grad()
            mark()
            batch = src.batch([k % len(src) for k in range(B)])
            mark()
            ret = model({"pts_input": batch["pts_input"], "gt_boxes3d": batch["gt_boxes3d"]})
            mark()
            res = L.rpn_loss(cfg, ret["rpn_cls"], ret["rpn_reg"], batch["rpn_cls_label"], batch["rpn_reg_label"])
            tb = res.tb_dict()
            mark()
            res.loss.backward()
            mark()
            opt.step()
            mark()
            if rep:
                for k, a, b in zip(names, marks[:-1], marks[1:]):
                    times[k].append(b - a)
    print(json.dumps({"step": "split", "batch": B, "points": N, "rpn_loss": tb["rpn_loss"], "stages": {k: stats(v) for k, v in times.items()}}))


def main():
    steps = {"step": time_step, "launches": count_step, "split": split_step}
    if len(sys.argv) > 1:
        steps[sys.argv[1]]()
        return
    for step, limit in (("step", 240), ("launches", 240), ("split", 420)):
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step])
        if rc != 0:
            sys.exit("step %s ended with status %d: nothing more is started" % (step, rc))


if __name__ == "__main__":
    main()
