"""Times forward plus backward of each stage's training loss (3d_adapt_auto_driving_amd/losses.py) at two shapes:
  rpn    the workload's own RPN shape, B 16 x 16384 points x C 76 (LOC_XZ_FINE, SigmoidFocalLoss), 5 % foreground points
  rcnn   4 x 64 RoIs x C 46 (BinaryCrossEntropy, the library defaults), about half of them regression rows
each against the same formulas run as torch operators on the device (losses._stage_cpu applied to the device tensors: what a user of
the reference has today, its host read of the foreground count included).
  kernels   the HIP path: one autograd Function, four launches forward
  torch_ops the operator path
Both are timed in the same process, alternating, inputs resident, every repetition ended by a synchronize: median of REPS after WARM
warm-up rounds, with the range.  A third step counts the device kernels each path launches per forward + backward with torch.profiler
(a run of its own: tracing slows the host).

Every step is a child process of its own under ``timeout``; its exit status is checked and a failure ends the run.
    python profiles/losses_probe.py            # all steps, one JSON line each
    python profiles/losses_probe.py rpn        # one step (what the parent starts)
"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARM, REPS = 5, 30
SHAPES = {"rpn": ("rpn_focal_c76", 16 * 16384, 0.05), "rcnn": ("rcnn_bce_c46", 4 * 64, 0.25)}


def setup(step):
    import torch
    import losses_batch as LB
    L = importlib.import_module("3d_adapt_auto_driving_amd.losses")
    name, n, share = SHAPES[step]
    spec, stage = LB.case_spec(name), LB.CASES[name][0]
    b = LB.make_batch(stage, "mixed", spec.channels, n=n, seed=5, fg_share=share)
    t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
    cls, reg = t["cls"].clone().requires_grad_(True), t["reg"].clone().requires_grad_(True)
    anchors = t["roi"] if spec.anchor_on_roi else None

    def kernels():
        res = L._stage(spec, cls, reg, t["label"], t.get("reg_mask"), t["reg_label"], anchors)
        return torch.autograd.grad(res.loss, [cls, reg])

    def torch_ops():
        loss, _parts = L._stage_cpu(spec, cls, reg, t["label"], t.get("reg_mask"), t["reg_label"], anchors)
        return torch.autograd.grad(loss, [cls, reg])
    fg = int((t["reg_mask"] > 0).sum()) if "reg_mask" in t else int((t["label"] > 0).sum())
    return {"kernels": kernels, "torch_ops": torch_ops}, {"rows": n, "channels": spec.channels, "cls": spec.cls_kind, "fg_rows": fg}


def time_step(step):
    import torch
    paths, info = setup(step)
    times = {k: [] for k in paths}
    for rep in range(WARM + REPS):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARM:
                times[k].append(time.perf_counter() - t0)
    out = dict(info, step=step, reps=REPS)
    for k, v in times.items():
        out[k] = {"us_median": 1e6 * float(np.median(v)), "us_min": 1e6 * min(v), "us_max": 1e6 * max(v)}
    print(json.dumps(out))


def count_step():
    import torch
    from torch.profiler import ProfilerActivity, profile
    out = {"step": "launches"}
    for step in SHAPES:
        paths, _info = setup(step)
        for k, fn in paths.items():
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
            out["%s_%s" % (step, k)] = {"device_events": len(names), "memcpy_or_memset": sum("mem" in x.lower() for x in names)}
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1:
        count_step() if sys.argv[1] == "launches" else time_step(sys.argv[1])
        return
    for step, limit in (("rpn", 240), ("rcnn", 180), ("launches", 240)):
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), step])
        if rc != 0:
            sys.exit("step %s ended with status %d: nothing more is started" % (step, rc))


if __name__ == "__main__":
    main()
