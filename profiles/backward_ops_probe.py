"""Times the backward of grouping (the fused QueryAndGroup form) and three_interpolate at the TRAINING shapes, the atomic entries
against the order-fixed path (csrc/scatter_plan.hip), in one process, alternating:
  atomic   what the autograd Functions run today: zero-fill of the output, for the fused grouping the contiguous copy of
           grad_out[:, 3:], then the atomicAdd kernel (prcnn_group_points_grad / prcnn_three_interpolate_grad)
  plan     prcnn_scatter_plan alone (workspace and output allocation included, as the wrapper does them)
  sum      the ordered sum alone over a plan built before (torch.empty output; grad_out whole, nothing copied)
  both     plan + sum: what ORDERED_BACKWARD costs per backward call
Shapes: the RPN's SA2-SA4 (both scales) and its four FP modules at B = 16 scenes of 16384 points, the RCNN's SA1 / SA2 at 256 RoI
clouds of 512 points (here: the 512 nearest neighbours of 256 random points of the scenes, centred -- local LiDAR density, not the
pooled RoIs of a trained RPN).  Scenes: synth.scenes and synth.lidar_scenes.  Index tensors come from the library's own FPS, ball
query and three_nn.  Per shape the median and the maximum list length of the plan are printed beside the times: the sum pass runs as
long as its most loaded lane.

Device events around each call, WARM warm-up rounds, then the median and the range of REPS calls; the clocks rocm-smi reports are
printed before and after.  Each scene kind is a child process of its own under ``timeout``; a failure ends the run.
    python profiles/backward_ops_probe.py            # both scene kinds: one JSON line per shape, then a markdown table
    python profiles/backward_ops_probe.py lidar      # one step (what the parent starts)
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "3d_adapt_auto_driving_amd"
WARM, REPS = 3, 9
B, ROIS = 16, 256
# (name, source level, centres, radius, nsample, feature channels)
RPN_SA = [("rpn_sa2_s0", 1, 1024, 0.5, 16, 96), ("rpn_sa2_s1", 1, 1024, 1.0, 32, 96), ("rpn_sa3_s0", 2, 256, 1.0, 16, 256),
          ("rpn_sa3_s1", 2, 256, 2.0, 32, 256), ("rpn_sa4_s0", 3, 64, 2.0, 16, 512), ("rpn_sa4_s1", 3, 64, 4.0, 32, 512)]
# (name, unknown level, known level, channels of the interpolated features)
RPN_FP = [("rpn_fp4", 3, 4, 1024), ("rpn_fp3", 2, 3, 512), ("rpn_fp2", 1, 2, 512), ("rpn_fp1", 0, 1, 256)]
RCNN_SA = [("rcnn_sa1", 0, 128, 0.2, 64, 128), ("rcnn_sa2", 1, 32, 0.4, 64, 128)]


def clocks():
    r = subprocess.run("rocm-smi --showclocks 2>/dev/null | grep -i 'sclk\\|mclk' | head -4", shell=True, capture_output=True, text=True)
    return " / ".join(" ".join(ln.split()) for ln in r.stdout.splitlines()) or "rocm-smi reported no clocks"


def pyramid(pu, xyz, counts):
    """[xyz, FPS(xyz, counts[0]), FPS of that, ...]: device tensors (b, n_k, 3)"""
    import torch
    levels = [xyz]
    for m in counts:
        sel = pu.furthest_point_sample(levels[-1], m)
        levels.append(torch.gather(levels[-1], 1, sel.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous())
    return levels


def timed(fns):
    """{name: fn} -> {name: (median, min, max) in us}, alternating the paths, device events around every call"""
    import torch
    times = {k: [] for k in fns}
    for rep in range(WARM + REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= WARM:
                times[k].append(1e3 * a.elapsed_time(b))
    return {k: [float(np.median(v)), min(v), max(v)] for k, v in times.items()}


def list_stats(plan):
    import torch
    lens = (plan.offsets[:, 1:] - plan.offsets[:, :-1]).flatten().float()
    return {"list_median": float(lens.median()), "list_max": int(lens.max()), "list_mean": float(lens.mean())}


def grouping(ops, name, idx, n, c):
    """the fused QueryAndGroup backward: grad_out (b, 3+c, m, ns) -> grad_features (b, c, n)"""
    import torch
    b, m, ns = idx.shape
    grad_out = torch.randn((b, 3 + c, m, ns), device=idx.device)
    plan = ops.scatter_plan_wrapper(idx, n)

    def atomic():
        g = grad_out[:, 3:].contiguous()
        out = torch.zeros((b, c, n), device=idx.device)
        ops.group_points_grad_wrapper(b, c, n, m, ns, g, idx, out)
        return out

    def ordered(pl):
        out = torch.empty((b, c, n), device=idx.device)
        ops.group_points_grad_ordered_wrapper(b, c, n, m * ns, 3 + c, 3, grad_out, pl, out)
        return out
    scale = float(atomic().abs().max())
    assert float((atomic() - ordered(plan)).abs().max()) <= 1e-4 * scale, name          # the same gradient before any time is taken
    t = timed({"atomic": atomic, "plan": lambda: ops.scatter_plan_wrapper(idx, n), "sum": lambda: ordered(plan),
               "both": lambda: ordered(ops.scatter_plan_wrapper(idx, n))})
    return dict(list_stats(plan), shape=name, b=b, c=c, n=n, slots=m * ns, float_adds=b * c * m * ns, us=t)


def interpolate(ops, name, idx, weight, m, c):
    import torch
    b, n, _ = idx.shape
    grad_out = torch.randn((b, c, n), device=idx.device)
    plan = ops.scatter_plan_wrapper(idx, m)

    def atomic():
        out = torch.zeros((b, c, m), device=idx.device)
        ops.three_interpolate_grad_wrapper(b, c, n, m, grad_out, idx, weight, out)
        return out

    def ordered(pl):
        out = torch.empty((b, c, m), device=idx.device)
        ops.three_interpolate_grad_ordered_wrapper(b, c, n, m, grad_out, weight, pl, out)
        return out
    scale = float(atomic().abs().max())
    assert float((atomic() - ordered(plan)).abs().max()) <= 1e-4 * scale, name
    t = timed({"atomic": atomic, "plan": lambda: ops.scatter_plan_wrapper(idx, m), "sum": lambda: ordered(plan),
               "both": lambda: ordered(ops.scatter_plan_wrapper(idx, m))})
    return dict(list_stats(plan), shape=name, b=b, c=c, n=m, slots=3 * n, float_adds=b * c * n * 3, us=t)


def step(kind):
    import torch
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is no other path"
    pu = importlib.import_module(PKG + ".pointnet2.pointnet2_utils")
    synth = importlib.import_module(PKG + ".synth")
    ops = pu.pointnet2
    print(json.dumps({"scenes": kind, "clocks_before": clocks(), "warm": WARM, "reps": REPS}), flush=True)
    host = (synth.lidar_scenes if kind == "lidar" else synth.scenes)(B, 16384, seed0=100)
    levels = pyramid(pu, torch.from_numpy(host).cuda(), [4096, 1024, 256, 64])
    rows = []
    for name, src, m, radius, ns, c in RPN_SA:
        assert levels[src + 1].shape[1] == m
        idx = pu.ball_query(radius, ns, levels[src], levels[src + 1])
        rows.append(grouping(ops, name, idx, levels[src].shape[1], c))
        print(json.dumps(rows[-1]), flush=True)
    for name, unknown, known, c in RPN_FP:
        dist, idx = pu.three_nn(levels[unknown], levels[known])
        inv = 1.0 / (dist + 1e-8)
        rows.append(interpolate(ops, name, idx, (inv / inv.sum(dim=2, keepdim=True)).contiguous(), levels[known].shape[1], c))
        print(json.dumps(rows[-1]), flush=True)
    # RoI-like clouds: the 512 nearest neighbours of 256 random scene points, centred on them
    rng = np.random.default_rng(3)
    clouds = []
    for r in range(ROIS):
        pts = host[r % B]
        centre = pts[rng.integers(len(pts))]
        near = np.argsort(((pts - centre) ** 2).sum(1))[:512]
        clouds.append(pts[near] - centre)
    rl = pyramid(pu, torch.from_numpy(np.stack(clouds).astype(np.float32)).cuda(), [128, 32])
    for name, src, m, radius, ns, c in RCNN_SA:
        idx = pu.ball_query(radius, ns, rl[src], rl[src + 1])
        rows.append(grouping(ops, name, idx, rl[src].shape[1], c))
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"scenes": kind, "clocks_after": clocks()}))
    print("\n| %s scenes | float adds | list median / max | atomic us | plan us | sum us | plan + sum us |\n|---|---|---|---|---|---|---|" % kind)
    fmt = lambda v: "%.0f (%.0f-%.0f)" % tuple(v)
    for r in rows:
        print("| %s | %.1f M | %.0f / %d | %s | %s | %s | %s |" % (r["shape"], r["float_adds"] / 1e6, r["list_median"], r["list_max"],
                                                                 fmt(r["us"]["atomic"]), fmt(r["us"]["plan"]), fmt(r["us"]["sum"]), fmt(r["us"]["both"])))
    sys.stdout.flush()


def main():
    if len(sys.argv) > 1:
        step(sys.argv[1])
        return
    for kind in ("uniform", "lidar"):
        rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), kind])
        if rc != 0:
            sys.exit("step %s ended with status %d: nothing more is started" % (kind, rc))


if __name__ == "__main__":
    main()
