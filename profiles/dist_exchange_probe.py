"""The per-iteration exchange of data-parallel training on ONE MI355X: a world of one rank with every exchange FORCED through RCCL
(dist_train.ReplicaGroup(force=True), backend "nccl"), over the full PointRCNN's parameter tensors (random gradients; no forward runs).

Timed with device events, 3 warm-up rounds, then 9 rounds in which the two paths ALTERNATE; median (min - max) of the 9:
  pack        prcnn_grad_pack: every gradient into the flat bucket, one launch
  bucket      ONE all_reduce of the bucket
  per tensor  the loop this replaces: one all_reduce per gradient tensor, in the same process
  row gather  the rows the RPN loss reads at B = 16 x 16384 (rpn_cls, rpn_reg, rpn_cls_label, rpn_reg_label), gathered by the one function
A world of one measures launch and call overheads and a device-local copy, NOT a link: nothing here says what W > 1 costs.

  python profiles/dist_exchange_probe.py [--out profiles/dist_exchange_probe.md]
"""
import argparse
import ctypes as C
import importlib
import os
import socket
import statistics
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "3d_adapt_auto_driving_amd"
WARMUP, ROUNDS = 3, 9


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                               # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    config, D, O, L = (importlib.import_module(PKG + "." + m) for m in ("config", "dist_train", "optim", "_lib"))
    losses = importlib.import_module(PKG + ".losses")
    PointRCNN = importlib.import_module(PKG + ".net.point_rcnn").PointRCNN
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    group = D.ReplicaGroup(0, 1, dev, "nccl", force=True)
    cfg = config.apply_train_defaults(config.make_cfg(), "rcnn")
    cfg.RPN.FIXED = False                                        # every tensor of both stages gets a gradient
    torch.manual_seed(0)
    model = PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TRAIN").to(dev)
    T = cfg.TRAIN
    opt = O.OneCycleAdam(model, 100, T.LR, list(T.MOMS), T.DIV_FACTOR, T.PCT_START, T.WEIGHT_DECAY, T.GRAD_NORM_CLIP, group=group)
    params = list(model.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    opt.schedule(0)
    opt.step()                                                   # builds the bucket and its table
    t, bucket = opt._table, opt._bucket
    stream = C.c_void_p(L.current_stream(bucket))
    pack = lambda: L.call("prcnn_grad_pack", t["src"], t["numel"], t["slot_start"], t["chunk_tensor"], t["chunk_start"], t["n_tensors"],
                          t["n_chunks"], bucket.data_ptr(), bucket.numel(), stream)
    one = lambda: group.all_reduce_bucket(bucket)
    grads = [p.grad for p in params]

    def per_tensor():
        for g in grads:
            dist.all_reduce(g)
    B, N, ch = 16, 16384, losses.rpn_spec(cfg).channels
    rows = {"rpn_cls": torch.randn(B, N, 1, device=dev), "rpn_reg": torch.randn(B, N, ch, device=dev),
            "rpn_cls_label": torch.zeros(B, N, dtype=torch.int64, device=dev), "rpn_reg_label": torch.randn(B, N, 7, device=dev)}
    row_bytes = sum(v.numel() * v.element_size() for v in rows.values())
    gather = lambda: group.gather_rows(rows)
    legs = [("pack (1 launch)", pack), ("bucket all_reduce (1 call)", one), ("per-tensor all_reduce (%d calls)" % len(grads), per_tensor),
            ("row gather, B = 16 x 16384", gather)]
    times = {name: [] for name, _ in legs}
    for r in range(WARMUP + ROUNDS):
        order = legs if r % 2 == 0 else legs[::-1]               # the paths alternate
        for name, fn in order:
            torch.cuda.synchronize()
            us = timed(fn)
            if r >= WARMUP:
                times[name].append(us)
    dist.barrier(device_ids=[0])
    group.close()
    lines = ["# The exchange of data-parallel training on one MI355X (world 1, forced through RCCL)", "",
             "`python profiles/dist_exchange_probe.py`: %d parameter tensors, %d elements, a bucket of %d elements (%.1f MB), %d chunks; "
             "the RPN rows at B = 16 x 16384 are %.1f MB.  Device events, %d warm-up rounds, median (min - max) of %d rounds, the paths "
             "alternating.  A world of one measures launch and call overheads and a device-local copy, not a link: no number here "
             "says what W > 1 costs." % (len(params), sum(p.numel() for p in params), bucket.numel(), bucket.numel() * 4 / 1e6,
                                          t["n_chunks"], row_bytes / 1e6, WARMUP, ROUNDS), "",
             "| leg | us, median (min - max) |", "|---|---|"]
    for name, _ in legs:
        v = times[name]
        lines.append("| %s | %.1f (%.1f - %.1f) |" % (name, statistics.median(v), min(v), max(v)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
