"""Child process of tests/test_gpu_dist_train.py (the pattern of rccl_world1_child.py): one rank of a data-parallel world on cuda:0.

  dist_train_child.py nccl1                       a world of ONE over "nccl" (= RCCL), the exchanges FORCED through it: the bucket
                                                  all-reduce and the row gather (with its backward) on HIP tensors equal their inputs
  dist_train_child.py step2 RANK PORT OUT.npz     one rank of a world of TWO over gloo, both ranks on cuda:0 (the exchange buffers are
                                                  staged through host copies): seeded gradients on optim_batch's tiny model, one dist
                                                  step(), the snapshot and the parameter digest -> OUT.npz
Prints one JSON line {"ok": true, ...}."""
import importlib
import json
import os
import socket
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

PKG = "3d_adapt_auto_driving_amd"


def step_grads(total, rank):
    """Rank ``rank``'s seeded gradients for the tiny model, concatenated in optimizer order"""
    return (np.random.RandomState(900 + rank).standard_normal(total) * 0.5).astype(np.float32)


def nccl1():
    import torch.distributed as dist
    D = importlib.import_module(PKG + ".dist_train")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    group = D.ReplicaGroup(0, 1, dev, "nccl", force=True)
    assert group.active and dist.get_backend() == "nccl"
    g = torch.Generator().manual_seed(4)
    bucket = torch.randn(3 * 2048 + 64, generator=g).to(dev)
    want = bucket.clone()
    group.all_reduce_bucket(bucket)
    assert bucket.is_cuda and torch.equal(bucket, want), "the all-reduce of one rank changed the bucket"
    rows = {"rpn_cls": torch.randn(2, 96, 1, generator=g).to(dev).requires_grad_(True), "rpn_reg": torch.randn(2, 96, 5, generator=g).to(dev).requires_grad_(True),
            "rpn_cls_label": torch.randint(-1, 2, (2, 96), generator=g).to(dev), "rpn_reg_label": torch.randn(2, 96, 7, generator=g).to(dev)}
    out = group.gather_rows(rows)
    for k, v in rows.items():
        assert out[k].is_cuda and out[k] is not v and torch.equal(out[k], v), k
    w = torch.randn(2, 96, 5, generator=g).to(dev)
    ((out["rpn_reg"] * w).sum() + out["rpn_cls"].sum()).backward()
    assert torch.equal(rows["rpn_reg"].grad, w) and torch.equal(rows["rpn_cls"].grad, torch.ones_like(rows["rpn_cls"]))
    assert not out["rpn_cls_label"].requires_grad
    p = [torch.randn(65, generator=g).to(dev), torch.randn(2049, generator=g).to(dev)]
    assert group.digest_check(p) == D.host_digest([t.cpu().numpy() for t in p])
    dist.barrier(device_ids=[0])
    group.close()
    print(json.dumps({"ok": True, "backend": "nccl"}))


def step2(rank, port, out_file):
    import dist_replica as DR
    import optim_batch as OB
    D = importlib.import_module(PKG + ".dist_train")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    group = D.ReplicaGroup.from_env("cuda", "gloo")
    assert group.active and group.device == torch.device("cuda", 0) and group.backend == "gloo"
    model = OB.tiny_model().to(group.device)
    names, sizes = OB.layout(model)
    opt = OB.O().OneCycleAdam(model, group=group, **OB.HYPER)
    OB.freeze(model)
    opt.schedule(0)
    OB.set_grads(model, names, step_grads(int(sum(sizes)), rank), sizes)
    own = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    opt.step()
    assert all(torch.equal(p.grad, own[k]) for k, p in model.named_parameters() if p.grad is not None), "p.grad is the rank's own"
    digest = group.digest_check(model.parameters())
    snap = DR.snapshot(model, opt, None)
    flat = {"digest": np.array([digest], dtype=np.uint64), "total_norm": np.array([snap["total_norm"]])}
    for key in ("params", "exp_avg", "exp_avg_sq", "steps"):
        flat.update({"%s/%s" % (key, k): np.asarray(v) for k, v in snap[key].items()})
    np.savez(out_file, **flat)
    group.close()
    print(json.dumps({"ok": True, "rank": rank, "digest": "%016x" % digest}))


if __name__ == "__main__":
    if sys.argv[1] == "nccl1":
        nccl1()
    elif sys.argv[1] == "step2":
        step2(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
    else:
        raise SystemExit("dist_train_child.py: unknown mode %r" % sys.argv[1])
