"""Data-parallel training on the device: prcnn_grad_pack and prcnn_param_digest (csrc/grad_bucket.hip) at the sizes where they can go
wrong, OneCycleAdam(group=...) against the plain device optimizer, the exchanges through RCCL at a world of one, a world of two sharing
cuda:0 over gloo, and the train loop's command line under a launcher's variables.  Every comparison is bit for bit: a pack is a copy, the
digest is integer arithmetic, and a two-term f32 sum is commutative.  At most this process and two children hold the GPU; every child is
a fresh process with its own time limit, and a test ends on its first failure."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dist_replica as DR  # noqa: E402
import optim_batch as OB  # noqa: E402
import train_tree  # noqa: E402
import dist_train_child as CH  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = OB.PKG
CHILD = os.path.join(HERE, "dist_train_child.py")


def _lib():
    return OB.importlib.import_module(PKG + "._lib")


def sizes():
    c = OB.O().CHUNK
    return [1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 5]


def make_table(tensors):
    """The pack / digest table of a list of CUDA tensors (None: no slot) -> (addresses, n_tensors, n_chunks, slot_start, total, buffer)"""
    O, D = OB.O(), DR.D()
    has = [i for i, t in enumerate(tensors) if t is not None]
    starts, total = D.bucket_layout([tensors[i].numel() for i in has])
    slot = np.zeros(len(tensors), dtype=np.int64)
    slot[has] = starts
    numel = np.array([0 if t is None else t.numel() for t in tensors], dtype=np.int64)
    addr = np.array([0 if t is None else t.data_ptr() for t in tensors], dtype=np.uint64)
    chunk_tensor, chunk_start = O.chunks_of(numel, addr != 0)
    buf, at = O.upload_sections([("src", addr), ("numel", numel), ("slot_start", slot), ("chunk_start", chunk_start),
                                 ("chunk_tensor", chunk_tensor)], "cuda")
    return at, len(tensors), len(chunk_tensor), slot, total, buf


def test_grad_pack_equals_cat_bit_for_bit():
    L = _lib()
    g = torch.Generator().manual_seed(11)
    c = OB.O().CHUNK
    grads = [torch.randn(n, generator=g).cuda() for n in sizes()]
    grads.insert(2, None)                                                        # no grad: no slot
    wide = torch.randn(40, 2 * 33, generator=g).cuda()
    strided = wide[:, ::2]                                                       # non-contiguous: the caller's copy is packed
    assert not strided.is_contiguous()
    grads.append(strided.contiguous())
    big = torch.randn(c + 70, generator=g).cuda()
    view = big[1:1 + c + 1]                                                      # starts at element 1: one whole chunk off 16 bytes + a tail
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    grads.append(view)
    at, nt, nc, slot, total, _buf = make_table(grads)
    bucket = torch.zeros(total, device="cuda")
    stream = C.c_void_p(L.current_stream(bucket))
    want = torch.zeros(total)
    for t, s in zip(grads, slot):
        if t is not None:
            want[int(s):int(s) + t.numel()] = t.reshape(-1).cpu()
    pad = torch.ones(total, dtype=torch.bool)
    for t, s in zip(grads, slot):
        if t is not None:
            pad[int(s):int(s) + t.numel()] = False
    assert int(pad.sum()) > 0
    for _ in range(2):                                                           # twice: padding words stay zero
        L.call("prcnn_grad_pack", at["src"], at["numel"], at["slot_start"], at["chunk_tensor"], at["chunk_start"], nt, nc,
               bucket.data_ptr(), total, stream)
        got = bucket.cpu()
        assert got.numpy().tobytes() == want.numpy().tobytes()
        assert bool((got[pad] == 0).all())
    live = torch.cat([t.reshape(-1) for t in grads if t is not None]).cpu()
    assert torch.equal(got[~pad], live)                                          # the slots in table order are torch.cat of the grads
    args = [at["src"], at["numel"], at["slot_start"], at["chunk_tensor"], at["chunk_start"], nt, nc, bucket.data_ptr(), total, stream]
    for k in (0, 1, 2, 3, 4, 7):
        bad = list(args)
        bad[k] = None
        with pytest.raises(L.PrcnnError, match="grad_pack"):
            L.call("prcnn_grad_pack", *bad)
    for k, v in ((5, 0), (6, 0), (6, -3), (8, 0)):
        bad = list(args)
        bad[k] = v
        with pytest.raises(L.PrcnnError, match="grad_pack"):
            L.call("prcnn_grad_pack", *bad)
    bad = list(args)
    bad[7] = bucket.data_ptr() + 4                                               # the bucket itself must be 16-byte aligned
    with pytest.raises(L.PrcnnError, match="grad_pack"):
        L.call("prcnn_grad_pack", *bad)
    torch.cuda.synchronize()


def test_param_digest_equals_the_numpy_definition():
    D, L = DR.D(), _lib()
    g = torch.Generator().manual_seed(12)
    host = [torch.randn(n, generator=g) for n in sizes()]
    dev = [t.cuda() for t in host]
    want = D.host_digest([t.numpy() for t in host])
    assert D.device_digest(dev) == want and D.digest(dev) == want
    bits = host[-1].numpy().copy()
    bits.view(np.uint32)[-1] ^= 1                                                # one mantissa bit of the last element of the last tensor
    dev[-1] = torch.from_numpy(bits).cuda()
    flipped = D.device_digest(dev)
    assert flipped != want and flipped == D.host_digest([t.numpy() for t in host[:-1]] + [bits])
    with pytest.raises(L.PrcnnError, match="param_digest"):
        L.call("prcnn_param_digest", None, None, None, None, None, 1, 1, None, None)
    with pytest.raises(L.PrcnnError, match="param_digest"):
        L.call("prcnn_param_digest", 8, 8, 8, 8, 8, 1, 0, 8, None)


def _device_run(group, steps, z, names, sizes_):
    model = OB.tiny_model().to("cuda")
    OB.set_params(model, names, z["p0"], sizes_)
    opt = OB.O().OneCycleAdam(model, group=group, **OB.HYPER)
    OB.freeze(model)                                                             # after the optimizer is built, as OB.fresh does
    out = []
    for k in range(steps):
        opt.schedule(k)
        if k == 0:
            OB.set_grads(model, names, z["grads"][0], sizes_)
        else:                                                                    # in place: the grads keep their addresses
            named = dict(model.named_parameters())
            for name, v in zip(names, OB.split(z["grads"][k], sizes_)):
                if OB.has_grad(name):
                    named[name].grad.copy_(torch.from_numpy(np.array(v)).reshape(named[name].shape))
        opt.step()
        out.append(DR.snapshot(model, opt, None))
    return opt, out


def test_world1_forced_exchange_equals_the_plain_device_optimizer(monkeypatch):
    D = DR.D()
    z, names, sizes_ = OB.load_fixture()
    _plain, want = _device_run(None, 3, z, names, sizes_)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(DR.free_port()))
    group = D.ReplicaGroup(0, 1, "cuda:0", "gloo", force=True)
    try:
        assert group.active
        opt, got = _device_run(group, 3, z, names, sizes_)
    finally:
        group.close()
    for k in range(3):
        assert DR.same_snapshot(want[k], got[k]) == [], k
    assert opt.table_uploads == 1 and opt.steps_done == 3                        # the table is uploaded once, not per step
    assert opt._bucket.numel() % 64 == 0 and _plain.table_uploads == 1


def _child(args, env=None, timeout=240):
    return subprocess.Popen([sys.executable] + args, cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True), timeout


def _finish(procs):
    """Waits for every child under its own time limit; the first failure ends the others"""
    outs = []
    try:
        for p, timeout in procs:
            out, err = p.communicate(timeout=timeout)
            assert p.returncode == 0, out[-2000:] + err[-4000:]
            outs.append(out + err)
    finally:
        for p, _t in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return outs


def test_world1_exchanges_through_rccl_in_a_child():
    out = _finish([_child([CHILD, "nccl1"])])[0]
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert line == {"ok": True, "backend": "nccl"}


def test_world2_sharing_one_gpu_equals_one_step_on_the_summed_gradients(tmp_path):
    port = DR.free_port()
    files = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    procs = [_child([CHILD, "step2", str(r), str(port), files[r]]) for r in range(2)]
    model = OB.tiny_model().cuda()                                               # meanwhile: the single-process step on g_0 + g_1
    names, sizes_ = OB.layout(model)
    total = int(sum(sizes_))
    opt = OB.O().OneCycleAdam(model, **OB.HYPER)
    OB.freeze(model)
    opt.schedule(0)
    OB.set_grads(model, names, CH.step_grads(total, 0) + CH.step_grads(total, 1), sizes_)
    opt.step()
    want = DR.snapshot(model, opt, None)
    digest = DR.D().digest(list(model.parameters()))
    _finish(procs)
    for r in range(2):
        got = dict(np.load(files[r]))
        assert int(got["digest"][0]) == digest, r
        assert float(got["total_norm"][0]) == want["total_norm"] and want["total_norm"] > 1.0
        for key in ("params", "exp_avg", "exp_avg_sq", "steps"):
            assert sorted("%s/%s" % (key, k) for k in want[key]) == sorted(k for k in got if k.startswith(key + "/"))
            for k, v in want[key].items():
                assert np.asarray(v).tobytes() == got["%s/%s" % (key, k)].tobytes(), (r, key, k)


def test_command_line_two_ranks_train_checkpoint_and_resume(tmp_path):
    import yaml
    from test_host_logic import TINY
    G = OB.importlib.import_module(PKG + ".gt_database")
    conf = OB.importlib.import_module(PKG + ".config")
    root = str(tmp_path / "tree")
    os.makedirs(root)
    train_tree.write_train_tree(root)
    G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cpu", log=lambda *a: None)
    db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
    over = {"RPN": dict(TINY["RPN"], NUM_POINTS=train_tree.NPOINTS), "TRAIN": {"SPLIT": train_tree.SPLIT, "PCT_START": 0.5}}
    cfg_file = str(tmp_path / "tiny.yaml")
    with open(cfg_file, "w") as f:
        yaml.safe_dump(over, f)
    outs = [str(tmp_path / ("out%d" % r)) for r in range(2)]

    def launch(extra):
        port = DR.free_port()
        procs = []
        for r in range(2):
            env = dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0")
            procs.append(_child(["-m", PKG + ".train_rcnn", "--train_mode", "rpn", "--root", root, "--gt_database", db, "--cfg_file", cfg_file,
                                 "--batch_size", "2", "--ckpt_save_interval", "1", "--npoints_faraway", str(train_tree.NPOINTS_FARAWAY),
                                 "--output_dir", outs[r], "--seed", "1", "--dist_backend", "gloo"] + extra, env, timeout=420))
        return _finish(procs)

    launch(["--epochs", "1"])
    ckpt = os.path.join(outs[0], "ckpt", "checkpoint_epoch_1.pth")
    assert os.path.isfile(ckpt) and not os.path.exists(outs[1])                  # rank 1 wrote no file
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert saved["it"] == 3 and saved["epoch"] == 1 and sorted(saved) == ["epoch", "it", "model_state", "optimizer_state"]
    with open(os.path.join(outs[0], "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["it"] for ln in lines] == [1, 2, 3]
    assert all(np.isfinite(ln["loss"]) and np.isfinite(ln["grad_norm"]) and np.isfinite(ln["rpn_loss"]) for ln in lines)
    with open(os.path.join(outs[0], "log_train.txt")) as f:
        text = f.read()
    assert len([ln for ln in text.splitlines() if "world_size 2 backend gloo" in ln]) == 1
    cfg = conf.apply_train_defaults(conf.make_cfg(), "rpn")
    conf.merge_into(over, cfg)
    model = OB.importlib.import_module(PKG + ".net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TEST")
    assert OB.importlib.import_module(PKG + ".eval_rcnn").load_checkpoint(model, ckpt) == 1
    out = launch(["--epochs", "2", "--ckpt", ckpt])
    assert "resumed at epoch 1, it 3" in out[0]
    again = torch.load(os.path.join(outs[0], "ckpt", "checkpoint_epoch_2.pth"), map_location="cpu", weights_only=False)
    assert again["it"] == 6 and not os.path.exists(outs[1])
