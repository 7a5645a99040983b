"""The weight step on the device (optim.OneCycleAdam on CUDA parameters, csrc/optim.hip) against fixture g24 (the reference's own
OptimWrapper + OneCycle + clip_grad_norm_, teacher-forced), against the package's cpu path at the shapes where the kernels can go wrong,
end to end through a small RCNNNet, and the train loop's command line in a child process.

Bound (tests/losses_batch.py tolerance, the g23 rule): every tensor and quantity within 8 x its own e_ref of the f64 result, 4 ulp (f32)
at the tensor's largest magnitude where e_ref is 0.  Against g24 e_ref is recorded (|ref32 - ref64| of the reference's own runs);
without a fixture it is taken from the cpu path run in f32 and in f64 on the same inputs.  Every comparison is ONE STEP DEEP, as in g24:
the f64 step and the device step both start from the f32 run's state before that step.  That is what makes the rule meaningful for a
tensor of one element, where e_ref is a single draw: the device result is the f64 value rounded to f32 once, so no other f32 number --
the f32 run's result among them -- lies closer to it, and err <= e_ref up to the f64 arithmetic's own error.  Over several free-running
steps the f64 run keeps unrounded state and the comparison would measure the f32 STORAGE of the state, not the step."""
import copy
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
import optim_batch as OB  # noqa: E402
import losses_batch as LB  # noqa: E402
import rcnn_targets_batch as RB  # noqa: E402
import train_tree  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = OB.PKG


def test_device_path_teacher_forced_through_g24():
    assert OB.teacher_forced("cuda") == []


# ------------------------------------------------------------------------------------------------------------------------ the sweep
class Bag(torch.nn.Module):
    """a leaf module of plain parameters (all in group 0); ``offset``: that tensor is a view 4 bytes into its storage"""

    def __init__(self, values, device, dtype, offset=None, frozen=(), nograd=()):
        super().__init__()
        self.nograd = set(nograd)
        for k, v in enumerate(values):
            t = torch.from_numpy(np.array(v)).to(device=device, dtype=dtype)       # (a copy: the step works in place)
            if k == offset:
                store = torch.empty(t.numel() + 1, device=device, dtype=dtype)
                store[1:].copy_(t)
                t = store[1:]
            self.register_parameter("t%d" % k, torch.nn.Parameter(t))
        self.frozen = frozen

    def freeze(self):
        for k in self.frozen:
            getattr(self, "t%d" % k).requires_grad = False

    def tensors(self):
        return [getattr(self, "t%d" % k) for k in range(len(self._parameters))]

    def set_grads(self, grads):
        for k, (p, g) in enumerate(zip(self.tensors(), grads)):
            p.grad = None if (k in self.frozen or k in self.nograd) else torch.from_numpy(np.array(g)).to(device=p.device, dtype=p.dtype)


def sweep_sizes():
    C = OB.O().CHUNK
    rng = np.random.RandomState(7)
    return [1, 3, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 3] + [int(n) for n in rng.randint(1, 8, size=300)]


def sweep_inputs(sizes, steps, norms, seed=11):
    rng = np.random.RandomState(seed)
    values = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    grads = []
    for k in range(steps):
        g = [rng.standard_normal(n) for n in sizes]
        scale = norms[k] / np.sqrt(sum((x * x).sum() for x in g))
        grads.append([(x * scale).astype(np.float32) for x in g])
    return values, grads


def force(model, opt, prev, k):
    """parameters and optimizer state <- a recorded step's (through load_state_dict, in the layout state_dict() gives)"""
    p, m, v, _norm, ids = prev
    ts = model.tensors()
    conv = lambda x, t: torch.from_numpy(np.array(x)).to(device=t.device, dtype=t.dtype)
    with torch.no_grad():
        for t, x in zip(ts, p):
            t.copy_(conv(x, t))
    state = {i: {"step": torch.tensor(float(k)), "exp_avg": conv(m[i], ts[i]), "exp_avg_sq": conv(v[i], ts[i])} for i in ids}
    opt.load_state_dict({"state": state, "param_groups": opt.state_dict()["param_groups"]})


def run_bag(device, dtype, values, grads, hyper, forced=None, **bag):
    """-> per step ([p], [m], [v] as f64 numpy per tensor, total_norm, the indices with state), and the last (model, optimizer).
    ``forced``: another run's output; step k then starts from that run's state after step k - 1 (teacher forcing)"""
    model = Bag(values, device, dtype, **bag)
    opt = OB.O().OneCycleAdam(model, **hyper)
    model.freeze()
    out = []
    for k, g in enumerate(grads):
        if forced is not None and k:
            force(model, opt, forced[k - 1], k)
        opt.schedule(k)
        opt.zero_grad()
        model.set_grads(g)
        opt.step()
        sd = opt.state_dict()["state"]
        host = lambda t: t.detach().cpu().double().numpy().reshape(-1).copy()
        zeros = [np.zeros(p.numel()) for p in model.tensors()]
        m, v = list(zeros), list(zeros)
        for i, st in sd.items():
            m[i], v[i] = host(st["exp_avg"]), host(st["exp_avg_sq"])
            assert float(st["step"]) == k + 1
        out.append(([host(p) for p in model.tensors()], m, v, float(opt.total_norm), sorted(sd)))
    return out, model, opt


def compare_runs(dev, ref32, ref64, tag):
    """the rule of the module docstring per step, tensor and quantity; prints the worst figure per step and quantity"""
    bad = []
    for k, (d, a, b) in enumerate(zip(dev, ref32, ref64)):
        assert d[4] == a[4] == b[4], "state exists for other tensors"
        for q, name in enumerate(("p", "m", "v")):
            worst = (0.0, None)
            for i, (x, r32, r64) in enumerate(zip(d[q], a[q], b[q])):
                e_ref = float(np.abs(r32 - r64).max())
                err, tol = float(np.abs(x - r64).max()), LB.tolerance(e_ref, float(np.abs(r64).max()))
                if not err <= tol:
                    bad.append((k, name, i, err, e_ref, tol))
                if tol > 0 and err / tol >= worst[0]:
                    worst = (err / tol, (i, x.size, err, e_ref, tol))
            print("%s step %d %s worst err / tol %.3f at (tensor, numel, err, e_ref, tol) %s" % ((tag, k, name) + worst))
        e_ref = abs(a[3] - b[3])
        err, tol = abs(d[3] - b[3]), LB.tolerance(e_ref, b[3])
        print("%s step %d norm device %.17g ref64 %.17g err %.3e e_ref %.3e" % (tag, k, d[3], b[3], err, e_ref))
        if not err <= tol:
            bad.append((k, "norm", err, e_ref, tol))
    return bad


SWEEP_HYPER = dict(total_steps=3, lr_max=0.002, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4, wd=0.001, grad_norm_clip=1.0)


def test_shape_sweep_against_the_cpu_path():
    sizes = sweep_sizes()
    C = OB.O().CHUNK
    values, grads = sweep_inputs(sizes, 3, (0.5, 30.0, 0.9))
    bag = dict(offset=sizes.index(C + 1), frozen=(20,), nograd=(21,))
    ref32, _m, _o = run_bag("cpu", torch.float32, values, grads, SWEEP_HYPER, **bag)
    dev, model, opt = run_bag("cuda", torch.float32, values, grads, SWEEP_HYPER, forced=ref32, **bag)
    assert model.tensors()[sizes.index(C + 1)].data_ptr() % 16 == 4
    assert opt._table["n_chunks"] == sum(-(-n // C) for k, n in enumerate(sizes) if k != 20) > len(sizes)
    ref64, _m, _o = run_bag("cpu", torch.float64, values, grads, SWEEP_HYPER, forced=ref32, **bag)
    assert compare_runs(dev, ref32, ref64, "sweep") == []
    for p, g in zip(model.tensors(), grads[-1]):                             # grads are read, never written: the unclipped grad
        if p.grad is not None:
            assert np.array_equal(p.grad.cpu().numpy(), g)


# ------------------------------------------------------------------------------------------------------------------------ the flags
def test_flags_frozen_untouched_nograd_decayed_and_the_clip_below_its_value():
    z, names, sizes = OB.load_fixture()
    at = np.cumsum([0] + sizes)
    k = OB.NEAR
    results = []
    for clip in (1.0, 1e30):
        model, opt = OB.fresh(z, names, sizes, "cuda", grad_norm_clip=clip)
        got, norm, ids, _steps = OB.forced_step(z, k, model, opt, names, sizes)
        results.append((got, norm))
        before = z["p32"][k - 1]
        for i, name in enumerate(names):
            a, b = at[i], at[i + 1]
            after = got["p"][a:b].astype(np.float32)
            if name.startswith(OB.FROZEN):
                assert i not in ids and np.array_equal(after, before[a:b])
            if name == OB.NOGRAD:                                            # (float)((double)p * (1 - wd lr)), exactly
                decay = 1 - OB.HYPER["wd"] * float(z["lr"][k])
                assert i not in ids and np.array_equal(after, (before[a:b].astype(np.float64) * decay).astype(np.float32))
    (g1, n1), (g2, n2) = results
    assert n1 == n2 and 1.0 - 1e-3 <= n1 < 1.0                               # just below the clip: coef is exactly 1
    assert all(np.array_equal(g1[q], g2[q]) for q in OB.QUANTITIES)


def test_one_inf_gives_the_cpu_paths_finite_pattern():
    sizes = [5, 300, OB.O().CHUNK + 7]
    values, grads = sweep_inputs(sizes, 2, (0.5, 0.5), seed=3)
    grads[1][2][OB.O().CHUNK + 2] = np.inf
    dev, _m, _o = run_bag("cuda", torch.float32, values, grads, SWEEP_HYPER)
    cpu, _m, _o = run_bag("cpu", torch.float32, values, grads, SWEEP_HYPER)
    assert np.isinf(dev[1][3]) and np.isinf(cpu[1][3])
    bad_elems = 0
    for q in range(3):
        for x, y in zip(dev[1][q], cpu[1][q]):
            assert np.array_equal(np.isfinite(x), np.isfinite(y)) and np.array_equal(np.isnan(x), np.isnan(y))
            bad_elems += int((~np.isfinite(x)).sum())
    assert bad_elems == 3                                                    # the one element, in p, m and v


def test_two_runs_from_the_same_state_give_identical_bytes():
    sizes = sweep_sizes()[:40]
    values, grads = sweep_inputs(sizes, 3, (0.5, 30.0, 0.9), seed=5)
    a, _m, _o = run_bag("cuda", torch.float32, values, grads, SWEEP_HYPER)
    b, _m, _o = run_bag("cuda", torch.float32, values, grads, SWEEP_HYPER)
    for x, y in zip(a, b):
        assert x[3] == y[3] and x[4] == y[4]
        for q in range(3):
            assert all(s.tobytes() == t.tobytes() for s, t in zip(x[q], y[q]))


def test_step_does_not_synchronise_once_the_table_is_built():
    sizes = sweep_sizes()[:40]
    values, grads = sweep_inputs(sizes, 1, (0.5,), seed=9)
    model = Bag(values, "cuda", torch.float32)
    opt = OB.O().OneCycleAdam(model, **SWEEP_HYPER)
    opt.schedule(0)
    model.set_grads(grads[0])
    opt.step()                                                               # builds and uploads the table
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    live = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
        except RuntimeError:
            live = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') is not live on this build: a plain .item() does not raise under it")
    table = opt._table["buf"].data_ptr()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.schedule(1)
        opt.step()
        opt.schedule(2)
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt._table["buf"].data_ptr() == table and opt.steps_done == 3     # nothing rebuilt, nothing uploaded
    assert np.isfinite(float(opt.total_norm))


# ----------------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_twenty_iterations_through_a_small_rcnn_net():
    from test_rcnn_targets import make_cfg, tiny_rcnn
    ALL = {"fg_lo": 3, "fg": 4, "none": 0.1, "hard": 0.3, "easy": 0.1}
    d = {k: v.cuda() for k, v in RB.make_batch(seed=12, B=2, M=96, g_real=3, g_pad=1, N=2048, C=128, plan=ALL).items()}
    cfg = make_cfg(ROI_SAMPLE_JIT=True, NUM_POINTS=64)
    torch.manual_seed(3)
    net = tiny_rcnn(cfg)
    cpu32, cpu64 = copy.deepcopy(net), copy.deepcopy(net).double()
    net = net.cuda()
    net.train()
    hyper = dict(OB.HYPER, total_steps=20)
    O, L = OB.O(), LB.L()
    opt = O.OneCycleAdam(net, **hyper)
    names = sum(O.group_names(net), [])
    losses = []
    for it in range(20):
        net.target_seed, net._targets = 5, None                              # the same RoI sample every iteration: one batch
        opt.schedule(it)
        opt.zero_grad()
        res = L.rcnn_loss(cfg, net(d))
        res.loss.backward()
        if it == 0:                                                          # the cpu optimizer, fed the device's gradients
            grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}
            refs = []
            for model in (cpu32, cpu64):
                ref = O.OneCycleAdam(model, **hyper)
                ref.schedule(0)
                for k, p in model.named_parameters():
                    p.grad = grads[k].to(p.dtype).clone() if k in grads else None
                ref.step()
                refs.append((model, ref))
        opt.step()
        if it == 0:
            host = lambda t: t.detach().cpu().double().numpy().reshape(-1)
            rows = []
            for model, o in [(net, opt)] + refs:
                named, sd = dict(model.named_parameters()), o.state_dict()["state"]
                zero = lambda i: np.zeros(named[names[i]].numel())
                rows.append([([host(named[k]) for k in names], [host(sd[i]["exp_avg"]) if i in sd else zero(i) for i in range(len(names))],
                              [host(sd[i]["exp_avg_sq"]) if i in sd else zero(i) for i in range(len(names))], float(o.total_norm), sorted(sd))])
            assert compare_runs(*rows, "rcnn net") == []
        losses.append(float(res.loss.detach()))
    print("loss", losses[0], "->", losses[-1], "grad norm at the end", float(opt.total_norm))
    assert losses[-1] < losses[0]
    assert all(torch.isfinite(p).all() for p in net.parameters())


# --------------------------------------------------------------------------------------------------------------------- command line
def test_command_line_trains_checkpoints_and_resumes(tmp_path):
    import yaml
    from test_host_logic import TINY
    G = OB.importlib.import_module(PKG + ".gt_database")
    O, C = OB.O(), OB.importlib.import_module(PKG + ".config")
    root = str(tmp_path / "tree")
    os.makedirs(root)
    train_tree.write_train_tree(root)
    G.generate_gt_database(root, class_name="Car", save_dir=os.path.join(root, "db"), device="cpu", log=lambda *a: None)
    db = G.database_file_name(os.path.join(root, "db"), "train", "Car")
    # the tiny RPN of the end-to-end fixtures at the tree's point count; PCT_START 0.5: with 2 steps the default 0.4 leaves the first
    # phase empty, which the reference's OneCycle (and one_cycle) answer with ZeroDivisionError
    over = {"RPN": dict(TINY["RPN"], NUM_POINTS=train_tree.NPOINTS), "TRAIN": {"SPLIT": train_tree.SPLIT, "PCT_START": 0.5}}
    cfg_file = str(tmp_path / "tiny.yaml")
    with open(cfg_file, "w") as f:
        yaml.safe_dump(over, f)
    out = str(tmp_path / "out")
    base = [sys.executable, "-m", PKG + ".train_rcnn", "--train_mode", "rpn", "--root", root, "--gt_database", db, "--cfg_file", cfg_file,
            "--batch_size", "3", "--ckpt_save_interval", "1", "--npoints_faraway", str(train_tree.NPOINTS_FARAWAY), "--output_dir", out,
            "--seed", "1"]

    def child(extra):                                                        # a fresh process: nothing here has touched the GPU for it
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r

    child(["--epochs", "1"])
    ckpt = os.path.join(out, "ckpt", "checkpoint_epoch_1.pth")
    assert os.path.isfile(ckpt) and os.path.isfile(os.path.join(out, "log_train.txt"))
    cfg = C.apply_train_defaults(C.make_cfg(), "rpn")
    C.merge_into(over, cfg)
    model = OB.importlib.import_module(PKG + ".net.point_rcnn").PointRCNN(cfg, num_classes=2, use_xyz=True, mode="TEST")
    assert OB.importlib.import_module(PKG + ".eval_rcnn").load_checkpoint(model, ckpt) == 1
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert saved["it"] == 2 and saved["epoch"] == 1 and sorted(saved) == ["epoch", "it", "model_state", "optimizer_state"]
    state = saved["optimizer_state"]["state"]
    assert len(state) == len(list(model.parameters())) and all(float(st["step"]) == 2 for st in state.values())
    T = cfg.TRAIN
    sched = lambda it, total: O.one_cycle(it, total, T.LR, list(T.MOMS), T.DIV_FACTOR, T.PCT_START)
    with open(os.path.join(out, "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["it"] for ln in lines] == [1, 2] and [ln["lr"] for ln in lines] == [sched(0, 2)[0], sched(1, 2)[0]]
    assert all(np.isfinite(ln["loss"]) and np.isfinite(ln["grad_norm"]) and "rpn_loss" in ln and ln["epoch"] == 0 for ln in lines)

    r = child(["--epochs", "2", "--ckpt", ckpt])
    assert "resumed at epoch 1, it 2" in r.stdout + r.stderr
    with open(os.path.join(out, "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["it"] for ln in lines] == [1, 2, 3, 4] and [ln["epoch"] for ln in lines] == [0, 0, 1, 1]
    assert [ln["lr"] for ln in lines[2:]] == [sched(2, 4)[0], sched(3, 4)[0]]
    again = torch.load(os.path.join(out, "ckpt", "checkpoint_epoch_2.pth"), map_location="cpu", weights_only=False)
    assert again["it"] == 4 and again["epoch"] == 2
    assert all(float(st["step"]) == 4 for st in again["optimizer_state"]["state"].values())   # restored, not restarted
