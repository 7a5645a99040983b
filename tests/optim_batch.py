"""Seeded inputs for the optimizer tests (optim.py): the tiny model and the recorded gradients of fixture g24
(tests/golden/make_golden_optim.py records the reference's OptimWrapper + OneCycle + clip_grad_norm_ on exactly these), the
teacher-forcing helpers, and the bound of the tests (the g23 rule of tests/losses_batch.py).

The model: 201 parameter elements in 14 tensors of 1, 3, 15, 64, 65, ... elements, both groups (two BatchNorm1d), one module
(``frozen``) frozen after the optimizer is built, one trainable tensor (``nograd.weight``) that never receives a grad.  It is never run
forward: the gradients are recorded numbers.  12 steps, total_steps = 12: even steps small (norm 0.07, not clipped), odd steps large
(norm 20, clipped), step NEAR the clip value from below (norm 0.9995).
"""
import importlib

import numpy as np

from losses_batch import tolerance, ulp32  # noqa: F401  (the bound: 8 x e_ref, 4 ulp (f32) at the largest magnitude where e_ref is 0)

PKG = "3d_adapt_auto_driving_amd"
SEED = 24
STEPS = 12
HYPER = dict(total_steps=12, lr_max=0.002, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4, wd=0.001, grad_norm_clip=1.0)
NEAR, NEAR_NORM, SMALL_NORM, LARGE_NORM = 4, 0.9995, 0.07, 20.0
FROZEN, NOGRAD = "frozen", "nograd.weight"
TABLES = [(t, p) for t in (1, 2, 5, 12, 100) for p in (0.1, 0.4)]
QUANTITIES = ("p", "m", "v")


def O():
    return importlib.import_module(PKG + ".optim")


def tiny_model(dtype=None):
    import torch
    import torch.nn as nn

    class Scalar(nn.Module):
        def __init__(self):
            super().__init__()
            self.s = nn.Parameter(torch.ones(1))

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv1d(8, 8, 1)               # 64 + 8
            self.bn2 = nn.BatchNorm1d(4)                 # 4 + 4
            self.lin_b = nn.Linear(13, 5)                # 65 + 5

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin_a = nn.Linear(5, 3)                 # 15 + 3
            self.bn = nn.BatchNorm1d(3)                  # 3 + 3
            self.block = Block()
            self.scale = Scalar()                        # 1
            self.frozen = nn.Linear(4, 4)                # 16 + 4
            self.nograd = nn.Linear(3, 2, bias=False)    # 6
    torch.manual_seed(SEED)
    m = Tiny()
    with torch.no_grad():
        for k, p in enumerate(m.parameters()):           # BatchNorm weights away from exactly 1, biases from exactly 0
            p.add_(0.01 * torch.randn(p.shape, generator=torch.Generator().manual_seed(SEED + k)))
    return m if dtype is None else m.to(dtype)


def freeze(model):
    for p in model.frozen.parameters():
        p.requires_grad = False


def has_grad(name):
    return not name.startswith(FROZEN) and name != NOGRAD


def step_norm(k):
    return NEAR_NORM if k == NEAR else (SMALL_NORM if k % 2 == 0 else LARGE_NORM)


def make_grads(names, sizes):
    """-> (STEPS, total) f32: the grads of every tensor, concatenated in ``names`` order (zeros where a tensor gets none)"""
    rng = np.random.RandomState(SEED)
    total = int(sum(sizes))
    mask = np.concatenate([np.full(n, has_grad(k)) for k, n in zip(names, sizes)])
    out = np.zeros((STEPS, total), dtype=np.float32)
    for k in range(STEPS):
        g = rng.standard_normal(total) * mask
        out[k] = (g * (step_norm(k) / np.sqrt((g * g).sum()))).astype(np.float32)
    return out


def split(vec, sizes):
    at = np.cumsum([0] + list(sizes))
    return [vec[a:b] for a, b in zip(at[:-1], at[1:])]


def layout(model):
    """-> (names in optimizer order: group 0 then group 1, sizes)"""
    names = sum(O().group_names(model), [])
    size = {k: p.numel() for k, p in model.named_parameters()}
    return names, [size[k] for k in names]


def set_params(model, names, vec, sizes):
    import torch
    named = dict(model.named_parameters())
    with torch.no_grad():
        for k, v in zip(names, split(vec, sizes)):
            named[k].copy_(torch.from_numpy(np.ascontiguousarray(v)).to(named[k].dtype).reshape(named[k].shape))


def set_grads(model, names, vec, sizes):
    import torch
    named = dict(model.named_parameters())
    for k, v in zip(names, split(vec, sizes)):
        p = named[k]
        p.grad = torch.from_numpy(np.array(v)).to(device=p.device, dtype=p.dtype).reshape(p.shape) if has_grad(k) else None    # (a copy: a clip scales it in place)


def get_params(model, names):
    named = dict(model.named_parameters())
    return np.concatenate([named[k].detach().cpu().double().numpy().reshape(-1) for k in names])


def make_state_dict(template, names, sizes, m, v, step, model):
    """An Adam state_dict in ``template``'s layout (a state_dict() of the same optimizer class) holding m, v (concatenated vectors) and
    ``step`` for every tensor that has a grad; no state when step == 0"""
    import torch
    named = dict(model.named_parameters())
    state = {}
    if step > 0:
        for i, (k, mm, vv) in enumerate(zip(names, split(m, sizes), split(v, sizes))):
            if has_grad(k):
                p = named[k]
                conv = lambda a: torch.from_numpy(np.array(a)).to(device=p.device, dtype=p.dtype).reshape(p.shape)
                state[i] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": conv(mm), "exp_avg_sq": conv(vv)}
    return {"state": state, "param_groups": [dict(g) for g in template["param_groups"]]}


def get_state(sd, names, sizes):
    """state_dict -> (m, v) concatenated f64 vectors (zeros where no state), the sorted indices that have state, their steps"""
    m, v = [np.zeros(n) for n in sizes], [np.zeros(n) for n in sizes]
    for i, st in sd["state"].items():
        m[i] = st["exp_avg"].detach().cpu().double().numpy().reshape(-1)
        v[i] = st["exp_avg_sq"].detach().cpu().double().numpy().reshape(-1)
    idx = sorted(sd["state"])
    return np.concatenate(m), np.concatenate(v), idx, [int(float(sd["state"][i]["step"])) for i in idx]


def check_step(z, k, names, sizes, got, norm, tag, report):
    """got = {"p", "m", "v"}: concatenated f64 vectors after step k -> the list of (tensor, quantity) that miss the bound"""
    bad = []
    for q in QUANTITIES:
        ref64, eref = split(z["%s64" % q][k], sizes), z["eref_%s" % q][k]
        for i, (name, g, r) in enumerate(zip(names, split(got[q], sizes), ref64)):
            err, mag = float(np.abs(g - r).max()), float(np.abs(r).max())
            tol = tolerance(eref[i], mag)
            report.append("%s step %2d %-22s %s err %.3e e_ref %.3e tol %.3e" % (tag, k, name, q, err, eref[i], tol))
            if not err <= tol:
                bad.append((k, name, q))
    err, e = abs(float(norm) - float(z["norm64"][k])), float(z["eref_norm"][k])
    tol = tolerance(e, z["norm64"][k])
    report.append("%s step %2d %-22s err %.3e e_ref %.3e tol %.3e" % (tag, k, "total_norm", err, e, tol))
    if not err <= tol:
        bad.append((k, "total_norm", "norm"))
    return bad


def load_fixture():
    import json
    import os
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_optim_ref.npz")))
    return z, json.loads(str(z["names"])), [int(n) for n in z["sizes"]]


def fresh(z, names, sizes, device="cpu", dtype=None, **over):
    """-> (model holding the fixture's initial parameters, its OneCycleAdam); ``frozen`` is frozen after the optimizer is built"""
    model = tiny_model(dtype).to(device)
    assert layout(model) == (names, sizes)
    set_params(model, names, z["p0"], sizes)
    opt = O().OneCycleAdam(model, **dict(HYPER, **over))
    freeze(model)
    return model, opt


def forced_step(z, k, model, opt, names, sizes):
    """Step k from the f32 reference run's state before it -> ({"p", "m", "v"} f64 vectors, total_norm, state indices, their steps)"""
    zero = np.zeros(int(sum(sizes)), dtype=np.float32)
    set_params(model, names, z["p32"][k - 1] if k else z["p0"], sizes)
    opt.load_state_dict(make_state_dict(opt.state_dict(), names, sizes, z["m32"][k - 1] if k else zero, z["v32"][k - 1] if k else zero, k, model))
    opt.schedule(k)
    assert (opt.lr, opt.mom) == (float(z["lr"][k]), float(z["mom"][k]))
    opt.zero_grad()
    set_grads(model, names, z["grads"][k], sizes)
    opt.step()
    m, v, ids, steps = get_state(opt.state_dict(), names, sizes)
    return {"p": get_params(model, names), "m": m, "v": v}, float(opt.total_norm), ids, steps


def teacher_forced(device):
    """The 12 steps of g24 on ``device``, each from the reference's f32 state -> the outputs that miss the bound; prints every figure"""
    import json
    z, names, sizes = load_fixture()
    model, opt = fresh(z, names, sizes, device)
    report, bad = [], []
    at = np.cumsum([0] + sizes)
    for k in range(STEPS):
        got, norm, ids, steps = forced_step(z, k, model, opt, names, sizes)
        bad += check_step(z, k, names, sizes, got, norm, str(device), report)
        assert ids == json.loads(str(z["state_ids"])) and steps == [k + 1] * len(ids)
        before = z["p32"][k - 1] if k else z["p0"]
        for i, name in enumerate(names):
            a, b = at[i], at[i + 1]
            if name.startswith(FROZEN):                               # never touched: the recorded bits
                assert np.array_equal(got["p"][a:b].astype(np.float32), z["p0"][a:b]), name
            if name == NOGRAD:                                        # decayed only, and without state
                assert i not in ids
                want = before[a:b].astype(np.float64) * (1 - HYPER["wd"] * float(z["lr"][k]))
                assert np.abs(got["p"][a:b] - want).max() <= ulp32(np.abs(want).max()), name
    print("\n".join(report))
    return bad
