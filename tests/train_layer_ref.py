"""The numpy / f64 definition of the training layer (include/prcnn_hip.h, "the order-fixed TRAINING layer"): forward and backward of
a 1x1 convolution, BatchNorm on batch statistics and ReLU, for the block forms conv+bn+relu, conv+bn, conv+bias+relu and conv+bias.
Written from the formulas; tests/test_train_layer_ref.py pins it against torch.autograd in f64.  Also the lattice case generator
that the GPU tests use.

Layout: x (B, Cin, P), w (Cout, Cin), z / y / dy (B, Cout, P); n = B * P."""
import numpy as np


def forward(x, w, gamma=None, beta=None, bias=None, eps=1e-5, relu=True):
    """-> dict z, pre, y and with BatchNorm (gamma given) mean, var (biased), rstd, zhat: all f64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    z = np.einsum("oc,bcp->bop", w, x)
    out = {"z": z}
    if gamma is not None:
        n = z.shape[0] * z.shape[2]
        mean = z.sum((0, 2)) / n
        var = np.maximum((z * z).sum((0, 2)) / n - mean * mean, 0.0)
        rstd = 1.0 / np.sqrt(var + eps)
        zhat = (z - mean[None, :, None]) * rstd[None, :, None]
        pre = zhat * np.asarray(gamma, np.float64)[None, :, None] + np.asarray(beta, np.float64)[None, :, None]
        out.update(mean=mean, var=var, rstd=rstd, zhat=zhat)
    else:
        pre = z + (0.0 if bias is None else np.asarray(bias, np.float64)[None, :, None])
    out["pre"] = pre
    out["y"] = np.maximum(pre, 0.0) if relu else pre
    return out


def running(running_mean, running_var, mean, var, n, momentum):
    """the running statistics after one training forward: the unbiased variance goes into running_var"""
    rm = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
    rv = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * (var * n / (n - 1.0))
    return rm, rv


def backward(dy, x, w, fw, gamma=None, relu=True):
    """fw = forward(...) of the same block -> dict dx, dw and dgamma, dbeta (BatchNorm) or dbias: f64"""
    dy, x, w = np.asarray(dy, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64)
    g = np.where(fw["pre"] > 0.0, dy, 0.0) if relu else dy
    out = {}
    if gamma is not None:
        n = dy.shape[0] * dy.shape[2]
        s1 = g.sum((0, 2))
        s2 = (g * fw["zhat"]).sum((0, 2))
        out.update(dbeta=s1, dgamma=s2)
        dz = (np.asarray(gamma, np.float64) * fw["rstd"])[None, :, None] * (g - (s1 / n)[None, :, None] - fw["zhat"] * (s2 / n)[None, :, None])
    else:
        dz = g
        out["dbias"] = g.sum((0, 2))
    out["dx"] = np.einsum("oc,bop->bcp", w, dz)
    out["dw"] = np.einsum("bop,bcp->oc", dz, x)
    return out


def torch_block(case, dtype, device="cpu"):
    """torch's own modules on the case's tensors -> dict of outputs (numpy f64), gradients and buffers included"""
    import torch
    t = lambda a: torch.from_numpy(np.asarray(a)).to(device=device, dtype=dtype)
    cout, cin = case["w"].shape
    conv = torch.nn.Conv1d(cin, cout, 1, bias=case["bias"] is not None).to(device=device, dtype=dtype)
    mods = [conv]
    with torch.no_grad():
        conv.weight.copy_(t(case["w"]).unsqueeze(-1))
        if case["bias"] is not None:
            conv.bias.copy_(t(case["bias"]))
    if case["bn"]:
        bn = torch.nn.BatchNorm1d(cout, eps=case["eps"], momentum=case["momentum"]).to(device=device, dtype=dtype)
        with torch.no_grad():
            bn.weight.copy_(t(case["gamma"])); bn.bias.copy_(t(case["beta"]))
            bn.running_mean.copy_(t(case["running_mean"])); bn.running_var.copy_(t(case["running_var"]))
        mods.append(bn)
    if case["relu"]:
        mods.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*mods).train()
    x = t(case["x"]).requires_grad_(True)
    y = net(x)
    y.backward(t(case["dy"]))
    n64 = lambda v: v.detach().double().cpu().numpy()
    out = dict(y=n64(y), dx=n64(x.grad), dw=n64(conv.weight.grad)[:, :, 0])
    if case["bn"]:
        out.update(dgamma=n64(bn.weight.grad), dbeta=n64(bn.bias.grad), running_mean=n64(bn.running_mean), running_var=n64(bn.running_var))
        with torch.no_grad():
            _, mean, rstd = torch.native_batch_norm(conv(x), bn.weight, bn.bias, None, None, True, 0.0, case["eps"])
        out.update(mean=n64(mean), rstd=n64(rstd))
    elif case["bias"] is not None:
        out["dbias"] = n64(conv.bias.grad)
    return out


def reference(case):
    """the f64 definition on the case's tensors -> the same dict"""
    fw = forward(case["x"], case["w"], case["gamma"], case["beta"], case["bias"], case["eps"], case["relu"])
    out = backward(case["dy"], case["x"], case["w"], fw, case["gamma"], case["relu"])
    out["y"] = fw["y"]
    if case["bn"]:
        n = case["x"].shape[0] * case["x"].shape[2]
        out["running_mean"], out["running_var"] = running(case["running_mean"], case["running_var"], fw["mean"], fw["var"], n, case["momentum"])
        out.update(mean=fw["mean"], rstd=fw["rstd"])
    return out


MARGIN = 1e-4       # every f64 pre-activation of a generated case is at least this far from zero


def lattice_case(b, cin, cout, p, bn=True, relu=True, seed=0, zero_row=None):
    """A single-layer case on the 1/8 lattice.  x and w are multiples of 1/8 in [-2, 2]: every product and partial sum of z is a
    multiple of 1/64 below 2^24 / 64 in magnitude, so exact in f32 in ANY order -- z has one right answer.  beta (or the bias) puts
    each channel's ReLU threshold half a lattice step (1/128) between two values of z, near the channel's median; the generator
    ASSERTS that every f64 pre-activation is at least MARGIN from zero, so no mask differs between an f32 and the f64 evaluation.
    zero_row: that weight row is zero (var = 0, rstd = 1 / sqrt(eps)).  -> dict of f32 arrays (dy, gamma, running buffers random)."""
    rng = np.random.default_rng(1000003 * seed + 7919 * b + 131 * cin + 17 * cout + p)
    x = (rng.integers(-16, 17, (b, cin, p)) / 8.0).astype(np.float32)
    w = (rng.integers(-16, 17, (cout, cin)) / 8.0).astype(np.float32)
    if zero_row is not None:
        w[zero_row] = 0.0
    assert cin * 4.0 * 64 < 2 ** 24
    z = np.einsum("oc,bcp->bop", w.astype(np.float64), x.astype(np.float64))
    med = np.floor(np.median(z, axis=(0, 2)) * 64.0) / 64.0 + 1.0 / 128.0      # per channel, half a step above a lattice value
    case = dict(x=x, w=w, eps=1e-5, momentum=0.1, bn=bn, relu=relu)
    case["dy"] = rng.standard_normal((b, cout, p)).astype(np.float32)
    if bn:
        gamma = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
        n = b * p
        mean = z.sum((0, 2)) / n
        var = ((z - mean[None, :, None]) ** 2).sum((0, 2)) / n
        beta = (-gamma.astype(np.float64) * (med - mean) / np.sqrt(var + case["eps"])).astype(np.float32)
        case.update(gamma=gamma, beta=beta, bias=None)
        case["running_mean"] = rng.standard_normal(cout).astype(np.float32)
        case["running_var"] = rng.uniform(0.5, 2.0, cout).astype(np.float32)
    else:
        case.update(gamma=None, beta=None, bias=(-med).astype(np.float32))
    fw = forward(x, w, case["gamma"], case["beta"], case["bias"], case["eps"], relu)
    margin = float(np.abs(fw["pre"]).min())
    assert margin >= MARGIN, "lattice case (%d, %d, %d, %d): smallest |pre-activation| %.3e" % (b, cin, cout, p, margin)
    case["margin"] = margin
    return case
