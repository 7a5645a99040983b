"""The training losses on the device (losses.py on CUDA tensors, csrc/losses.hip) against fixture g23 (the reference's own get_rpn_loss /
get_rcnn_loss in f32 and f64), against the package's cpu path at the shapes where the kernels can go wrong, and end to end through a
small RCNNNet.

Bounds.  Against g23: tests/losses_batch.py tolerance (8 x the output's own e_ref, 4 ulp where e_ref is 0; counts exact).  Against the
cpu path without a fixture: both paths take their decisions in f32 and evaluate in f64, rounding to f32 once, so an output differs by
one rounding flip at most -- 2 ulp (f32) at the output's magnitude (gradients: at the tensor's largest magnitude) is allowed.  The one
exception is BinaryCrossEntropy, whose definition goes through an F32 sigmoid: the device takes exp correctly rounded, torch's exp is
within 1 ulp, so p may differ by one ulp of a number near 1, 2^-24, which log1p(-p) magnifies by 1 / (1 - p).  The sweep's logits are
at most 6 in magnitude apart from the saturated ones (where both give exactly 0 or 1, or 1 - p = 1), so a BCE term may differ by
2^-24 (1 + e^6) = 2.5e-5 and so may their mean; the gradient of an entry, w (p - t) / n_valid, by w 2^-23 / n_valid."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import losses_batch as LB  # noqa: E402
import rcnn_targets_batch as RB  # noqa: E402

pytestmark = pytest.mark.gpu
G23 = os.path.join(HERE, "golden", "g23_losses_ref.npz")
ROWS = (1, 63, 64, 65, 257, 2 * 1300 + 3)
BCE_VALUE_TOL = 2.0 ** -24 * (1.0 + np.exp(6.0))
# C -> the fixture case whose configuration the sweep borrows
SWEEP_CFG = {46: "rcnn_bce_c46", 52: "rpn_dice_c52", 53: "rcnn_focal_c53_roi", 76: "rpn_focal_c76"}


def compare_paths(spec, dev, cpu, what):
    """(LossResult, grad_cls, grad_reg) of both paths under the docstring's rule; prints every figure first"""
    P, names = LB.L().P, LB.L().PART_NAMES
    bce = spec.cls_kind == "BinaryCrossEntropy"
    pd, pc = dev[0].parts.cpu().numpy().astype(np.float64), cpu[0].parts.cpu().numpy().astype(np.float64)
    bad = []
    for k in names:
        d, c = pd[P[k]], pc[P[k]]
        tol = 0.0 if k in LB.COUNT_PARTS else 2 * LB.ulp32(c)
        if bce and k in ("loss", "cls"):
            tol += BCE_VALUE_TOL * spec.w_cls
        print("%s %-9s device % .9e cpu % .9e diff %.3e tol %.3e" % (what, k, d, c, abs(d - c), tol))
        if not abs(d - c) <= tol:
            bad.append(k)
    n_valid = max(pc[P["n_valid"]], 1.0)
    for k, d, c in (("grad_cls", dev[1], cpu[1]), ("grad_reg", dev[2], cpu[2])):
        tol = 2 * LB.ulp32(np.abs(c).max(initial=0.0))
        if bce and k == "grad_cls":
            tol += max(spec.fg_weight, 1.0) * spec.w_cls * 2.0 ** -23 / n_valid
        diff = float(np.abs(d - c).max(initial=0.0))
        print("%s %-9s max diff %.3e tol %.3e (max |cpu| %.3e)" % (what, k, diff, tol, np.abs(c).max(initial=0.0)))
        if not diff <= tol:
            bad.append(k)
    return bad


def both(name_or_spec, b, shape=None):
    out = []
    for device in ("cuda", "cpu"):
        res, cls, reg = LB.run(name_or_spec, b, device=device, shape=shape)
        out.append((res,) + LB.grads(res, cls, reg))
    return out


@pytest.mark.parametrize("name", list(LB.CASES))
def test_device_path_against_the_reference_and_the_cpu_path(name):
    z = np.load(G23, allow_pickle=False)
    b = LB.case_batch(name)
    LB.check_inputs(z, name, b)
    dev, cpu = both(name, b, shape=LB.RPN_SHAPE if LB.CASES[name][0] == "rpn" else None)
    res = dev[0]
    assert res.loss.is_cuda and res.parts.is_cuda and res.loss.dim() == 0 and res.loss.grad_fn is not None
    bad = LB.check_against_fixture(z, name, res, dev[1], dev[2], "device")
    assert LB.check_against_fixture(z, name, cpu[0], cpu[1], cpu[2], "cpu") == []
    assert torch.equal(res.parts[-6:-2].cpu(), cpu[0].parts[-6:-2])                # the four counts
    assert bad == []
    assert res.tb_dict().keys() == cpu[0].tb_dict().keys()


@pytest.mark.parametrize("channels", sorted(SWEEP_CFG))
@pytest.mark.parametrize("rows", ROWS)
def test_shape_sweep_against_the_cpu_path(rows, channels):
    name = SWEEP_CFG[channels]
    spec, stage = LB.case_spec(name), LB.CASES[name][0]
    assert spec.channels == channels
    b = LB.make_batch(stage, "mixed", channels, n=rows, seed=rows + channels, fg_share=0.3)
    dev, cpu = both(spec, b)
    assert compare_paths(spec, dev, cpu, "rows %d C %d" % (rows, channels)) == []


@pytest.mark.parametrize("name", ["rpn_dice_c52", "rpn_focal_c76", "rpn_bce_c76", "rcnn_bce_c46", "rcnn_focal_c53_roi"])
def test_rows_outside_the_mask_and_ignored_entries_reach_nothing(name):
    b = LB.case_batch(name)
    fg = (b["reg_mask"] > 0) if "reg_mask" in b else (b["label"] > 0)
    dirty = {k: v.copy() for k, v in b.items()}
    dirty["reg"][~fg] = np.where(np.arange((~fg).sum())[:, None] % 2 == 0, np.nan, np.inf)
    dirty["cls"][b["label"] == -1] = np.nan
    want, cls, reg = LB.run(name, b, device="cuda")
    want_g = LB.grads(want, cls, reg)
    got, cls, reg = LB.run(name, dirty, device="cuda")
    got_g = LB.grads(got, cls, reg)
    assert torch.isfinite(got.parts).all() and torch.isfinite(got.loss) and np.isfinite(got_g[0]).all() and np.isfinite(got_g[1]).all()
    assert not got_g[1][~fg].any() and not got_g[0][b["label"] == -1].any()
    assert torch.equal(got.parts, want.parts) and np.array_equal(got_g[0], want_g[0]) and np.array_equal(got_g[1], want_g[1])


@pytest.mark.parametrize("channels", [52, 76, 46])
def test_two_runs_agree_bit_for_bit(channels):
    name = SWEEP_CFG[channels]
    b = LB.make_batch(LB.CASES[name][0], "mixed", channels, n=ROWS[-1], seed=7, fg_share=0.3)
    runs = []
    for _ in range(2):
        res, cls, reg = LB.run(name, b, device="cuda")
        res.loss.backward()
        runs.append((res.parts.clone(), cls.grad.clone(), reg.grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(*runs))


def test_backward_scales_and_accumulates():
    b1, b2 = LB.case_batch("rpn_focal_c76"), LB.case_batch("rcnn_focal_c53_roi")
    res, cls, reg = LB.run("rpn_focal_c76", b1, device="cuda")
    g_cls, g_reg = torch.autograd.grad(res.loss, [cls, reg])
    res, cls, reg = LB.run("rpn_focal_c76", b1, device="cuda")
    (2.5 * res.loss).backward()
    assert torch.equal(cls.grad, 2.5 * g_cls) and torch.equal(reg.grad, 2.5 * g_reg)
    # two stages fed from one leaf: the sum's backward accumulates both into it
    t1 = {k: torch.from_numpy(v).cuda() for k, v in b1.items()}
    t2 = {k: torch.from_numpy(v).cuda() for k, v in b2.items()}
    s1, s2 = LB.case_spec("rpn_focal_c76"), LB.case_spec("rcnn_focal_c53_roi")
    leaf = torch.tensor([1.0, 0.5], device="cuda", requires_grad=True)

    def stages(leaf):
        r1 = LB.L()._stage(s1, t1["cls"] * leaf[0], t1["reg"] * leaf[1], t1["label"], None, t1["reg_label"], None)
        r2 = LB.L()._stage(s2, t2["cls"] * leaf[1], t2["reg"] * leaf[0], t2["label"], t2["reg_mask"], t2["reg_label"], t2["roi"])
        return r1, r2
    r1, r2 = stages(leaf)
    (r1.loss + r2.loss).backward()
    r1, r2 = stages(leaf)
    want = torch.autograd.grad(r1.loss, leaf)[0].double() + torch.autograd.grad(r2.loss, leaf)[0].double()
    print("leaf grad", leaf.grad.tolist(), "sum of the stages' own", want.tolist())
    # f32 sums of ~1e5 products, accumulated in another order by the two routes: 1e-5 relative covers sqrt(n) x 2^-24 with room
    assert torch.allclose(leaf.grad.double(), want, rtol=1e-5, atol=0)


def test_forward_and_backward_do_not_synchronise():
    b1, b2 = LB.case_batch("rpn_bce_c76"), LB.case_batch("rcnn_bce_c53")
    probe = torch.ones(1, device="cuda")
    for name, b in (("rpn_bce_c76", b1), ("rcnn_bce_c53", b2)):                  # warm-up outside the mode: library load, allocator
        res, cls, reg = LB.run(name, b, device="cuda")
        res.loss.backward()
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
    staged = []
    for name, b in (("rpn_dice_c52", LB.case_batch("rpn_dice_c52")), ("rpn_focal_c76", LB.case_batch("rpn_focal_c76")), ("rpn_bce_c76", b1),
                    ("rcnn_bce_c53", b2), ("rcnn_focal_c53_roi", LB.case_batch("rcnn_focal_c53_roi")), ("rcnn_bce_nofg", LB.case_batch("rcnn_bce_nofg"))):
        spec = LB.case_spec(name)
        t = {k: torch.from_numpy(v).cuda() for k, v in b.items()}
        staged.append((spec, t, t["cls"].clone().requires_grad_(True), t["reg"].clone().requires_grad_(True)))
    torch.cuda.synchronize()
    results = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for spec, t, cls, reg in staged:
            res = LB.L()._stage(spec, cls, reg, t["label"], t.get("reg_mask"), t["reg_label"], t["roi"] if spec.anchor_on_roi else None)
            (res.loss * 2.0).backward()
            results.append(res)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for res in results:                                                       # tb_dict() is the read, outside the mode
        assert np.isfinite(list(res.tb_dict().values())).all()


def test_end_to_end_through_a_small_rcnn_net():
    from test_rcnn_targets import make_cfg, tiny_rcnn
    ALL = {"fg_lo": 3, "fg": 4, "none": 0.1, "hard": 0.3, "easy": 0.1}
    d = {k: v.cuda() for k, v in RB.make_batch(seed=12, B=2, M=96, g_real=3, g_pad=1, N=2048, C=128, plan=ALL).items()}
    cfg = make_cfg(ROI_SAMPLE_JIT=True, NUM_POINTS=64)
    torch.manual_seed(3)
    net = tiny_rcnn(cfg).cuda()
    net.target_seed = 5
    net.train()
    feats = []
    hook = net.reg_layer[-1].register_forward_hook(lambda _m, inp, _out: feats.append(inp[0].detach()))
    ret = net(d)
    hook.remove()
    L = LB.L()
    spec = L.rcnn_spec(cfg)
    weight = net.reg_layer[-1].conv.weight
    res = L.rcnn_loss(cfg, ret)
    n = ret["rcnn_cls"].numel()
    loss_f, parts_f = L._stage_cpu(spec, ret["rcnn_cls"].reshape(-1), ret["rcnn_reg"].reshape(n, -1), ret["cls_label"], ret["reg_valid_mask"],
                                   ret["gt_of_rois"], None)
    leaves = [ret["rcnn_cls"], ret["rcnn_reg"], weight]
    got = torch.autograd.grad(res.loss, leaves, retain_graph=True)
    want = torch.autograd.grad(loss_f, leaves, retain_graph=True)
    flat = lambda g: g.detach().cpu().numpy().astype(np.float64)
    dev = (res, flat(got[0]).reshape(-1), flat(got[1]).reshape(n, -1))
    ref = (L.LossResult(spec, loss_f, parts_f), flat(want[0]).reshape(-1), flat(want[1]).reshape(n, -1))
    print("fg rows", int(parts_f[L.P["n_reg_fg"]]), "labels", [int((ret["cls_label"] == v).sum()) for v in (-1, 0, 1)])
    assert int(parts_f[L.P["n_reg_fg"]]) > 0
    assert compare_paths(spec, dev, ref, "end to end") == []
    # the last regression layer's weight: the same product of the same features with two grad_reg tensors that differ by 2 ulp of their
    # largest entry at most (checked above), so entry (o, i) may differ by that times sum_rows |f[row, i]|, plus the f32 sum's own
    # reordering-free rounding (the same kernel runs both): 2 ulp of the result
    f = feats[0].reshape(n, -1).abs().sum(dim=0).cpu().numpy().astype(np.float64)
    tol = 2 * LB.ulp32(np.abs(ref[2]).max()) * f[None, :] + 2 * np.vectorize(LB.ulp32)(np.abs(flat(want[2]).reshape(-1, f.size)).max())
    diff = np.abs(flat(got[2]) - flat(want[2])).reshape(-1, f.size)
    print("reg weight grad: max diff %.3e, max |grad| %.3e, smallest tol %.3e" % (diff.max(), np.abs(flat(want[2])).max(), tol.min()))
    assert (diff <= tol).all()
    res.loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
