"""-m gpu: the order-fixed training layer (csrc/train_layer.hip; include/prcnn_hip.h prcnn_train_layer_*) through its wrappers
against the f64 definition of tests/train_layer_ref.py.

Inputs are LATTICE inputs (train_layer_ref.lattice_case): x and w multiples of 1/8, so z has one right answer in f32 and must come
out bit for bit, and every pre-activation keeps 1e-4 from zero, so no ReLU mask differs between an f32 and the f64 evaluation.
Every float output is then compared with the f64 definition under the project's rule (losses_batch.tolerance):
8 x e_ref, and 4 ulp at the tensor's magnitude where e_ref is 0, with e_ref = |ref32 - ref64| measured here from torch's own f32
Conv1d + BatchNorm1d + ReLU on the same GPU -- or from the same modules in f32 on the CPU where that error is the smaller one, which
only tightens the bound: measured on an MI355X, torch's f32 BatchNorm backward on the GPU is off by up to 19 in dgamma (magnitude
70 - 180) at P = 1027 and P = 2051, where its CPU form and this layer stay near 1e-5, and a bound of 8 x that would check nothing.
Every ratio is printed.

Shapes (B, Cin, Cout, P) are the smallest that cross the kernels' boundaries: Cin in {1, 3, 19, 33 = one above the 32 of a weight
stage, 65 = one above the 64-wide tile of the weight gradient, 131}; Cout in {1, 16, 32, 130, 196} (one 32-row tile, two, beyond the
64 rows of a workgroup, no multiple of 32); P in {1, 63, 129 = one above the 128 positions of a sub-tile, 257, 1027,
2 * PRCNN_TRAIN_CHUNK + 3}; B in {1, 2, 3}.  Wide channels go with short P: no case has more than 2e5 output elements."""
import numpy as np
import pytest
import torch

import losses_batch as LB
import train_layer_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ops():
    return pkg("pointnet2.pointnet2_utils").pointnet2


def chunk():
    return pkg("_lib").PRCNN_TRAIN_CHUNK


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shapes():
    return [(3, 1, 1, 1), (1, 3, 16, 63), (3, 19, 130, 63), (1, 33, 196, 129), (1, 65, 1, 129), (2, 131, 196, 257), (2, 96, 32, 1027),
            (3, 3, 16, 2 * chunk() + 3)]


# BatchNorm + ReLU on every shape; the three other forms where the tiles, the chunks and the narrow widths are crossed
CASES = [(i, True, True) for i in range(8)] + [(i, bn, relu) for i in (2, 4, 7) for bn, relu in ((True, False), (False, True), (False, False))]
IDS = ["s%d-%s%s" % (i, "bn" if bn else "bias", "-relu" if relu else "") for i, bn, relu in CASES]


def run_layer(case, need_dx=True, need_dw=True, stream=None):
    """forward + backward through the wrappers -> dict of device tensors (z and stats as well)"""
    t = {k: dev(case[k]) for k in ("x", "w", "dy", "gamma", "beta", "bias")}
    out = {}
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        if case["bn"]:
            rm, rv = dev(case["running_mean"]), dev(case["running_var"])
            y, z, stats = ops().train_layer_forward_wrapper(t["x"], t["w"], t["gamma"], t["beta"], case["eps"], case["momentum"], rm, rv, case["relu"])
            dx, dw, dgamma, dbeta = ops().train_layer_backward_wrapper(t["dy"], t["x"], t["w"], z, t["gamma"], t["beta"], stats, case["relu"],
                                                                       need_dx, need_dw)
            out.update(z=z, mean=stats[0], rstd=stats[1], running_mean=rm, running_var=rv, dgamma=dgamma, dbeta=dbeta)
        else:
            y, z, stats = ops().train_layer_forward_wrapper(t["x"], t["w"], None, t["bias"], 0.0, 0.0, None, None, case["relu"])
            assert z is None and stats is None
            dx, dw, dgamma, dbias = ops().train_layer_backward_wrapper(t["dy"], t["x"], t["w"], y, None, None, None, case["relu"], need_dx, need_dw)
            assert dgamma is None
            out["dbias"] = dbias
        out.update(y=y, dx=dx, dw=dw)
    if stream is not None:
        stream.synchronize()
    return out


_CACHE = {}


def solved(i, bn, relu, zero_row=None):
    """-> (case, ref64, e_ref per output from torch's f32 block on this GPU, ours as numpy); computed once and left unchanged"""
    key = (i, bn, relu, zero_row)
    if key not in _CACHE:
        case = R.lattice_case(*shapes()[i], bn=bn, relu=relu, zero_row=zero_row)
        ref = R.reference(case)
        ref["z"] = R.forward(case["x"], case["w"])["z"]
        t32, c32 = R.torch_block(case, torch.float32, DEV), R.torch_block(case, torch.float32, "cpu")
        e_ref = {k: min(float(np.abs(t32[k] - ref[k]).max()), float(np.abs(c32[k] - ref[k]).max())) for k in t32}
        got = {k: v.cpu().numpy() for k, v in run_layer(case).items() if v is not None}
        _CACHE[key] = (case, ref, e_ref, got)
    return _CACHE[key]


def check_all(name, case, ref, e_ref, got):
    report, ok = [], True
    for k in sorted(e_ref):
        assert got[k].shape == ref[k].shape or got[k].size == ref[k].size, k
        assert np.isfinite(got[k]).all(), k
        ok &= LB.check_tensor("%s %s" % (name, k), got[k].reshape(ref[k].shape).astype(np.float64), ref[k], e_ref[k], report)
    print("\n".join(report))
    assert ok, "\n".join(report)


@pytest.mark.parametrize("i,bn,relu", CASES, ids=IDS)
def test_z_is_exact_and_every_output_is_inside_the_bound(i, bn, relu):
    case, ref, e_ref, got = solved(i, bn, relu)
    b, cin, cout, p = shapes()[i]
    assert b * cout * p <= 2e5
    if bn:
        assert got["z"].dtype == np.float32 and np.array_equal(got["z"].astype(np.float64), ref["z"]), "z differs from its one right answer"
        assert got["mean"].dtype == np.float64 and got["rstd"].dtype == np.float64
    else:
        assert np.array_equal(got["y"].astype(np.float64), ref["y"]), "z + bias is exact on the lattice"
    assert set(e_ref) <= set(got)
    check_all(IDS[CASES.index((i, bn, relu))], case, ref, e_ref, got)


def test_a_channel_with_a_zero_weight_row():
    case, ref, e_ref, got = solved(2, True, True, zero_row=5)
    assert got["mean"][5] == 0.0 and got["rstd"][5] == 1.0 / np.sqrt(case["eps"])
    assert (got["z"][:, 5] == 0).all()
    check_all("zero-row", case, ref, e_ref, got)


def test_one_value_per_channel_raises_with_batchnorm():
    case = R.lattice_case(1, 3, 16, 2)
    x = dev(case["x"][:, :, :1])
    with pytest.raises(ValueError):
        ops().train_layer_forward_wrapper(x, dev(case["w"]), dev(case["gamma"]), dev(case["beta"]), 1e-5, 0.1, None, None, True)
    pt = pkg("pointnet2.pytorch_utils")
    block = pt.Conv1d(3, 16, bn=True).to(DEV).train()
    with pt.fused_train_layers(), pytest.raises(ValueError):
        block(x)
    y, _, _ = ops().train_layer_forward_wrapper(x, dev(case["w"]), None, None, 0.0, 0.0, None, None, True)      # no BatchNorm: n = 1 is fine
    assert y.shape == (1, 16, 1)


def same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k].view(torch.int32 if a[k].dtype == torch.float32 else torch.int64),
                               b[k].view(torch.int32 if b[k].dtype == torch.float32 else torch.int64)), k


@pytest.mark.parametrize("i,bn", [(2, True), (7, True), (7, False)])
def test_same_call_same_bits(i, bn):
    case = solved(i, bn, True)[0]
    first = run_layer(case)
    same_bits(first, run_layer(case))
    junk = [torch.randn(n, device=DEV) for n in (1000003, 77, 4099)]             # unrelated allocations move every buffer
    same_bits(first, run_layer(case))
    del junk
    torch.cuda.synchronize()
    same_bits(first, run_layer(case, stream=torch.cuda.Stream(DEV)))
    want = solved(i, bn, True)[3]
    for k, v in first.items():
        if v is not None:
            assert np.array_equal(v.cpu().numpy(), want[k]), k


@pytest.mark.parametrize("bn", [True, False])
def test_flags_skip_dx_and_dw_and_leave_the_rest(bn):
    case = solved(2, bn, True)[0]
    full = run_layer(case)
    no_dx = run_layer(case, need_dx=False)
    assert no_dx["dx"] is None
    no_dw = run_layer(case, need_dw=False)
    assert no_dw["dw"] is None
    neither = run_layer(case, need_dx=False, need_dw=False)
    assert neither["dx"] is None and neither["dw"] is None
    for part in (no_dx, no_dw, neither):
        same_bits({k: v for k, v in full.items() if part[k] is not None}, {k: v for k, v in part.items() if v is not None})


def test_autograd_function_honours_needs_input_grad():
    tl = pkg("pointnet2.train_layer")
    case = solved(2, True, True)[0]
    full = run_layer(case)
    x, w, gamma, beta = dev(case["x"]), dev(case["w"]).requires_grad_(True), dev(case["gamma"]).requires_grad_(True), dev(case["beta"]).requires_grad_(True)
    rm, rv = dev(case["running_mean"]), dev(case["running_var"])
    y = tl.TrainLayer.apply(x, w, gamma, beta, rm, rv, case["eps"], case["momentum"], True)
    y.backward(dev(case["dy"]))
    assert x.grad is None
    for got, k in ((y.detach(), "y"), (w.grad, "dw"), (gamma.grad, "dgamma"), (beta.grad, "dbeta"), (rm, "running_mean"), (rv, "running_var")):
        assert torch.equal(got, full[k]), k
    w.grad = None
    w.requires_grad_(False)
    x.requires_grad_(True)
    tl.TrainLayer.apply(x, w, gamma, beta, rm, rv, case["eps"], case["momentum"], True).backward(dev(case["dy"]))
    assert w.grad is None and torch.equal(x.grad, full["dx"])


def test_wrapper_argument_checks():
    case = solved(2, True, True)[0]
    x, w, g, be, dy = (dev(case[k]) for k in ("x", "w", "gamma", "beta", "dy"))
    fwd, bwd = ops().train_layer_forward_wrapper, ops().train_layer_backward_wrapper
    y, z, stats = fwd(x, w, g, be, 1e-5, 0.1, None, None, True)
    with pytest.raises(ValueError):
        fwd(x, w[:, :-1].contiguous(), g, be, 1e-5, 0.1, None, None, True)           # Cin differs
    with pytest.raises(ValueError):
        fwd(x, w, g[:-1].contiguous(), be, 1e-5, 0.1, None, None, True)
    with pytest.raises(ValueError):
        fwd(x, w, g, be, 1e-5, 0.1, g[:-1].contiguous(), None, True)
    with pytest.raises(ValueError):
        fwd(x[:, :, :0].contiguous(), w, g, be, 1e-5, 0.1, None, None, True)
    with pytest.raises(RuntimeError):
        fwd(x.double(), w, g, be, 1e-5, 0.1, None, None, True)
    with pytest.raises(RuntimeError):
        fwd(x.cpu(), w, g, be, 1e-5, 0.1, None, None, True)
    with pytest.raises(ValueError):
        bwd(dy[:, :-1].contiguous(), x, w, z, g, be, stats, True, True, True)
    with pytest.raises(ValueError):
        bwd(dy, x, w, z[:, :-1].contiguous(), g, be, stats, True, True, True)
    with pytest.raises(ValueError):
        bwd(dy, x, w, z, g, be, stats[:, :-1].contiguous(), True, True, True)
    with pytest.raises(ValueError):
        bwd(dy, x, w, None, None, None, None, True, True, True)                      # ReLU without the saved y
    L = pkg("_lib")
    with pytest.raises(L.PrcnnError):
        ops().train_layer_workspace_wrapper(0, 3, 3, 3)
    stat_n, dw_n = ops().train_layer_workspace_wrapper(3, 19, 130, 2 * chunk() + 3)
    assert stat_n == (3 * 3 + 1) * 2 * 130 and dw_n == 9 * 130 * 19
