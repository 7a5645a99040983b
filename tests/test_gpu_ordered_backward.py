"""-m gpu: the order-fixed, atomic-free backward of grouping, gather and three_interpolate (csrc/scatter_plan.hip; include/prcnn_hip.h
prcnn_scatter_plan, prcnn_group_points_grad_ordered, prcnn_three_interpolate_grad_ordered) against the numpy definitions of
tests/scatter_ref.py: the plan and the sums bit for bit, both paths against the f64 scatter-add inside the forward bound of a
fixed-order f32 sum, and the four autograd Functions under pointnet2_utils.ordered_backward().

Shapes are the smallest that cross the kernels' boundaries: n = 257 (no multiple of the 64 destinations of an ordering wave nor of
the 256 of a summing workgroup, more than one of each), c in {1, 7, 130} (below, no multiple of and beyond the 8 channels a thread
sums), lists of 0, 1, a few, 592, 1000 + 1500 (two lists that do not fit one ordering tile together) and 5000 slots (longer than the
ordering tile and than PRCNN_SCATTER_CHUNK, read from the header)."""
import types

import numpy as np
import pytest
import torch

import scatter_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def pu():
    return pkg("pointnet2.pointnet2_utils")


def ops():
    return pu().pointnet2


def chunk():
    return pkg("_lib").PRCNN_SCATTER_CHUNK


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(b, n, m, seed0):
    """xyz (b,n,3), the m furthest-point-sampled centres (b,m,3): device tensors"""
    xyz = dev(pkg("synth").scenes(b, n, seed0=seed0))
    sel = pu().furthest_point_sample(xyz, m)
    return xyz, torch.gather(xyz, 1, sel.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()


_INDEX, _REF_PLAN, _GPU_PLAN = {}, {}, {}


def index_case(name):
    """-> (idx (b, slots) i32 numpy, n); computed once"""
    if name in _INDEX:
        return _INDEX[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("base", "inrange"):
        n = 257
        idx = rng.integers(0, n, (3, 37 * 16)).astype(np.int32)
        idx[1] = 5                                                          # every slot on one point: 256 empty lists beside it
        if name == "base":
            idx[2, rng.choice(idx.shape[1], 40, replace=False)] = -1       # no list, nothing out of bounds
            idx[2, rng.choice(idx.shape[1], 40, replace=False)] = n
    elif name == "ball":                                                    # a real ball query: back-filled duplicates
        n = 2048
        xyz, new_xyz = scene(2, n, 512, 7)
        idx = pu().ball_query(2.0, 32, xyz, new_xyz).cpu().numpy().reshape(2, -1)
    elif name == "long":
        n = 300
        idx = rng.integers(0, n, (2, 9000)).astype(np.int32)
        idx[0, rng.choice(9000, 5000 - int((idx[0] == 7).sum()), replace=False, p=(idx[0] != 7) / (idx[0] != 7).sum())] = 7
        for k, cnt in ((3, 1500), (4, 1000), (70, 100)):
            free = np.nonzero(~np.isin(idx[1], (3, 4, 70)))[0]
            idx[1, rng.choice(free, cnt - int((idx[1] == k).sum()), replace=False)] = k
        assert (idx[0] == 7).sum() == 5000 and (idx[1] == 3).sum() == 1500 and (idx[1] == 4).sum() == 1000
    elif name == "one":
        n, idx = 1, np.array([[0, 0, 0, 0, 0], [0, 1, -1, 0, 0]], np.int32)
    elif name == "noslots":
        n, idx = 4, np.zeros((2, 0), np.int32)
    elif name == "nobatch":
        n, idx = 4, np.zeros((0, 6), np.int32)
    else:
        raise KeyError(name)
    _INDEX[name] = (idx, n)
    return _INDEX[name]


def ref_plan(name):
    if name not in _REF_PLAN:
        _REF_PLAN[name] = R.plan(*index_case(name))
    return _REF_PLAN[name]


def gpu_plan(name):
    if name not in _GPU_PLAN:
        idx, n = index_case(name)
        _GPU_PLAN[name] = ops().scatter_plan_wrapper(dev(idx), n)
    return _GPU_PLAN[name]


def same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert not np.isnan(got).any(), (what, "NaN survived: an element was not written")
    bad = np.nonzero(R.bits(got) != R.bits(want))
    assert len(bad[0]) == 0, (what, len(bad[0]), [int(x[0]) for x in bad], float(got[bad][0]), float(want[bad][0]))


# ------------------------------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("name", ["base", "ball", "long", "one", "noslots", "nobatch"])
def test_plan_equals_the_stable_argsort(name):
    idx, n = index_case(name)
    want_off, want_ent = ref_plan(name)
    pl = gpu_plan(name)
    torch.cuda.synchronize()
    assert tuple(pl.offsets.shape) == (len(idx), n + 1) and tuple(pl.entries.shape) == idx.shape and len(pl.tensors()) == 2
    off, ent = pl.offsets.cpu().numpy(), pl.entries.cpu().numpy()
    assert np.array_equal(off, want_off)
    for i in range(len(idx)):
        assert np.array_equal(ent[i][:off[i][n]], want_ent[i][:off[i][n]]), (name, i)
    if name == "ball":                                                       # the premise of this case: back-filled duplicates exist
        assert (np.diff(np.sort(idx.reshape(2, 512, 32), axis=2), axis=2) == 0).any()


def test_plan_is_a_pure_function_of_the_index():
    idx, n = index_case("long")
    a, b = ops().scatter_plan_wrapper(dev(idx), n), ops().scatter_plan_wrapper(dev(idx), n)
    assert torch.equal(a.offsets, b.offsets) and torch.equal(a.offsets, gpu_plan("long").offsets)
    total = int(a.offsets[0, n])
    assert torch.equal(a.entries[0, :total], b.entries[0, :total])


# ------------------------------------------------------------------------------------------------------------------------ 2. the sums
def run_group(name, c, c0=0, seed=0):
    idx, n = index_case(name)
    b, slots = idx.shape
    g = np.random.default_rng(seed).standard_normal((b, c0 + c, slots)).astype(np.float32)
    out = torch.full((b, c, n), float("nan"), device=DEV)
    ops().group_points_grad_ordered_wrapper(b, c, n, slots, c0 + c, c0, dev(g), gpu_plan(name), out)
    return out, g[:, c0:]


@pytest.mark.parametrize("name, c", [("base", 1), ("base", 7), ("base", 130), ("long", 7), ("ball", 9), ("one", 3), ("noslots", 3)])
def test_group_sums_equal_the_chunked_definition(name, c):
    got, g = run_group(name, c)
    n = index_case(name)[1]
    want = R.ordered_sum(*ref_plan(name), g, n, chunk())
    same_bits(got, want, (name, c))
    if name == "long":                                                       # the premise of this case: the chunk rule decides bits
        assert 5000 > chunk() and not np.array_equal(R.bits(want), R.bits(R.ordered_sum(*ref_plan(name), g, n, 1 << 20)))


@pytest.mark.parametrize("slots", [3000, 6000, 20000, 40000])
def test_group_sums_at_every_row_length_the_library_treats_differently(slots):
    """A row of grad_out is staged in LDS, 4 / 2 / 1 rows per workgroup (3000 / 6000 / 20000 slots; the cases above have 592 -- 8 rows --
    and 9000 and 16384 -- 2 rows above 64 KiB, the raised LDS limit), and 40000 slots (more than 128 KiB a row) are gathered through L2.
    c = 3 leaves a partial channel tile on every path."""
    rng = np.random.default_rng(slots)
    n, c = 70, 3
    idx = rng.integers(0, n, (2, slots)).astype(np.int32)
    g = rng.standard_normal((2, c, slots)).astype(np.float32)
    out = torch.full((2, c, n), float("nan"), device=DEV)
    ops().group_points_grad_ordered_wrapper(2, c, n, slots, c, 0, dev(g), ops().scatter_plan_wrapper(dev(idx), n), out)
    same_bits(out, R.ordered_sum(*R.plan(idx, n), g, n, chunk()), slots)


@pytest.mark.parametrize("name, c", [("base", 7), ("ball", 5)])
def test_group_sums_read_the_feature_channels_of_the_fused_gradient_in_place(name, c):
    got, g = run_group(name, c, c0=3, seed=1)
    same_bits(got, R.ordered_sum(*ref_plan(name), g, index_case(name)[1], chunk()), (name, c, "c_total = 3 + c, c0 = 3"))


def test_gather_form_is_the_group_form_with_one_sample():
    rng = np.random.default_rng(5)
    b, c, n, npoint = 3, 7, 257, 100
    idx = rng.integers(0, n, (b, npoint)).astype(np.int32)
    idx[:, :10] = idx[:, 10:20]                                              # repeated picks accumulate
    g = rng.standard_normal((b, c, npoint)).astype(np.float32)
    pl = ops().scatter_plan_wrapper(dev(idx), n)
    out = torch.full((b, c, n), float("nan"), device=DEV)
    ops().group_points_grad_ordered_wrapper(b, c, n, npoint, c, 0, dev(g), pl, out)
    same_bits(out, R.ordered_sum(*R.plan(idx, n), g, n, chunk()), "gather")


_INTERP = {}


def interp_case():
    """idx / weight of three_nn at n = 301 unknown, m = 40 known points -> numpy (idx (b,n,3), weight (b,n,3), m)"""
    if not _INTERP:
        xyz, known = scene(2, 301, 40, 21)
        dist, idx = pu().three_nn(xyz, known)
        inv = 1.0 / (dist + 1e-8)
        _INTERP["v"] = (idx.cpu().numpy(), (inv / inv.sum(dim=2, keepdim=True)).cpu().numpy().astype(np.float32), 40)
    return _INTERP["v"]


@pytest.mark.parametrize("weights", ["three_nn", "random"])
def test_interpolate_sums_equal_the_chunked_definition(weights):
    idx, w, m = interp_case()
    b, n, c = idx.shape[0], idx.shape[1], 7
    rng = np.random.default_rng(8)
    if weights == "random":
        w = rng.standard_normal(w.shape).astype(np.float32)
    g = rng.standard_normal((b, c, n)).astype(np.float32)
    pl = ops().scatter_plan_wrapper(dev(idx), m)
    out = torch.full((b, c, m), float("nan"), device=DEV)
    ops().three_interpolate_grad_ordered_wrapper(b, c, n, m, dev(g), dev(w), pl, out)
    same_bits(out, R.ordered_sum(*R.plan(idx.reshape(b, -1), m), R.interp_terms(g, w), m, chunk()), weights)


# ------------------------------------------------------------------------------------------------- 3. both paths against the f64 sum
def exact_and_bound(idx, terms64, n, extra):
    """-> (exact (b,c,n) f64, bound (b,c,n) f64): |got - exact| <= (L + extra) 2^-24 sum |term| for a list of L terms"""
    b, c, _ = terms64.shape
    exact, mass = np.zeros((b, c, n)), np.zeros((b, c, n))
    length = np.zeros((b, 1, n))
    for i in range(b):
        for ch in range(c):
            np.add.at(exact[i, ch], idx[i], terms64[i, ch])
            np.add.at(mass[i, ch], idx[i], np.abs(terms64[i, ch]))
        length[i, 0] = np.bincount(idx[i], minlength=n)
    return exact, (length + extra) * U * mass


def inside(got, exact, bound, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - exact)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(what, "largest error / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
    assert (err <= bound).all(), (what, worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("name", ["inrange", "ball", "long"])
def test_ordered_and_atomic_grouping_stay_inside_the_forward_bound(name):
    idx, n = index_case(name)
    b, slots, c = idx.shape[0], idx.shape[1], 7
    g = np.random.default_rng(2).standard_normal((b, c, slots)).astype(np.float32)
    exact, bound = exact_and_bound(idx, g.astype(np.float64), n, 0)
    ordered = torch.full((b, c, n), float("nan"), device=DEV)
    ops().group_points_grad_ordered_wrapper(b, c, n, slots, c, 0, dev(g), gpu_plan(name), ordered)
    atomic = torch.zeros((b, c, n), device=DEV)
    ops().group_points_grad_wrapper(b, c, n, slots, 1, dev(g), dev(idx), atomic)
    inside(ordered, exact, bound, name + " ordered")
    inside(atomic, exact, bound, name + " atomic")


def test_ordered_and_atomic_interpolate_stay_inside_the_forward_bound():
    idx, w, m = interp_case()
    b, n, c = idx.shape[0], idx.shape[1], 7
    g = np.random.default_rng(9).standard_normal((b, c, n)).astype(np.float32)
    terms64 = np.repeat(g.astype(np.float64), 3, axis=2) * w.astype(np.float64).reshape(b, 1, 3 * n)
    exact, bound = exact_and_bound(idx.reshape(b, -1), terms64, m, 1)        # + 1: the product's rounding
    ordered = torch.full((b, c, m), float("nan"), device=DEV)
    ops().three_interpolate_grad_ordered_wrapper(b, c, n, m, dev(g), dev(w), ops().scatter_plan_wrapper(dev(idx), m), ordered)
    atomic = torch.zeros((b, c, m), device=DEV)
    ops().three_interpolate_grad_wrapper(b, c, n, m, dev(g), dev(idx), dev(w), atomic)
    inside(ordered, exact, bound, "interpolate ordered")
    inside(atomic, exact, bound, "interpolate atomic")


# --------------------------------------------------------------------------------------------------------------------- 4. autograd
def test_gather_operation_backward_is_the_ordered_sum():
    rng = np.random.default_rng(12)
    idx = rng.integers(0, 257, (3, 100)).astype(np.int32)
    idx[:, :10] = idx[:, 10:20]
    g = rng.standard_normal((3, 7, 100)).astype(np.float32)
    feats = torch.randn((3, 7, 257), device=DEV, requires_grad=True)
    out = pu().gather_operation(feats, dev(idx))
    with pu().ordered_backward():
        grad, = torch.autograd.grad(out, feats, dev(g))
    same_bits(grad, R.ordered_sum(*R.plan(idx, 257), g, 257, chunk()), "GatherOperation")


def test_grouping_operation_backward_is_the_ordered_sum_and_repeats_its_bits():
    idx, n = index_case("inrange")
    g = np.random.default_rng(13).standard_normal((3, 7, 37, 16)).astype(np.float32)
    feats = torch.randn((3, 7, n), device=DEV, requires_grad=True)
    out = pu().grouping_operation(feats, dev(idx.reshape(3, 37, 16)))
    want = R.ordered_sum(*ref_plan("inrange"), g.reshape(3, 7, -1), n, chunk())
    with pu().ordered_backward():
        grads = [torch.autograd.grad(out, feats, dev(g), retain_graph=True)[0] for _ in range(3)]
    for k, grad in enumerate(grads):                                         # cloud 1 is the all-duplicates cloud
        same_bits(grad, want, "GroupingOperation, call %d" % k)


def test_three_interpolate_backward_is_the_ordered_sum():
    idx, w, m = interp_case()
    b, n = idx.shape[:2]
    g = np.random.default_rng(14).standard_normal((b, 7, n)).astype(np.float32)
    feats = torch.randn((b, 7, m), device=DEV, requires_grad=True)
    out = pu().three_interpolate(feats, dev(idx), dev(w))
    with pu().ordered_backward():
        grad, = torch.autograd.grad(out, feats, dev(g))
    same_bits(grad, R.ordered_sum(*R.plan(idx.reshape(b, -1), m), R.interp_terms(g, w), m, chunk()), "ThreeInterpolate")


def test_fused_query_and_group_backward_is_the_ordered_sum_of_the_whole_gradient():
    P = pu()
    xyz, new_xyz = scene(2, 2048, 512, 7)
    idx = P.ball_query(0.8, 32, xyz, new_xyz).cpu().numpy().reshape(2, -1)
    g = np.random.default_rng(15).standard_normal((2, 3 + 5, 512, 32)).astype(np.float32)
    feats = torch.randn((2, 5, 2048), device=DEV, requires_grad=True)
    out = P._QueryAndGroupFused.apply(0.8, 32, xyz, new_xyz, feats)
    with P.ordered_backward():
        grad, = torch.autograd.grad(out, feats, dev(g))
    same_bits(grad, R.ordered_sum(*R.plan(idx, 2048), g[:, 3:].reshape(2, 5, -1), 2048, chunk()), "_QueryAndGroupFused")


def t_group(features, idx):
    """features (B,C,N), idx (B,M,ns) -> (B,C,M,ns) by torch.gather (differentiable: backward = scatter-add)"""
    B, C, N = features.shape
    M, ns = idx.shape[1], idx.shape[2]
    flat = idx.long().view(B, 1, M * ns).expand(-1, C, -1)
    return torch.gather(features, 2, flat).view(B, C, M, ns)


def t_interpolate(feats, idx, w):
    """feats (B,C,m), idx / w (B,n,3) -> (B,C,n): w0 f[i0] + w1 f[i1] + w2 f[i2]"""
    B, C, m = feats.shape
    n = idx.shape[1]
    out = 0
    for k in range(3):
        g = torch.gather(feats, 2, idx[:, :, k].long().view(B, 1, n).expand(-1, C, -1))
        out = out + g * w[:, :, k].unsqueeze(1)
    return out


def sa_reference(mod, xyz, features, P):
    sel = P.furthest_point_sample(xyz, mod.npoint)
    new_xyz = torch.gather(xyz, 1, sel.long().unsqueeze(-1).expand(-1, -1, 3))
    outs = []
    for grouper, mlp in zip(mod.groupers, mod.mlps):
        idx = P.ball_query(grouper.radius, grouper.nsample, xyz, new_xyz.contiguous())
        rel = t_group(xyz.transpose(1, 2), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
        grouped = torch.cat([rel, t_group(features, idx)], dim=1)
        y = mlp(grouped)
        outs.append(torch.nn.functional.max_pool2d(y, kernel_size=[1, y.size(3)]).squeeze(-1))
    return new_xyz, torch.cat(outs, dim=1)


def fp_reference(mod, unknown, known, skip, known_feats, P):
    dist, idx = P.three_nn(unknown, known)
    inv = 1.0 / (dist + 1e-8)
    w = inv / torch.sum(inv, dim=2, keepdim=True)
    carried = t_interpolate(known_feats, idx, w)
    stacked = torch.cat([carried, skip], dim=1).unsqueeze(-1)
    return mod.mlp(stacked).squeeze(-1)


def sa_fp_graph(fused, ordered):
    """The SA-MSG + FP graph of tests/test_gpu_autograd.py (same modules, shapes and seeds) -> [(out, coarse, d features, d parameters)]
    for the modules and for their torch.gather twin"""
    PM, P = pkg("pointnet2.pointnet2_modules"), pu()
    torch.manual_seed(4)
    B, N, M, C = 3, 2048, 512, 24
    xyz = torch.from_numpy(pkg("synth").scenes(B, N, seed0=60)).to(DEV)
    sa = PM.PointnetSAModuleMSG(npoint=M, radii=[0.8, 1.6], nsamples=[16, 32], mlps=[[C, 32, 48], [C, 32, 64]], use_xyz=True, bn=True).to(DEV)
    fp = PM.PointnetFPModule(mlp=[48 + 64 + C, 64, 32], bn=True).to(DEV)
    sa.train(); fp.train()
    base = torch.randn((B, C, N), device=DEV)
    target = torch.randn((B, 32, N), device=DEV)
    results = []
    saved = P.REFERENCE_ORDER
    for which in ("modules", "torch"):
        feats = base.clone().requires_grad_(True)
        for p in list(sa.parameters()) + list(fp.parameters()):
            p.grad = None
        if which == "modules":
            P.REFERENCE_ORDER = not fused
            try:
                new_xyz, coarse = sa(xyz, feats)
                out = fp(xyz, new_xyz, feats, coarse)
            finally:
                P.REFERENCE_ORDER = saved
        else:
            new_xyz, coarse = sa_reference(sa, xyz, feats, P)
            out = fp_reference(fp, xyz, new_xyz.contiguous(), feats, coarse, P)
        loss = ((out - target) ** 2).mean() + coarse.abs().mean()
        with P.ordered_backward(ordered and which == "modules"):
            loss.backward()
        torch.cuda.synchronize()
        results.append((out.detach().clone(), coarse.detach().clone(), feats.grad.detach().clone(),
                        [p.grad.detach().clone() for p in list(sa.parameters()) + list(fp.parameters())]))
    return results


def counted(monkeypatch):
    """wrap the three ordered wrappers of the extension module with call counters -> the counter dict"""
    calls = {}
    for name in ("scatter_plan_wrapper", "group_points_grad_ordered_wrapper", "three_interpolate_grad_ordered_wrapper"):
        def wrap(*a, _fn=getattr(ops(), name), _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **kw)
        monkeypatch.setattr(ops(), name, wrap)
    return calls


@pytest.mark.parametrize("fused", [True, False], ids=["fused_query_and_group", "reference_order"])
def test_ordered_backward_through_sa_and_fp_modules_equals_torch_gather_graph(fused, monkeypatch):
    calls = counted(monkeypatch)
    (o1, c1, g1, p1), (o2, c2, g2, p2) = sa_fp_graph(fused, ordered=True)
    # two scales (fused: one grouping each; reference order: the xyz grouping carries no gradient) and one interpolation
    assert calls == {"scatter_plan_wrapper": 3, "group_points_grad_ordered_wrapper": 2, "three_interpolate_grad_ordered_wrapper": 1}, calls
    assert float(g1.abs().max()) > 0 and all(float(p.abs().max()) > 0 for p in p1)

    def close(a, b, what):
        scale = max(1e-6, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-7, (what, float((a - b).abs().max()), scale)
    close(o1, o2, "fp output"); close(c1, c2, "sa output"); close(g1, g2, "d loss / d features")
    for k, (a, b) in enumerate(zip(p1, p2)):
        close(a, b, "parameter %d" % k)


def test_switch_off_never_reaches_the_ordered_entries(monkeypatch):
    calls = counted(monkeypatch)
    assert pu().ORDERED_BACKWARD is False and not torch.are_deterministic_algorithms_enabled()
    sa_fp_graph(True, ordered=False)
    assert calls == {}


def test_deterministic_algorithms_select_the_ordered_path(monkeypatch):
    calls = counted(monkeypatch)
    feats = torch.randn((2, 3, 50), device=DEV, requires_grad=True)
    idx = torch.randint(0, 50, (2, 20), device=DEV, dtype=torch.int32)
    out = pu().gather_operation(feats, idx)
    torch.use_deterministic_algorithms(True)
    try:
        torch.autograd.grad(out, feats, torch.ones_like(out))
    finally:
        torch.use_deterministic_algorithms(False)
    assert calls == {"scatter_plan_wrapper": 1, "group_points_grad_ordered_wrapper": 1}


@pytest.mark.parametrize("missing", ["scatter_plan_wrapper", "group_points_grad_ordered_wrapper", "three_interpolate_grad_ordered_wrapper"])
def test_missing_entry_raises_by_name_and_never_falls_back(missing, monkeypatch):
    P = pu()
    real = P.pointnet2
    stand_in = types.SimpleNamespace(**{k: getattr(real, k) for k in dir(real) if not k.startswith("__") and k != missing})
    stand_in.__name__ = "stand_in_without_" + missing
    fell_back = []
    for name in ("group_points_grad_wrapper", "gather_points_grad_wrapper", "three_interpolate_grad_wrapper"):
        setattr(stand_in, name, lambda *a, _n=name, **kw: fell_back.append(_n))
    monkeypatch.setattr(P, "pointnet2", stand_in)
    feats = torch.randn((2, 3, 50), device=DEV, requires_grad=True)
    if missing == "three_interpolate_grad_ordered_wrapper":
        out = P.three_interpolate(feats, torch.randint(0, 50, (2, 20, 3), device=DEV, dtype=torch.int32), torch.rand((2, 20, 3), device=DEV))
    else:
        out = P.gather_operation(feats, torch.randint(0, 50, (2, 20), device=DEV, dtype=torch.int32))
    with P.ordered_backward():
        with pytest.raises(RuntimeError, match=missing):
            torch.autograd.grad(out, feats, torch.ones_like(out))
    assert fell_back == []
