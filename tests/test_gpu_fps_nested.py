"""-m gpu: prcnn_fps_new_xyz_nested (csrc/fps_prefix.hip) gives prcnn_fps_new_xyz's outputs bit for bit on ANY input -- clouds in pick order
(accepted by the prefix check: the sampling kernels skip them), raw clouds, lattices, duplicates, NaN / inf (rejected: sampled as
before) and batches that mix the two, in both arithmetic modes and at the smallest size of every kernel route; the check's per-cloud
verdict equals the numpy predicate of tests/test_fps_prefix_predicate.py; and the engine's detections do not depend on the route."""
import numpy as np
import pytest
import torch

from conftest import pkg
from test_fps_prefix_predicate import prefix_predicate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture()
def arithmetic():
    """-> set(mode); the library's default (0) is restored afterwards"""
    L = pkg("_lib")
    yield lambda mode: L.call("prcnn_set_fps_arithmetic", mode)
    L.call("prcnn_set_fps_arithmetic", 0)


def lattice(n, seed=5):
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(len(g))][:n].astype(np.float32)


def both_entries(P, x, m):
    """-> the check's verdict; asserts nested == plain, bit for bit"""
    want_idx, want_xyz = P.fps_new_xyz_wrapper(x, m)
    got_idx, got_xyz = P.fps_new_xyz_nested_wrapper(x, m)
    rejected = P.fps_prefix_check_wrapper(x, m) if P.fps_new_xyz_nested_supported(x.shape[1], m) else None
    torch.cuda.synchronize()
    assert torch.equal(got_idx, want_idx)
    assert torch.equal(got_xyz.view(torch.int32), want_xyz.view(torch.int32))          # bits: NaN coordinates compare too
    return want_idx, rejected


# (b, outer n, n, m): the smallest shape of every route a nested level can take
ROUTES = [(4, 1024, 256, 64),        # fps_reg_kernel<1, 4>
          (4, 2048, 1024, 256),      # fps_reg_kernel<4, 4>
          (128, 2048, 1024, 256),    # fps_reg_kernel<1, 16>: many clouds, a wave each
          (2, 8192, 4096, 1024),     # fps_order_kernel + fps_spec_kernel<4>
          (3, 4096, 2049, 256),      # ragged: the last tile of the speculative kernel holds one point
          (2, 4096, 1500, 300),      # 1024 < n <= 2048: fps_reg_kernel<16, 4> over the internal distance scratch + the gather
          (1, 32768, 16384, 4096)]   # fps_spec_kernel<16> with a flag (not a shape of the engine)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("b,n0,n,m", ROUTES)
def test_nested_entry_equals_the_plain_entry(ext, oracle, arithmetic, mode, b, n0, n, m):
    """the batch: b clouds in pick order (the plain entry's own n0 -> n sampling), one raw cloud and one lattice behind them -- one
    launch both skips and samples"""
    P, S = ext.pointnet2, pkg("synth")
    arithmetic(mode)
    raw = S.scenes(b + 1, n0, seed0=n + m)
    _, nested = P.fps_new_xyz_wrapper(T(raw[:b]), n)
    x = torch.cat([nested, T(raw[b:, :n]), T(np.resize(lattice(min(n, 4096)), (1, n, 3)))], 0).contiguous()
    idx, rejected = both_entries(P, x, m)
    rej = rejected.cpu().numpy()
    print("b=%d %d -> %d mode %d: rejected %s" % (b, n, m, mode, rej[:b].sum()), rej[b:])
    assert rej[:b].sum() <= max(1, b // 16) and rej[b] == 1                            # pick order: accepted; a raw cloud: rejected at once
    assert (idx[:b][torch.from_numpy(rej[:b] == 0).to(DEV)] == torch.arange(m, device=DEV, dtype=torch.int32)).all()
    if b <= 4:                                                                         # every route: the oracle's picks, and
        xs = x.cpu().numpy()
        assert np.array_equal(idx.cpu().numpy(), oracle.furthest_point_sample(xs, m, hipcc_arithmetic=bool(mode)))
        if mode == 0:                                                                  # the verdict is the predicate's, cloud by cloud
            want = [0 if prefix_predicate(c, m, oracle.opt_n_threads(n))[0] else 1 for c in xs]
            assert rej.tolist() == want


def test_nested_entry_on_ties_copies_and_non_finite_clouds(ext, oracle, arithmetic):
    """lattices in pick order (the oracle returns a non-prefix for 16^3 -> 1024 -> 256), clouds of copies sampled to more points than are
    distinct (zero minima: picks fall back to 0), m = n, m = 1, and a NaN / an infinity at a pivot and behind the pivots"""
    P, S = ext.pointnet2, pkg("synth")
    _, lat1024 = P.fps_new_xyz_wrapper(T(lattice(4096)[None]), 1024)
    idx, rejected = both_entries(P, lat1024, 256)
    _, lat256 = P.fps_new_xyz_wrapper(lat1024, 256)
    idx2, rejected2 = both_entries(P, lat256, 64)
    xs = lat1024.cpu().numpy()
    assert np.array_equal(idx.cpu().numpy(), oracle.furthest_point_sample(xs, 256))
    assert int(rejected) == (0 if prefix_predicate(xs[0], 256, oracle.opt_n_threads(1024))[0] else 1)
    assert int(rejected) + int(rejected2) >= 1
    few = np.repeat(S.scene(4, 100), 4, axis=0)[np.random.default_rng(9).permutation(400)][None]
    _, few200 = P.fps_new_xyz_wrapper(T(few), 200)
    idx, rejected = both_entries(P, few200, 150)
    assert int(rejected) == 1 and np.array_equal(idx.cpu().numpy(), oracle.furthest_point_sample(few200.cpu().numpy(), 150))
    _, base = P.fps_new_xyz_wrapper(T(S.scenes(3, 1024, seed0=21)), 128)
    both_entries(P, base, 128)                                                         # m = n
    idx, rejected = both_entries(P, base, 1)                                           # m = 1: outside the check, the plain entry inside
    assert rejected is None and (idx == 0).all()
    for bad in (float("nan"), float("inf")):
        for where in (0, 7, 100):
            x = base.clone()
            x[1, where, 1] = bad
            _, rejected = both_entries(P, x, 32)
            assert rejected.tolist() == [0, 1, 0], (bad, where, rejected.tolist())


@pytest.mark.parametrize("b,n,m", [(5, 256, 64), (5, 1024, 256), (130, 1024, 256), (3, 4096, 1024), (3, 1500, 300), (2, 16384, 4096)])
def test_sampling_kernels_leave_an_accepted_cloud_alone(ext, b, n, m):
    """the skip itself, which no output comparison can see: the sampling launches under a hand-made verdict (prcnn_fps_new_xyz_flagged)
    -- a cloud flagged 0 keeps the sentinel its outputs were filled with although it is a RAW cloud, one flagged 1 is sampled as by
    the plain entry; every kernel route of the nested entry"""
    P, S = ext.pointnet2, pkg("synth")
    x = T(S.scenes(b, n, seed0=7 * n + m))
    want_idx, want_xyz = P.fps_new_xyz_wrapper(x, m)
    flags = torch.tensor([c % 2 for c in range(b)], dtype=torch.int32, device=DEV)
    idx = torch.full((b, m), 1, dtype=torch.int32, device=DEV)          # (a valid index: the gather route reads it)
    new_xyz = torch.full((b, m, 3), -7.0, device=DEV)
    P.fps_new_xyz_flagged_wrapper(x, m, flags, idx, new_xyz)
    torch.cuda.synchronize()
    run, skip = flags.bool(), ~flags.bool()
    assert torch.equal(idx[run], want_idx[run]) and torch.equal(new_xyz[run], want_xyz[run])
    if n <= 1024 or (n > 2048 and m >= 256):                                           # (the gather route rewrites new_xyz from idx for every cloud)
        assert (new_xyz[skip] == -7.0).all()
    assert (idx[skip] == 1).all()                                                      # (a sampled cloud starts with pick 0)


def test_engine_takes_the_nested_entry(monkeypatch):
    """_geometry_level hands the hint over as PrefixExpected(npoint): levels 1.. up to NESTED_FPS_MAX_N points reach
    prcnn_fps_new_xyz_nested, level 0 and larger clouds prcnn_fps_new_xyz"""
    C, E, F, S, L = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer"), pkg("synth"), pkg("_lib")
    cfg = C.default_eval_cfg()
    eng = F.FastPointRCNN(E.build_model(cfg, DEV, seed=0), cfg)
    x = torch.from_numpy(S.scenes(2, 16384, seed0=3)).to(DEV)
    seen, real = [], L.call

    def spy(name, *args):
        if name.startswith("prcnn_fps_new_xyz"):
            seen.append((name, args[1]))
        return real(name, *args)
    monkeypatch.setattr(L, "call", spy)
    for limit, want in ((4096, ["", "_nested", "_nested", "_nested"]), (1024, ["", "", "_nested", "_nested"]), (0, ["", "", "", ""])):
        monkeypatch.setattr(F, "NESTED_FPS_MAX_N", limit)
        del seen[:]
        eng.geometry(x)
        assert seen == [("prcnn_fps_new_xyz" + w, n) for w, n in zip(want, (16384, 4096, 1024, 256))], (limit, seen)


@pytest.mark.parametrize("scene", ["uniform", "lidar"])
def test_engine_detections_do_not_depend_on_the_nested_route(scene, monkeypatch):
    """one geometry group (4 batches) through the product runner with PRCNN_NESTED_FPS's two settings: every detection tensor bit for
    bit -- and the levels' clouds ARE accepted, so the default run took the skipping route"""
    C, E, F, S, pu = pkg("config"), pkg("eval_rcnn"), pkg("net.fast_infer"), pkg("synth"), pkg("pointnet2.pointnet2_utils")
    dev = torch.device("cuda", 0)
    cfg = C.default_eval_cfg()
    model = E.build_model(cfg, dev, seed=0)
    make = S.lidar_scenes if scene == "lidar" else S.scenes
    batches = [torch.from_numpy(make(4, 16384, seed0=100 + 4 * s)).to(dev) for s in range(4)]
    keys = ("boxes", "scores", "num", "pred_boxes3d", "rois", "rcnn_cls", "rcnn_reg")

    def run():
        runner = E.make_runner(model, cfg, dev)
        outs = []

        def take(det):
            if det is not None:
                with torch.cuda.stream(det["stream"]):
                    outs.append({k: det[k].clone() for k in keys})
        for i, b in enumerate(batches):
            take(runner.submit(b, batches[i + 1:i + 1 + runner.depth]))
        while True:
            det = runner.flush()
            if det is None:
                break
            take(det)
        torch.cuda.synchronize()
        return outs
    monkeypatch.setattr(F, "NESTED_FPS_MAX_N", 4096)                                   # every nested level through the check
    got = run()
    monkeypatch.setattr(F, "NESTED_FPS_MAX_N", 0)
    want = run()
    assert len(got) == len(want) == 4 and sum(int(w["num"].sum()) for w in want) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            assert torch.equal(g[k], w[k]), "batch %d: %s" % (i, k)
    geo = F.FastPointRCNN(model, cfg).geometry(batches[0])
    rejected = sum(int(pu.pointnet2.fps_prefix_check_wrapper(a, b.shape[1]).sum()) for a, b in zip(geo["l_xyz"][1:], geo["l_xyz"][2:]))
    assert rejected <= 1, rejected
