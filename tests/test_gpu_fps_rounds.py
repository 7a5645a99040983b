"""-m gpu: the rounds of the speculative sampling kernels (csrc/fps_spec.hip) on the clouds that decide whether a round's parts are
right -- the wave-level pivot cull in front of the tile tests, the lazy rebuild of a wave's entries, the merge -- at the smallest
shapes at which they can go wrong.  Everywhere: the picks equal oracle.furthest_point_sample's, the handed-back running minima
equal its minima bit for bit, in both distance arithmetics, through the (idx, temp) entry, through the new_xyz entry, and with a
`rejected` flag that leaves one cloud of the batch alone.

B = 3 throughout, so that a workgroup's cloud is not cloud 0.  The clouds:
  route edges      n = 2049 .. 16384, m = n / 4: the first and last size of fps_spec_kernel<4>, <8>, <16>; at n = 2049 fifteen waves hold
                   no point or one (empty boxes, bounds of -inf)
  clusters         sixteen tight clusters on a 4 x 4 grid in (x, z), n / 16 points each: in Morton order a wave IS a cluster, every
                   pivot of a round survives the wave-level cull in exactly one wave
  one box          all but 16 points in one small box: the far points' waves' boxes span the scene, nearly every pivot reaches one wave
  ties             an integer lattice, and integer points that each occur eight times (m beyond the distinct points: zero minima)
  exhaustion       m = n = 2049 with 64 points twice: the run goes on until every minimum is 0, 64 rounds of one pick on zeros follow
  resumed          `temp` handed in as a first call with a smaller m left it
  two workgroups   n = 16385: fps_spec2_kernel, whose tile tests and rebuild are copies of fps_spec_kernel<16>'s"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3


def T(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # (a copy: the shared references are read-only)


def routes(n):
    return pkg("synth").scenes(B, n, seed0=n).astype(np.float32)


def run_dry(n):
    xyz = routes(n).copy()
    xyz[:, -64:] = xyz[:, 100:164]                  # 64 points twice: every minimum is 0 after n - 64 picks, 64 picks follow
    return xyz


def clusters(n):
    rng = np.random.default_rng(n)
    per = n // 16
    out = np.empty((B, n, 3), np.float32)
    for c in range(B):
        centres = np.array([[20.0 * (k % 4) - 30.0, 0.5 * (k % 3), 20.0 * (k // 4) + 5.0] for k in range(16)])
        pts = np.repeat(centres, per, axis=0) + rng.uniform(-0.4 - 0.1 * c, 0.4 + 0.1 * c, (16 * per, 3))
        out[c] = pts[rng.permutation(n)]
    return out


def one_box(n):
    rng = np.random.default_rng(n + 1)
    out = np.empty((B, n, 3), np.float32)
    for c in range(B):
        pts = rng.uniform(-1.0, 1.0, (n, 3)) * [1.5, 0.5, 1.5] + [3.0 * c, 0.0, 20.0]
        pts[:16] = rng.uniform(-1.0, 1.0, (16, 3)) * [40.0, 1.0, 35.0] + [0.0, 0.0, 35.0]
        out[c] = pts[rng.permutation(n)]
    return out


def lattice(n):
    g = np.stack(np.meshgrid(np.arange(32), np.arange(16), np.arange(17), indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(n + 2)
    return np.stack([g[rng.permutation(len(g))][:n] for _ in range(B)], 0).astype(np.float32)


def copies(n):
    rng = np.random.default_rng(n + 3)
    out = np.empty((B, n, 3), np.float32)
    for c in range(B):
        base = rng.integers(-60, 61, size=(n // 8, 3)).astype(np.float32)
        out[c] = np.resize(base, (n, 3))[rng.permutation(n)]
    return out


# name -> (builder, n, m)
CASES = {}
for _n in (2049, 4096, 4097, 8192, 8193, 16384):
    CASES["route-%d" % _n] = (routes, _n, _n // 4)
CASES.update({
    "clusters-4096": (clusters, 4096, 1024), "clusters-16384": (clusters, 16384, 2048),
    "one-box-8193": (one_box, 8193, 1024), "one-box-16384": (one_box, 16384, 2048),
    "lattice-4097": (lattice, 4097, 1024), "lattice-8193": (lattice, 8193, 2048),
    "copies-4097": (copies, 4097, 600), "copies-8193": (copies, 8193, 1100),
    "exhaustion-2049": (run_dry, 2049, 2049),
    "two-workgroups-16385": (routes, 16385, 512),
})
_cache = {}


def reference(oracle, name, mode):
    """-> (xyz, m, picks, minima) of the case; computed once per case and arithmetic, never written to"""
    if (name, mode) not in _cache:
        build, n, m = CASES[name]
        xyz = build(n)
        assert xyz.shape == (B, n, 3) and xyz.dtype == np.float32 and np.isfinite(xyz).all()
        idx, temp = oracle.furthest_point_sample(xyz, m, return_temp=True, hipcc_arithmetic=bool(mode))
        for a in (xyz, idx, temp):
            a.setflags(write=False)
        _cache[(name, mode)] = (xyz, m, idx, temp)
    return _cache[(name, mode)]


@pytest.fixture()
def arithmetic():
    """-> set(mode); the library's default (0) is restored afterwards"""
    L = pkg("_lib")
    yield lambda mode: L.call("prcnn_set_fps_arithmetic", mode)
    L.call("prcnn_set_fps_arithmetic", 0)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_picks_and_minima_equal_the_oracle(ext, oracle, arithmetic, name, mode):
    """the (idx, temp) entry: indices equal, running minima bit-equal"""
    xyz, m, want, wtemp = reference(oracle, name, mode)
    arithmetic(mode)
    n = xyz.shape[1]
    temp = torch.full((B, n), 1e10, device=DEV)
    idx = torch.empty((B, m), dtype=torch.int32, device=DEV)
    ext.pointnet2.furthest_point_sampling_wrapper(B, n, m, T(xyz), temp, idx)
    got, gtemp = idx.cpu().numpy(), temp.cpu().numpy()
    first = np.argwhere(got != want)
    assert first.size == 0, "first differing pick (cloud, position): %s" % first[0]
    assert np.array_equal(gtemp.view(np.int32), wtemp.view(np.int32))
    if name.startswith("exhaustion"):                                                  # it did run dry: 64 picks on minima that are all 0
        assert (wtemp == 0).all() and all(len(np.unique(r)) < m for r in want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_new_xyz_entry_and_a_cloud_left_alone(ext, oracle, arithmetic, name, mode):
    """prcnn_fps_new_xyz: the same picks with their coordinates; prcnn_fps_new_xyz_flagged with rejected = (1, 0, 1): the middle cloud
    keeps the sentinels its outputs held, the others are sampled as before"""
    xyz, m, want, _ = reference(oracle, name, mode)
    arithmetic(mode)
    P, x = ext.pointnet2, T(xyz)
    idx, new_xyz = P.fps_new_xyz_wrapper(x, m)
    wxyz = np.take_along_axis(xyz, want.astype(np.int64)[..., None].repeat(3, -1), 1)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(new_xyz.cpu().numpy().view(np.int32), wxyz.view(np.int32))
    if xyz.shape[1] > 16384:                                                           # (the flagged entry: one workgroup per cloud)
        return
    flags = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    fidx = torch.full((B, m), 1, dtype=torch.int32, device=DEV)
    fxyz = torch.full((B, m, 3), -7.0, device=DEV)
    P.fps_new_xyz_flagged_wrapper(x, m, flags, fidx, fxyz)
    torch.cuda.synchronize()
    assert torch.equal(fidx[0::2], idx[0::2]) and torch.equal(bits(fxyz[0::2]), bits(new_xyz[0::2]))
    assert (fidx[1] == 1).all() and (fxyz[1] == -7.0).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m0,m", [(4097, 100, 1024), (16384, 64, 2048)])
def test_resumed_minima(ext, oracle, arithmetic, mode, n, m0, m):
    """`temp` handed in already lowered -- as a first call with m0 picks left it -- and sampling run again over it: the oracle's own
    scan, started on the same minima, gives the same picks and the same minima"""
    xyz, _, _, _ = reference(oracle, "route-%d" % n, mode)
    _, temp0 = oracle.furthest_point_sample(xyz, m0, return_temp=True, hipcc_arithmetic=bool(mode))
    wtemp, want = temp0.copy(), np.empty((B, m), np.int32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    args = (xyz.ctypes.data_as(fp), wtemp.ctypes.data_as(fp), want.ctypes.data_as(ip))
    if mode:
        oracle.lib().orc_furthest_point_sampling_hipcc_bs(B, n, m, int(oracle.lib().orc_opt_n_threads(n)), *args)
    else:
        oracle.lib().orc_furthest_point_sampling(B, n, m, *args)
    assert (wtemp <= temp0).all() and (wtemp < temp0).any()
    arithmetic(mode)
    temp = torch.full((B, n), 1e10, device=DEV)
    idx0 = torch.empty((B, m0), dtype=torch.int32, device=DEV)
    ext.pointnet2.furthest_point_sampling_wrapper(B, n, m0, T(xyz), temp, idx0)
    assert np.array_equal(temp.cpu().numpy().view(np.int32), temp0.view(np.int32))
    idx = torch.empty((B, m), dtype=torch.int32, device=DEV)
    ext.pointnet2.furthest_point_sampling_wrapper(B, n, m, T(xyz), temp, idx)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(temp.cpu().numpy().view(np.int32), wtemp.view(np.int32))
