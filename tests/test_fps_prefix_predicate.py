"""The acceptance predicate of the nested sampling entry (prcnn_fps_new_xyz_nested, csrc/fps_prefix.hip: fps_prefix_check_kernel), restated
in numpy and held against the CPU oracle: a cloud the predicate ACCEPTS must be sampled by oracle.furthest_point_sample to the prefix
0 .. m-1, with the running minima the predicate computed.  The predicate never looks at the oracle's answer; it is the definition the
GPU kernels implement (tests/test_gpu_fps_nested.py compares them with it):

    T_s[j] = min(1e10, min_{i < s} d(P[j], P[i])),  D[s] = T_s[s];  accepted  <=>  every coordinate is finite and for s = 1 .. m-1:
    D[s] > 0  and for every j > s:  D[s] > T_s[j]  or  (D[s] == T_s[j] and key(s) < key(j))

d is the squared distance of sampling_gpu.cu:133 in f32, one rounding per operation; key is the reference's tie order for a block of
opt_n_threads(n) threads: (bit-reversed k mod bs, k div bs).  The running minima FPS hands back hold the pivots 0 .. m-2 (the last
pick updates nothing): T_{m-1}."""
import numpy as np
import pytest

from conftest import pkg


def tie_keys(n, bs):
    k = np.arange(n, dtype=np.int64)
    low, bits = k % bs, int(bs).bit_length() - 1
    rev = np.zeros(n, np.int64)
    for i in range(bits):
        rev |= ((low >> i) & 1) << (bits - 1 - i)
    return rev * (n // bs + 1) + k // bs                   # lexicographic (rev, k div bs) as one integer


def sqdist(P, q):
    d = P - q                                               # float32 throughout: one rounding per operation
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def prefix_predicate(P, m, bs):
    """-> (accepted, T_{m-1} or None)"""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P)
    assert 1 <= m <= n
    if not np.isfinite(P).all():
        return False, None
    key = tie_keys(n, bs)
    T = np.full(n, 1e10, np.float32)
    with np.errstate(over="ignore"):
        for s in range(1, m):
            T = np.minimum(T, sqdist(P, P[s - 1]))
            D = T[s]
            if not D > 0:
                return False, None
            rest = T[s + 1:]
            if not ((D > rest) | ((D == rest) & (key[s] < key[s + 1:]))).all():
                return False, None
    return True, T


def check_implication(oracle, clouds, m):
    """accepted => the oracle's picks are the prefix and its running minima the predicate's; -> accepted flags"""
    clouds = np.ascontiguousarray(clouds, np.float32)
    n = clouds.shape[1]
    bs = oracle.opt_n_threads(n)
    want_idx, want_temp = oracle.furthest_point_sample(clouds, m, return_temp=True)
    flags = []
    for c, P in enumerate(clouds):
        ok, T = prefix_predicate(P, m, bs)
        flags.append(ok)
        if ok:
            assert np.array_equal(want_idx[c], np.arange(m)), c
            assert np.array_equal(want_temp[c], T), c
    return np.array(flags), want_idx


def gather(clouds, idx):
    return np.take_along_axis(clouds, idx.astype(np.int64)[..., None].repeat(3, -1), 1)


def nested_levels(oracle, clouds, sizes):
    """clouds sampled to sizes[0] by the oracle, then the predicate at sizes[0] -> sizes[1] -> ...; -> accepted flags per level"""
    cur = gather(clouds, oracle.furthest_point_sample(clouds, sizes[0]))
    out = []
    for m in sizes[1:]:
        flags, idx = check_implication(oracle, cur, m)
        out.append(flags)
        cur = gather(cur, idx)
    return out


@pytest.mark.parametrize("kind", ["uniform", "lidar"])
def test_nested_clouds_of_a_scene_are_accepted(oracle, kind):
    """2048 -> 512 by the oracle, then 512 -> 128 -> 32: what the RPN's levels 1.. see.  At most 1 cloud in 16 rejected."""
    S = pkg("synth")
    clouds = S.scenes(16, 2048, seed0=300) if kind == "uniform" else np.stack([S.lidar_scene(300 + i, 2048) for i in range(16)], 0)
    for level, flags in enumerate(nested_levels(oracle, clouds, (512, 128, 32))):
        print(kind, "level", level, "accepted", int(flags.sum()), "of", len(flags))
        assert (~flags).sum() <= 1, (kind, level, flags)


def test_raw_clouds_are_rejected(oracle):
    """a cloud that is NOT in pick order: point 1 is not the furthest from point 0"""
    S = pkg("synth")
    flags, _ = check_implication(oracle, S.scenes(4, 512, seed0=11), 128)
    assert not flags.any()


def test_integer_lattice_is_rejected_at_some_level(oracle):
    """16^3 lattice, shuffled: thousands of exact ties, and the tie key changes with n -- the oracle returns a non-prefix"""
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    lat = g[np.random.default_rng(5).permutation(len(g))].astype(np.float32)[None]
    levels = nested_levels(oracle, lat, (1024, 256, 64))
    assert not all(f.all() for f in levels), levels


def test_duplicates_m_equal_n_and_m_one(oracle):
    S = pkg("synth")
    rng = np.random.default_rng(9)
    # every point four times, sampled down to fewer points than are distinct: nested levels without a zero minimum
    dup = np.repeat(S.scene(3, 256), 4, axis=0)[None]
    dup = dup[:, rng.permutation(dup.shape[1])]
    for flags in nested_levels(oracle, dup, (200, 64)):
        assert flags.shape == (1,)
    # ... and to MORE than are distinct: the picks past the 100th are copies of point 0 (running minima all 0): D[s] = 0 rejects
    few = np.repeat(S.scene(4, 100), 4, axis=0)[None]
    few = few[:, rng.permutation(few.shape[1])]
    (flags,) = nested_levels(oracle, few, (200, 150))
    assert not flags.any()
    # m = n: every point picked; m = 1: nothing to decide, always the prefix
    base = S.scenes(3, 1024, seed0=21)
    (flags,) = nested_levels(oracle, base, (128, 128))
    assert (~flags).sum() <= 1
    flags, idx = check_implication(oracle, base[:, :300], 1)
    assert flags.all() and (idx == 0).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_clouds_are_rejected(oracle, bad):
    S = pkg("synth")
    cur = gather(S.scenes(1, 1024, seed0=5), oracle.furthest_point_sample(S.scenes(1, 1024, seed0=5), 128))[0]
    assert prefix_predicate(cur, 32, oracle.opt_n_threads(128))[0]
    for where in (0, 7, 100):
        P = cur.copy()
        P[where, 1] = bad
        assert not prefix_predicate(P, 32, oracle.opt_n_threads(128))[0]
