"""tests/input_stage_ref.py -- the definition the device input sampler is held to (tests/test_gpu_input_stage.py) -- against itself:
the properties every branch must have, the hash against values computed by hand, and the class counts of the reference's own
sampler on the g11 scenes.  No GPU, no torch."""
import os

import numpy as np
import pytest

import input_stage_ref as R
from conftest import pkg

NP, CAP = 256, 64
SEEDS = (1024 + 7, (1 << 33) + 5, 0x80000000 + 11)


def clouds():
    rng = np.random.default_rng(11)
    return [(tri, want, R.classify(R.make_cloud(*tri, rng), R.SCOPE, R.FAR_DEPTH)) for tri, want in R.BRANCH_CASES]


def test_fmix32_hand_values_and_bijection():
    # carried through the five steps with plain integers: 1 -> 0x85ebca6b -> ^ 0x42f5e = 0x85efe535 -> * 0xc2b2ae35 -> ^ >> 16;
    # 0 is the fixed point; murmur3's published finaliser gives the same words
    assert [int(R.fmix32(v)) for v in (0, 1, 0xffffffff)] == [0, 0x514e28b7, 0x81f16f39]
    assert int(R.fmix32(0x9e3779b9)) == 0x92ca2f0e                      # sb of every seed below 2^32
    assert R.seed_words(5)[1] == R.seed_words(1024 + 99)[1] == 0x92ca2f0e != R.seed_words((1 << 33) + 5)[1]
    for base in (0, 0x7fff8000, 0xffff0000):
        out = R.fmix32(np.arange(base, base + (1 << 16), dtype=np.uint64))
        assert len(np.unique(out)) == 1 << 16 and int(out.max()) < 1 << 32
    assert np.array_equal(R.fmix32(np.uint64((1 << 32) + 77)), R.fmix32(77))          # modulo 2^32
    assert len(np.unique(R.selection_keys(70000, 1031))) == 70000


def test_every_branch_is_reached_by_its_case():
    seen = set()
    for tri, want, cls in clouds():
        for seed in SEEDS:
            trace = set()
            R.sample_choice(cls, NP, CAP, seed, trace)
            assert want <= trace, (tri, seed, trace)
            seen |= trace
    rng = np.random.default_rng(12)
    for tri, npoints, cap, want in (((500, 1500, 20), 1000, 4000, {"far_by_threshold", "near_none"}),
                                    ((0, 400, 5), 256, 0, {"far_none", "nothing_taken"})):
        trace = set()
        R.sample_choice(R.classify(R.make_cloud(*tri, rng), R.SCOPE, R.FAR_DEPTH), npoints, cap, 9, trace)
        assert want <= trace, (tri, trace)
        seen |= trace
    assert seen == set(R.BRANCHES)


def test_counts_duplicates_and_presence_on_every_branch():
    for tri, _, cls in clouds():
        near, far = np.nonzero(cls == 1)[0], np.nonzero(cls == 2)[0]
        nn, nf = len(near), len(far)
        for seed in SEEDS:
            trace = set()
            ch = R.sample_choice(cls, NP, CAP, seed, trace)
            assert ch.shape == (NP,) and ch.dtype == np.int64
            if nn + nf == 0:
                assert (ch == -1).all()
                continue
            assert (cls[ch] != 0).all()
            cnt = np.bincount(ch, minlength=len(cls))
            copies = trace & {"near_copies", "any_copies_large", "any_copies_small", "distinct_extras", "distinct_all"}
            if not copies:
                assert cnt.max() == 1                                        # no duplicate unless the branch copies
            key = R.selection_keys(len(cls), seed)
            if nn + nf > NP:
                far_keep = min(nf, CAP)
                assert int((cnt[far] > 0).sum()) == far_keep
                assert set(far[cnt[far] > 0]) == set(far[np.argsort(key[far])[:far_keep]])
                if nn >= NP - far_keep:                                      # a subset of the near class, by key
                    assert int(cnt[near].sum()) == NP - far_keep and cnt[near].max() == 1
                    assert set(near[cnt[near] > 0]) == set(near[np.argsort(key[near])[:NP - far_keep]])
                    assert int(cnt[far].sum()) == far_keep
                else:                                                        # the whole near class and copies
                    assert (cnt[near] >= 1).all() and int(cnt.sum()) == NP
                    if nn and "fallback16" not in trace:
                        assert int(cnt[far].sum()) == far_keep               # no far copy while a near point was reachable
            else:
                assert (cnt[cls != 0] >= 1).all()                            # every valid point present
                extra = NP - nn - nf
                if 0 < extra <= nn + nf:
                    valid = np.nonzero(cls)[0]
                    twice = valid[np.argsort(key[valid])[:extra]]
                    assert cnt.max() == 2 and set(np.nonzero(cnt == 2)[0]) == set(twice)


def test_redraw_falls_back_only_on_the_crafted_cloud():
    """3 near points among 64 kept far ones: a pick is near with probability 3 / 67, so some of the 189 copies miss 17 times in a
    row ((64 / 67)^17 = 0.46) and the far pick stands; with 100 near among 164 none does ((64 / 164)^17 ~ 1e-7)."""
    by_case = {tri: cls for tri, _, cls in clouds()}
    for seed in SEEDS:
        trace = set()
        ch = R.sample_choice(by_case[(3, 400, 0)], NP, CAP, seed, trace)
        assert "fallback16" in trace and int((by_case[(3, 400, 0)][ch] == 2).sum()) > CAP
        trace = set()
        ch = R.sample_choice(by_case[(100, 500, 9)], NP, CAP, seed, trace)
        assert "redraw" in trace and "fallback16" not in trace and int((by_case[(100, 500, 9)][ch] == 2).sum()) == CAP


def test_copies_pick_by_rank_in_ascending_raw_index():
    """One copy, worked by hand from the rule: 2 valid points at raw indices 3 and 9, npoints = 5 -> 3 copies with replacement."""
    cls = np.zeros(12, dtype=np.uint8)
    cls[[3, 9]] = 1
    seed = 77
    sa, sb, sc = R.seed_words(seed)
    rows = [(int(R.fmix32(3 ^ sb)), 3), (int(R.fmix32(9 ^ sb)), 9)]
    for e in range(3):
        h = int(R.fmix32(e ^ sc))
        rows.append((int(R.fmix32(h ^ sb ^ 0x51ed270b)), (3, 9)[h % 2]))
    assert R.sample_choice(cls, 5, 4000, seed).tolist() == [i for _, i in sorted(rows)]


def test_invalid_points_behind_the_cloud_change_nothing():
    for tri, _, cls in clouds():
        longer = np.concatenate([cls, np.zeros(1500, dtype=cls.dtype)])
        for seed in SEEDS[:2]:
            assert np.array_equal(R.sample_choice(cls, NP, CAP, seed), R.sample_choice(longer, NP, CAP, seed)), tri


def test_seed_changes_the_subset_but_not_the_relative_order():
    """sb is one constant for seeds below 2^32: two scenes order the raw indices they share in the same way."""
    cls = clouds()[0][2]
    a, b = R.sample_choice(cls, NP, CAP, 1024 + 5), R.sample_choice(cls, NP, CAP, 1024 + 6)
    assert not np.array_equal(np.sort(a), np.sort(b))
    shared = np.intersect1d(a, b)
    assert len(shared) > 10 and np.array_equal(a[np.isin(a, shared)], b[np.isin(b, shared)])
    c = R.sample_choice(cls, NP, CAP, (1 << 33) + 1024 + 5)                  # another high word: same subset, another order
    assert np.array_equal(np.sort(a), np.sort(c)) and not np.array_equal(a, c)


def test_classify_bounds_in_double():
    f = np.float32
    z = np.array([f(70.4), np.nextafter(f(70.4), f(0)), np.nextafter(f(70.4), f(100)), f(40), np.nextafter(f(40), f(0)), f(0),
                  np.nextafter(f(0), f(-1))], dtype=f)
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    assert R.classify(pts, R.SCOPE, R.FAR_DEPTH).tolist() == [0, 2, 0, 2, 1, 1, 0]  # f32(70.4) = 70.40000153 > 70.4
    K = pkg("kitti_io")
    img, depth = np.zeros((len(z), 2), f), np.zeros(len(z), f)
    flag = K.valid_flag(pts, img, depth, (10, 10, 3), pkg("config").default_eval_cfg().PC_AREA_SCOPE)
    assert np.array_equal(flag, R.classify(pts, R.SCOPE, R.FAR_DEPTH) > 0)


def test_reference_sampler_counts_on_the_g11_scenes(tmp_path):
    """The reference's own choice on the five fixture scenes (one per branch of its sampler) and the definition's: the same
    branch, the same count per class, the same number of distinct points."""
    import helpers
    K = pkg("kitti_io")
    cfg = pkg("config").default_eval_cfg()
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g11_input_writer_ref.npz"))
    ids = helpers.write_fake_kitti_tree(str(tmp_path), int(g["seed"]))
    src = K.KittiSource(str(tmp_path), cfg, split="val")
    N = cfg.RPN.NUM_POINTS
    branches = set()
    for sid in ids:
        _, rect, flag, _, _ = src.rect_and_flags(sid)
        assert np.array_equal(flag, np.unpackbits(g["valid_%d" % sid])[:len(flag)].astype(bool))
        cls = np.where(flag, np.where(rect[:, 2] < np.float32(40.0), 1, 2), 0)
        nv, nf = int(flag.sum()), int((cls == 2).sum())
        trace = set()
        ch = R.sample_choice(cls, N, 4000, 1024 + sid, trace)
        ref = np.nonzero(flag)[0][g["choice_%d" % sid]]
        assert (cls[ch] > 0).all()
        if nv > N:                                           # far points: all of them up to the cap, on both sides
            far_keep = min(nf, 4000)
            assert int((cls[ref] == 2).sum()) == far_keep and len(np.unique(ref[cls[ref] == 2])) == far_keep
            if nv - nf >= N - far_keep:                      # enough near points: no copies
                assert int((cls[ch] == 2).sum()) == far_keep and len(np.unique(ch)) == len(np.unique(ref)) == N
                assert trace & {"near_by_threshold", "near_exact"}
            else:                                            # too few: the reference draws the near rows with replacement, the
                assert "near_copies" in trace                # definition keeps every near point and copies the rest
                assert len(np.unique(ch)) == nv - nf + far_keep >= len(np.unique(ref))
                assert len(np.unique(ch[cls[ch] == 2])) == far_keep
        else:
            assert len(np.unique(ch)) == len(np.unique(ref)) == nv             # every valid point at least once
            if N - nv <= nv:                                 # distinct extras on both sides: nobody three times
                assert int(np.bincount(ch).max()) == int(np.bincount(ref).max()) == 2
                assert int((np.bincount(ch) == 2).sum()) == int((np.bincount(ref) == 2).sum()) == N - nv
        branches |= trace
    assert {"far_by_threshold", "far_whole", "near_by_threshold", "distinct_extras", "any_copies_small"} <= branches, branches
